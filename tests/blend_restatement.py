"""CPU restatement of sdfhip_scene_blend (include/sdfhip.h), numpy, float32 throughout, every operation an
array operation of its own in the order the header writes it -- by BRUTE FORCE: a = dist_A(p) and b = dist_B(p) are
distance_restatement.dist on each operand's Surface (every point against every triangle, twice: no search, no pruning), the value is
the smooth minimum or the morph of the two, and the tree is distance_restatement.construct's loop with this value.

np.fmax / np.fmin are C's fmaxf / fminf: they return the operand that is not a NaN, so inf - inf (two empty surfaces, or a point as
far from one as from the other at infinity) gives h = 0 and never reaches a byte.

tests/test_blend.py holds this file to things it did not come from (the offset's bytes, a bridge's closed form, volumes, the bounds
of a smooth minimum); tests/test_gpu_blend.py holds the GPU to this file, byte for byte."""
import numpy as np

import distance_restatement as dr
from edit_restatement import tree_depth

f32 = np.float32
UNION, INTERSECT, SUBTRACT, MORPH = 0, 1, 2, 3


def smin(a, b, k):
    """h = k > 0 ? fmaxf(k - fabsf(a - b), 0) / k : 0;  smin = fminf(a, b) - ((h * h) * k) * 0.25f"""
    a, b, k = np.asarray(a, dtype=f32), np.asarray(b, dtype=f32), f32(k)
    with np.errstate(all="ignore"):
        if k > f32(0):
            h = np.fmax(k - np.abs(a - b), f32(0)) / k
        else:
            h = np.zeros(np.broadcast(a, b).shape, dtype=f32)
        out = np.fmin(a, b) - ((h * h) * k) * f32(0.25)
    assert out.dtype == f32
    return out


def value_of(a, b, op, amount):
    """value by op from the two distances (float32 arrays)"""
    a, b = np.asarray(a, dtype=f32), np.asarray(b, dtype=f32)
    with np.errstate(all="ignore"):
        if op == UNION:
            out = smin(a, b, amount)
        elif op == INTERSECT:
            out = -smin(-a, -b, amount)
        elif op == SUBTRACT:
            out = -smin(-a, b, amount)
        elif op == MORPH:
            out = a + (b - a) * f32(amount)
        else:
            raise ValueError(f"unknown op {op}")
    assert out.dtype == f32
    return out


def value(surf_a, surf_b, points, op, amount):
    """value(p) for finite points (m, 3)"""
    return value_of(dr.dist(surf_a, points), dr.dist(surf_b, points), op, amount)


def blend(src_a, src_b, op, amount, depth=-1, level_a=-1, level_b=-1, want_counts=False, surf_a=None, surf_b=None):
    """sdfhip_scene_blend: src_a, src_b = (structs, values) -> (structs, values) of the new tree, breadth first.  want_counts: also
    {"depth_out", "levels", "points"}.  A morph of an empty surface is refused (ValueError), as the call refuses it."""
    surf_a = surf_a if surf_a is not None else dr.Surface(src_a[0], src_a[1], level_a)
    surf_b = surf_b if surf_b is not None else dr.Surface(src_b[0], src_b[1], level_b)
    amount = float(amount)
    if not np.isfinite(amount) or amount < 0 or (op == MORPH and amount > 1):
        raise ValueError(f"amount {amount}")
    if op == MORPH and (not len(surf_a) or not len(surf_b)):
        raise ValueError("a morph of an empty surface")
    max_depth = max(tree_depth(surf_a.structs), tree_depth(surf_b.structs)) if depth < 0 else int(depth)
    return dr.construct(lambda p: value(surf_a, surf_b, p, op, amount), max_depth, want_counts)

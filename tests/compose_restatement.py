"""CPU restatement of sdfhip_scene_compose (include/sdfhip.h), numpy, float32 throughout, every operation an
array operation of its own in the order the header writes it.  The value of one instance is place_restatement.value -- the placement
is not restated here -- the fold is fminf / fmaxf (np.fmin / np.fmax, -0 below +0) in list order, and the construct rule and the node order are the ones
place_restatement.place runs (from_float, CORNER, breadth first): the contracts cannot drift.  Every distinct point of a level is
evaluated once against every instance (np.unique, as place_restatement.node_values does): a point's value depends on the point alone.

tests/test_compose.py holds this file to things it did not come from (the placement's own restatement, the monotone byte, the closed
form of two spheres, the measured volume); tests/test_gpu_compose.py holds the GPU to this file, byte for byte."""
import numpy as np

import place_restatement as plr
from edit_restatement import tree_depth
from trimesh_restatement import CORNER, from_float

f32 = np.float32
COMBINE_UNION, COMBINE_INTERSECT, COMBINE_SUBTRACT = 0, 1, 2


def as_instances(parts):
    """parts: (src, (R, s, t)) or (src, (R, s, t), op), src = (structs, values) -> [(src, (R, s, t) as float32, op)].  The first
    op must be the union, every op a known one."""
    out = []
    for k, part in enumerate(parts):
        src, pl = part[0], part[1]
        op = COMBINE_UNION if len(part) == 2 else int(part[2])
        if op not in (COMBINE_UNION, COMBINE_INTERSECT, COMBINE_SUBTRACT) or (k == 0 and op != COMBINE_UNION):
            raise ValueError(f"instance {k}: op {op}")
        SS = np.ascontiguousarray(src[0], dtype=np.int32).reshape(-1, 2)
        SV = np.ascontiguousarray(src[1], dtype=np.uint8).reshape(-1, 8)
        out.append(((SS, SV), plr.as_placement(*pl), op))
    if not out:
        raise ValueError("no instances")
    return out


def fminf(a, b):
    """fminf as the header pins it (sdfhip_instances_*, F(p)): np.fmin, and of two zeros of opposite sign -0 whichever comes first
    (np.fmin returns its second operand there).  No byte of a composition sees the difference: from_float does not see a zero's sign"""
    r = np.fmin(a, b)
    zero = r == 0                                   # (a tie of zeros can only be where the result is one: a long list folds fast)
    if zero.any():
        r = np.where(zero & (a == 0) & (b == 0) & (np.signbit(a) | np.signbit(b)), f32(-0.0), r)
    return r


def fmaxf(a, b):
    """fmaxf as the header pins it: np.fmax, and of two zeros of opposite sign +0 whichever comes first"""
    r = np.fmax(a, b)
    zero = r == 0
    if zero.any():
        r = np.where(zero & (a == 0) & (b == 0) & ~(np.signbit(a) & np.signbit(b)), f32(0.0), r)
    return r


def value(instances, p):
    """v(p) of the rule for points p (n, 3), float32: v = u_0, then in list order fminf(v, u_k), fmaxf(v, u_k) or fmaxf(v, -u_k)"""
    v = None
    for src, (R, s, t), op in instances:
        u = plr.value(src, p, R, s, t)
        if v is None:
            v = u
        elif op == COMBINE_UNION:
            v = fminf(v, u)
        elif op == COMBINE_INTERSECT:
            v = fmaxf(v, u)
        else:
            v = fmaxf(v, -u)
    assert v.dtype == f32
    return v


def node_values(instances, coords, depth, value_of=value):
    """corner values (n, 8) and centre values (n,) of the nodes with integer coordinates coords (n, 3) at `depth`"""
    S = f32(2.0 ** -depth)
    coords = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    pts = np.concatenate([(2 * (coords[:, None, :] + CORNER[None])).reshape(-1, 3), 2 * coords + 1])     # in units of S / 2
    uniq, inv = np.unique(pts, axis=0, return_inverse=True)
    v = value_of(instances, uniq.astype(f32) * f32(S * f32(0.5)))[inv.reshape(-1)]
    n = len(coords)
    return v[:8 * n].reshape(n, 8), v[8 * n:]


def compose(parts, depth=-1, want_counts=False, value_of=value):
    """parts: see as_instances -> (structs, values) of the composed tree (new arrays), breadth first.  depth: -1 = the largest depth
    among the instances' sources, else 0..12.  want_counts: also {"depth_out", "levels", "samples"}; samples = instances * (9 for the
    root + 35 for every block of eight siblings), the look-ups the header counts.  value_of: another route to value(instances, p),
    for a list too long to evaluate instance by instance (compose_cases.folded_value, which tests/test_compose.py holds to value)."""
    instances = as_instances(parts)
    max_depth = max(tree_depth(src[0]) for src, _, _ in instances) if depth < 0 else int(depth)
    coords = np.zeros((1, 3), dtype=np.int64)
    parent = np.full(1, -1, dtype=np.int64)
    S_out, V_out = [], []
    start, d, points = 0, 0, 0
    while True:
        S = f32(2.0 ** -d)
        n = len(coords)
        points += 9 if d == 0 else 35 * (n // 8)
        cv, mv = node_values(instances, coords, d, value_of)
        V_out.append(from_float(cv, S))
        links = np.full((n, 2), -1, dtype=np.int32)
        links[:, 0] = parent
        with np.errstate(all="ignore"):
            split = np.nonzero(np.abs(mv) < f32(2) * S)[0] if d < max_depth else np.zeros(0, dtype=np.int64)
        end = start + n
        links[split, 1] = end + 8 * np.arange(len(split))
        S_out.append(links)
        if not len(split):
            break
        coords = (2 * coords[split][:, None, :] + CORNER[None]).reshape(-1, 3)
        parent = np.repeat(start + split, 8)
        start = end
        d += 1
    structs, values = np.concatenate(S_out), np.concatenate(V_out)
    if want_counts:
        return structs, values, {"depth_out": d, "levels": d + 1, "samples": len(instances) * points}
    return structs, values

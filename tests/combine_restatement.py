"""CPU restatement of sdfhip_scene_combine (include/sdfhip.h), numpy, float32 throughout, level by level
from the root down.  The decode, the interpolation and the quantisation are edit_restatement's (`decode`, `trilerp`, `quantise`,
`CHILD_T`), and the bytes an operand has where it has no node of its own are prune_restatement's `inherited`, applied once per
level: the three contracts cannot drift."""
import numpy as np

from edit_restatement import CHILD_T, F, decode, quantise, trilerp      # noqa: F401  (CHILD_T, trilerp: through `inherited`)
from prune_restatement import inherited

COMBINE_UNION, COMBINE_INTERSECT, COMBINE_SUBTRACT = 0, 1, 2
OPS = (COMBINE_UNION, COMBINE_INTERSECT, COMBINE_SUBTRACT)


def negate(b, S):
    """neg(b) = from_float(-to_float(b, S), S): byte 63 <-> 64, the sign flips exactly at the surface"""
    return quantise(-decode(b, S), S)


def combine(a, b, op, max_depth=-1, want_counts=False):
    """a, b: (structs, values) -> (structs, values) of the combination (new arrays), breadth first.  max_depth: -1 = no cut, else
    0..12.  want_counts: also {"nodes_shared": result cells that are nodes of both operands, "depth_out": the result's depth}."""
    assert op in OPS
    SA, VA = np.ascontiguousarray(a[0], dtype=np.int32).reshape(-1, 2), np.ascontiguousarray(a[1], dtype=np.uint8).reshape(-1, 8)
    SB, VB = np.ascontiguousarray(b[0], dtype=np.int32).reshape(-1, 2), np.ascontiguousarray(b[1], dtype=np.uint8).reshape(-1, 8)
    ia, ib = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)          # the operand's node at the cell, or -1
    va, vb = VA[:1].copy(), VB[:1].copy()                                      # the operand's bytes at the cell, own or inherited
    parent = np.full(1, -1, dtype=np.int64)
    S_out, V_out = [], []
    start, shared, d = 0, 0, 0
    while len(ia):
        S = F(2.0 ** -d)
        n = len(ia)
        end = start + n
        vb_op = negate(vb, S) if op == COMBINE_SUBTRACT else vb
        V_out.append(np.minimum(va, vb_op) if op == COMBINE_UNION else np.maximum(va, vb_op))
        shared += int(((ia >= 0) & (ib >= 0)).sum())
        kids_a = np.where(ia >= 0, SA[np.maximum(ia, 0), 1], -1).astype(np.int64)
        kids_b = np.where(ib >= 0, SB[np.maximum(ib, 0), 1], -1).astype(np.int64)
        split = (kids_a >= 0) | (kids_b >= 0)
        if max_depth >= 0 and d >= max_depth:
            split[:] = False
        sp = np.nonzero(split)[0]                                              # in ascending result index of the parent
        links = np.full((n, 2), -1, dtype=np.int32)
        links[:, 0] = parent
        links[sp, 1] = end + 8 * np.arange(len(sp))
        S_out.append(links)

        def children(kids, V, own):
            """the operand's side of the next level's items: its own eight records, or its bytes carried one level down"""
            has = kids[sp] >= 0
            first = np.where(has, kids[sp], 0)[:, None] + np.arange(8)
            nidx = np.where(has[:, None], first, -1).reshape(-1)
            nv = np.empty((len(sp), 8, 8), dtype=np.uint8)
            nv[has] = V[first[has]]
            nv[~has] = inherited(own[sp[~has]], d)
            return nidx, nv.reshape(-1, 8)

        ia, va = children(kids_a, VA, va)
        ib, vb = children(kids_b, VB, vb)
        parent = np.repeat(start + sp, 8)
        start = end
        d += 1
    structs, values = np.concatenate(S_out), np.concatenate(V_out)
    if want_counts:
        return structs, values, {"nodes_shared": shared, "depth_out": d - 1}
    return structs, values

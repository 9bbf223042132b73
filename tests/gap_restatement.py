"""CPU restatement of sdfhip_instances_gap (include/sdfhip.h), numpy, float32 throughout, every operation an
array operation of its own in the order the header writes it -- by BRUTE FORCE: the surface is penetration_restatement.surface_of's
(mesh_restatement's triangles in emitted order), a world vertex is penetration_restatement.forward_map of an emitted position, r_k is
penetration_restatement.searched (every vertex against every triangle of the other part) and the flag's containment is
clash_restatement.contains.  The candidates of a pair are concatenated direction 0 then direction 1, each in emitted order, and argmin
takes the first: the lowest (direction, node, 3 k + v).  There is no search tree, no bound, no broad phase and no atomic here.  The
records are the C dtype.

tests/test_gap.py holds this file to things it did not come from (the list reversed, the limit on either side of a gap, two balls in
closed form, the witness as an emitted vertex); tests/test_gpu_gap.py holds the GPU to this file, byte for byte."""
import numpy as np

import clash_restatement as clr
import penetration_restatement as pr
import place_restatement as plr

f32 = np.float32
GAP = np.dtype([("a", "<u4"), ("b", "<u4"), ("gap", "<f4"), ("flags", "<u4"), ("node_a", "<u4"), ("node_b", "<u4"), ("corner", "<u4"),
                ("point_a", "<f4", (3,)), ("point_b", "<f4", (3,)), ("pad_", "<u4", (3,))])
assert GAP.itemsize == 64
WITNESS_OF_B, CONTAINED = 1, 2


def candidates(instance):
    """(world vertices (3 T, 3), node (3 T,), corner (3 T,)) of one instance's surface in emitted order: triangle-major, then the
    vertex; corner = 3 k + v with k the triangle's index among its cell's"""
    src, (R, s, t), _ = instance
    surf = pr.surface_of(src)
    T = len(surf)
    if T == 0:
        return np.zeros((0, 3), f32), np.zeros(0, np.int64), np.zeros(0, np.int64)
    cell = surf.cell
    assert (np.diff(cell) >= 0).all()                                   # emitted order: node ascending
    first = np.searchsorted(cell, cell, side="left")                    # the first triangle of each triangle's cell
    k = np.arange(T) - first
    w = pr.forward_map(surf.pos.reshape(-1, 3), R, s, t)
    return w, np.repeat(cell, 3), (3 * k[:, None] + np.arange(3)[None]).reshape(-1)


def _searched(instance, w):
    """penetration_restatement.searched at the points w, each distinct point (bit for bit) held against the surface once: a cut vertex
    is a vertex of several triangles, and an answer depends on the point alone"""
    uniq, inv = np.unique(np.ascontiguousarray(w).view(np.uint32), axis=0, return_inverse=True)
    r, node, near = pr.searched(instance, uniq.view(f32))
    inv = inv.reshape(-1)
    return r[inv], node[inv], near[inv]


def gap(instances, limit=np.inf, want_counts=False):
    """instances: compose_restatement.as_instances' list, 1..64 of them -> the records of every pair a < b whose gap is <= limit (and
    below +inf), in (a, b) order.  want_counts: also {"searches"}: SDFHIP_GAP_NO_PRUNE's count, the sum over the ordered pairs with
    two non-empty surfaces of 3 x the triangles of the first part"""
    K = len(instances)
    if not 1 <= K <= clr.MAX_INSTANCES:
        raise ValueError(f"{K} instances")
    limit = f32(limit)
    if np.isnan(limit) or limit < 0:
        raise ValueError(f"limit {limit}")
    cand = [candidates(inst) for inst in instances]
    out, searches = [], 0
    for a in range(K):
        for b in range(a + 1, K):
            if not len(cand[a][0]) or not len(cand[b][0]):
                continue
            searches += len(cand[a][0]) + len(cand[b][0])
            found = [_searched(instances[b], cand[a][0]), _searched(instances[a], cand[b][0])]
            r = np.concatenate([found[0][0], found[1][0]])
            r = np.where(np.isnan(r), f32(np.inf), r)                   # a NaN never wins
            assert r.dtype == f32 and (r >= 0).all()
            i = int(r.argmin())                                         # the first of the minima: the lowest (direction, node, corner)
            g = r[i]
            if not g < f32(np.inf) or not g <= limit:
                continue
            second = i >= len(cand[a][0])
            j = i - len(cand[a][0]) if second else i
            mine, other = (b, a) if second else (a, b)
            w = cand[mine][0][j]
            far_node, far_point = found[second][1][j], found[second][2][j]
            held = bool(clr.contains([instances[other]], w[None])[0, 0]) or bool(clr.contains([instances[mine]], far_point[None])[0, 0])
            flags = (WITNESS_OF_B if second else 0) | (CONTAINED if held else 0)
            node, point = cand[mine][1][j], w
            na, nb, pa, pb = (far_node, node, far_point, point) if second else (node, far_node, point, far_point)
            out.append((a, b, g, flags, na, nb, cand[mine][2][j], pa, pb, (0, 0, 0)))
    rec = np.array(out, dtype=GAP) if out else np.zeros(0, GAP)
    if want_counts:
        return rec, {"searches": searches}
    return rec


def gap_vector(rec):
    """point_b - point_a of a record"""
    return (np.asarray(rec["point_b"], dtype=f32) - np.asarray(rec["point_a"], dtype=f32)).astype(f32)

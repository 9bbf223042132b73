"""CPU restatement of sdfhip_scene_prune (include/sdfhip.h), numpy, float32 throughout, level by level from
the deepest up.  The decode, the interpolation and the quantisation are edit_restatement's own (`decode`, `trilerp`, `quantise`,
`CHILD_T`): the bytes a block is compared with are exactly the bytes sdfhip_scene_edit gives a new child before the brush touches
it, so the two contracts cannot drift."""
import numpy as np

from edit_restatement import CHILD_T, F, HALF, decode, quantise, trilerp


def levels(structs):
    """[indices of the nodes of depth 0, 1, ...] (int64), by the children links from the root"""
    out, level = [], np.zeros(1, dtype=np.int64)
    while len(level):
        out.append(level)
        kids = structs[level, 1]
        kids = kids[kids >= 0].astype(np.int64)
        level = (kids[:, None] + np.arange(8)).reshape(-1)
    return out


def inherited(parent_bytes, d):
    """(m, 8) bytes of internal nodes of depth d -> (m, 8 children, 8 corners) bytes q(i, k): the parent's decoded corners,
    interpolated at the child's corners and quantised at the child's scale"""
    S = F(2.0 ** -d)
    f = decode(parent_bytes, S)[:, None, None, :]
    v = trilerp(f, CHILD_T[None, :, :, 0], CHILD_T[None, :, :, 1], CHILD_T[None, :, :, 2]).astype(F)
    return quantise(v, S * HALF)


def prune(structs, values, tolerance=0, max_depth=-1):
    """-> (structs, values) of the pruned tree (new arrays).  tolerance: 0..255 (-1 = 0); max_depth: -1 = no cut, else 0..12."""
    structs = np.ascontiguousarray(structs, dtype=np.int32).reshape(-1, 2)
    values = np.ascontiguousarray(values, dtype=np.uint8).reshape(-1, 8)
    tol = 0 if tolerance < 0 else int(tolerance)
    n = len(structs)
    leaf = structs[:, 1] < 0                                  # a leaf, or a node that has become one
    removed = np.zeros(n, dtype=bool)
    by_depth = levels(structs)
    for d in range(len(by_depth) - 1, -1, -1):
        idx = by_depth[d]
        P = idx[structs[idx, 1] >= 0]                         # the internal nodes of depth d: one block of eight each
        if not len(P):
            continue
        kids = structs[P, 1].astype(np.int64)[:, None] + np.arange(8)
        all_leaves = leaf[kids].all(1)
        if max_depth >= 0 and d + 1 > max_depth:
            close = np.ones(len(P), dtype=bool)
        else:
            q = inherited(values[P], d).astype(np.int32)
            close = (np.abs(values[kids].astype(np.int32) - q) <= tol).all((1, 2))
        gone = all_leaves & close
        removed[kids[gone].reshape(-1)] = True
        leaf[P[gone]] = True
    keep = ~removed
    new = np.cumsum(keep) - 1                                 # a survivor's index: the survivors with a lower old index
    S = structs[keep].copy()
    inner = S[:, 1] >= 0
    collapsed = inner & leaf[keep]
    S[collapsed, 1] = -1
    live = inner & ~collapsed
    S[live, 1] = new[S[live, 1]]
    S[1:, 0] = new[S[1:, 0]]
    return S, values[keep].copy()


def split_leaves(structs, values):
    """Every leaf split once, its eight children appended with the inherited bytes (what an edit whose brush changes nothing would
    add): pruning the result at tolerance 0 gives what pruning the input gives."""
    structs = np.ascontiguousarray(structs, dtype=np.int32).reshape(-1, 2)
    values = np.ascontiguousarray(values, dtype=np.uint8).reshape(-1, 8)
    S, V = [structs.copy()], [values]
    n = len(structs)
    for d, idx in enumerate(levels(structs)):
        L = idx[structs[idx, 1] < 0]
        if not len(L):
            continue
        S[0][L, 1] = n + 8 * np.arange(len(L))
        blk = np.empty((8 * len(L), 2), dtype=np.int32)
        blk[:, 0] = np.repeat(L, 8)
        blk[:, 1] = -1
        S.append(blk)
        V.append(inherited(values[L], d).reshape(-1, 8))
        n += 8 * len(L)
    return np.concatenate(S), np.concatenate(V)

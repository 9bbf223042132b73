"""CPU restatement of sdfhip_scene_mesh (include/sdfhip.h), numpy, float32 throughout.  It visits EVERY
node: depth and cell coordinates come from a walk up the parent links of all nodes at once, whether their bytes are mixed or not --
the GPU's shortcuts (only mixed cells walk, counts before vertices) are not restated, so the tests hold the GPU to the rule.  The
orientation table is derived here from the rule (unit tetrahedron, cuts at the edge midpoints); the library's constant table is not
read.  Normals are py_restatement_vec.ShaderV.gradient with the cursor put on the cell, times 1 / sqrt(dot(g, g)).

tests/test_mesh.py holds this file to things it did not make (pinned counts, closedness, orientation, the frozen oracle's
distances); tests/test_gpu_mesh.py holds the GPU to this file, byte for byte."""
import itertools

import numpy as np

from py_restatement_vec import ShaderV, normalize

f32 = np.float32
SURFACE = f32(63.75)          # (b / 255 - 0.25) * 2 S == 0; no byte equals it: inside <=> b <= 63

# the Kuhn decomposition: six tetrahedra round the diagonal 0-7, one per axis permutation in lexicographic order
PERMS = list(itertools.permutations(range(3)))
TETS = np.array([[0, 1 << a0, (1 << a0) | (1 << a1), 7] for a0, a1, _ in PERMS], dtype=np.int64)      # cube corners v0..v3
CORNER = np.array([[k & 1, (k >> 1) & 1, (k >> 2) & 1] for k in range(8)], dtype=np.float64)


def _triangles_of(tet, mask):
    """The triangles of tetrahedron `tet` for inside-mask `mask` (bit i: local corner i inside), each three cut edges (i, j), i < j,
    in the pinned order, oriented counter-clockwise seen from outside by the rule's test on the unit tetrahedron."""
    ins = [i for i in range(4) if mask >> i & 1]
    outs = [i for i in range(4) if not mask >> i & 1]
    if not ins or not outs:
        return []
    if len(ins) in (1, 3):
        cut = sorted((min(i, o), max(i, o)) for i in ins for o in outs)
        tris = [cut]
    else:
        (i0, i1), (o0, o1) = ins, outs
        q = [tuple(sorted(e)) for e in ((i0, o0), (i0, o1), (i1, o1), (i1, o0))]
        tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    P = CORNER[TETS[tet]]
    mid = lambda e: (P[e[0]] + P[e[1]]) / 2
    outward = P[outs].mean(0) - P[ins].mean(0)
    out = []
    for a, b, c in tris:
        ccw = np.dot(np.cross(mid(b) - mid(a), mid(c) - mid(a)), outward) > 0
        out.append((a, b, c) if ccw else (a, c, b))
    return out


TABLE = [[_triangles_of(t, m) for m in range(16)] for t in range(6)]
NTRI = np.array([0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0], dtype=np.int64)     # by mask: 1 or 3 inside -> 1, 2 inside -> 2
assert all(len(TABLE[t][m]) == NTRI[m] for t in range(6) for m in range(16))


def walk(structs):
    """Every node's depth and integer cell coordinates (n, 3) of its depth, from the links: a node's octant within its parent is
    index - parent.children (bit order x + 2y + 4z); the coordinates collect the octant bits on the way up to the root."""
    S = np.ascontiguousarray(structs, dtype=np.int32).reshape(-1, 2)
    n = len(S)
    cur = np.arange(n, dtype=np.int64)
    depth = np.zeros(n, dtype=np.int32)
    c = np.zeros((n, 3), dtype=np.int32)
    for k in range(64):
        par = S[cur, 0].astype(np.int64)
        up = par >= 0
        if not up.any():
            return depth, c
        w = np.nonzero(up)[0]
        octant = (cur[w] - S[par[w], 1]).astype(np.int32)
        if ((octant < 0) | (octant > 7)).any():
            raise ValueError("mesh restatement: inconsistent links")
        for a in range(3):
            c[w, a] |= ((octant >> a) & 1) << k
        depth[w] += 1
        cur[w] = par[w]
    raise ValueError("mesh restatement: a parent chain of more than 64 links")


def cells_of(structs, level, depth):
    """The cell set of `level` as a mask over the nodes: -1 = the leaves; L = the leaves of depth <= L and the internal nodes of
    depth exactly L."""
    leaf = np.asarray(structs).reshape(-1, 2)[:, 1] < 0
    if level < 0:
        return leaf
    return (leaf & (depth <= level)) | (~leaf & (depth == level))


def count(structs, values, level=-1, walked=None):
    """(cells, cells_cut, n_triangles) without making a vertex.  walked: walk(structs), when the caller has it already."""
    V = np.ascontiguousarray(values, dtype=np.uint8).reshape(-1, 8)
    depth, _ = walked if walked is not None else walk(structs)
    cell = cells_of(structs, level, depth)
    cut = np.nonzero(cell & (V.min(1) <= 63) & (V.max(1) > 63))[0]
    B = V[cut]
    total = 0
    for t in range(6):
        ins = B[:, TETS[t]] <= 63
        total += int(NTRI[ins[:, 0] + 2 * ins[:, 1] + 4 * ins[:, 2] + 8 * ins[:, 3]].sum())
    return int(cell.sum()), len(cut), total


def mesh(structs, values, level=-1, want_cells=False, chunk=1 << 20, walked=None):
    """sdfhip_scene_mesh: (n_triangles, 3, 6) float32 {position, normal}, cells in ascending node index, tetrahedra and triangles in
    the pinned order.  want_cells: also each triangle's node index and (cells, cells_cut)."""
    S = np.ascontiguousarray(structs, dtype=np.int32).reshape(-1, 2)
    V = np.ascontiguousarray(values, dtype=np.uint8).reshape(-1, 8)
    depth, coord = walked if walked is not None else walk(S)
    cell = cells_of(S, level, depth)
    cut = np.nonzero(cell & (V.min(1) <= 63) & (V.max(1) > 63))[0]           # ascending node index
    B = V[cut]
    m = len(cut)
    masks = np.zeros((m, 6), dtype=np.int64)
    for t in range(6):
        ins = B[:, TETS[t]] <= 63
        masks[:, t] = ins[:, 0] + 2 * ins[:, 1] + 4 * ins[:, 2] + 8 * ins[:, 3]
    per = NTRI[masks]                                                        # (m, 6)
    first = np.concatenate([[0], np.cumsum(per.reshape(-1))])                # triangle offset of (cell, tetrahedron)
    T = int(first[-1])
    tri_cell = np.zeros(T, dtype=np.int64)                                   # rank of the triangle's cell in `cut`
    lo = np.zeros((T, 3), dtype=np.int64)                                    # cube corners of each vertex's cut edge
    hi = np.zeros((T, 3), dtype=np.int64)
    for t in range(6):
        for mk in range(1, 15):
            sel = np.nonzero(masks[:, t] == mk)[0]
            if not len(sel):
                continue
            for k, tri in enumerate(TABLE[t][mk]):
                at = first[sel * 6 + t] + k
                tri_cell[at] = sel
                for v, (i, j) in enumerate(tri):
                    lo[at, v] = TETS[t][i]
                    hi[at, v] = TETS[t][j]
    out = np.zeros((T, 3, 6), dtype=f32)
    sh = ShaderV(S, V, bytes(112))
    for a0 in range(0, T, chunk):
        a1 = min(T, a0 + chunk)
        k = np.repeat(tri_cell[a0:a1], 3)                                    # per vertex
        l, h = lo[a0:a1].reshape(-1), hi[a0:a1].reshape(-1)
        node = cut[k]
        scale = np.ldexp(f32(1), -depth[node]).astype(f32)
        bl, bh = B[k, l].astype(f32), B[k, h].astype(f32)
        t = ((SURFACE - bl).astype(f32) / (bh - bl).astype(f32)).astype(f32)
        pos, lower = [], []
        for a in range(3):
            la, ha = (l >> a) & 1, (h >> a) & 1
            base = (coord[node, a].astype(np.int64) + la).astype(f32)
            pos.append(((base + np.where(ha != la, t, f32(0)).astype(f32)).astype(f32) * scale).astype(f32))
            lower.append((coord[node, a].astype(f32) * scale).astype(f32))
        sh.index, sh.lower, sh.scale = node.astype(np.int64), lower, scale
        with np.errstate(all="ignore"):
            nrm = normalize(sh.gradient(pos))
        flat = out[a0:a1].reshape(-1, 6)
        for a in range(3):
            flat[:, a] = pos[a]
            flat[:, 3 + a] = nrm[a]
    if want_cells:
        return out, cut[tri_cell], (int(cell.sum()), m)
    return out


def same_bytes(got, want):
    """float32 arrays equal bit for bit, NaN equal to NaN"""
    a, b = np.ascontiguousarray(got, dtype=f32), np.ascontiguousarray(want, dtype=f32)
    if a.shape != b.shape:
        return False
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def edges(tris):
    """The directed edges of a triangle soup, endpoints keyed by the bits of their positions: (3 n, 2) int64 keys (a, b) of the
    edges 0->1, 1->2, 2->0 of every triangle, and the number of distinct positions."""
    p = np.ascontiguousarray(tris[:, :, :3], dtype=f32).reshape(-1, 3)
    _, key = np.unique(p.view(np.uint32).reshape(-1, 3), axis=0, return_inverse=True)
    key = key.reshape(-1, 3).astype(np.int64)
    return np.stack([key.reshape(-1), np.roll(key, -1, axis=1).reshape(-1)], 1), int(key.max()) + 1 if len(key) else 0


def closedness(tris):
    """-> (undirected edges, edges not shared by exactly two triangles, shared edges both triangles traverse the same way,
    distinct positions, degenerate edges)"""
    e, nv = edges(tris)
    degenerate = int((e[:, 0] == e[:, 1]).sum())
    und = np.sort(e, axis=1)
    uniq, inv, cnt = np.unique(und, axis=0, return_inverse=True, return_counts=True)
    forward = (e[:, 0] < e[:, 1]).astype(np.int64)
    fsum = np.bincount(inv.reshape(-1), weights=forward, minlength=len(uniq))
    same_way = int(((cnt == 2) & (fsum != 1)).sum())
    return len(uniq), int((cnt != 2).sum()), same_way, nv, degenerate

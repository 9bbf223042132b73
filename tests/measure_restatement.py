"""CPU restatement of sdfhip_scene_measure (include/sdfhip.h), numpy, float64 throughout, vectorised over
cells.  The cells, their depth and coordinates, the six tetrahedra and the triangles of a (tetrahedron, mask) are mesh_restatement's
own (walk, cells_of, TETS, TABLE, CORNER), so the mesh's contract and this one cannot drift.  Every operation is one numpy call on
float64 arrays, rounded on its own in the order the rule writes; the one float32 operation is the triangle area's root.  The sums
over cells are the adjacent-pair tree over node index, done here literally (tree_sum).

tests/test_measure.py holds this file to things it did not come from (the mesh restatement's triangles by the divergence theorem,
exact one-node cases, closed forms); tests/test_gpu_measure.py holds the GPU to this file, byte for byte."""
import numpy as np

from mesh_restatement import CORNER, TABLE, TETS, cells_of, walk

f64 = np.float64
SUMS = ("volume", "area", "m1x", "m1y", "m1z", "m2xx", "m2yy", "m2zz", "m2xy", "m2xz", "m2yz")
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))                     # moment2: xx, yy, zz, xy, xz, yz
BIT = CORNER.astype(np.int64)                                                # (8, 3): bit_a(k)


def _pieces(mask):
    """The signed tetrahedra of one Kuhn tetrahedron clipped to `mask` (bit i: local corner i inside), in the rule's order.  A vertex
    is ("c", i), local corner i, or ("p", lo, hi), the cut point on the edge between local corners lo < hi."""
    ins = [i for i in range(4) if mask >> i & 1]
    outs = [i for i in range(4) if not mask >> i & 1]
    C = lambda i: ("c", i)
    P = lambda i, o: ("p", min(i, o), max(i, o))
    whole = (C(0), C(1), C(2), C(3))
    if len(ins) == 4:
        return [(+1, whole)]
    if len(ins) == 1:
        i0 = ins[0]
        return [(+1, (C(i0), P(i0, outs[0]), P(i0, outs[1]), P(i0, outs[2])))]
    if len(ins) == 3:
        o0 = outs[0]
        return [(+1, whole), (-1, (C(o0), P(ins[0], o0), P(ins[1], o0), P(ins[2], o0)))]
    if len(ins) == 2:
        (i0, i1), (o0, o1) = ins, outs
        q0, q1, q2, q3 = P(i0, o0), P(i0, o1), P(i1, o1), P(i1, o0)
        return [(+1, (C(i0), q0, q1, q2)), (+1, (C(i0), q0, q3, q2)), (+1, (C(i0), C(i1), q3, q2))]
    return []


PIECES = [_pieces(m) for m in range(16)]


def tree_sum(x):
    """The adjacent-pair tree over the index: pad with +0.0 to a power of two, x = x[0::2] + x[1::2] until one value is left."""
    x = np.asarray(x, dtype=f64)
    m = 1
    while m < len(x):
        m *= 2
    y = np.zeros(m, dtype=f64)
    y[:len(x)] = x
    while len(y) > 1:
        y = y[0::2] + y[1::2]
    return f64(y[0])


def _tet(a, b, c, d):
    """volume, first and second moments (m, 3), (m, 6) of the tetrahedra (a, b, c, d), each (m, 3)"""
    e1, e2, e3 = b - a, c - a, d - a
    det = ((e1[:, 0] * (e2[:, 1] * e3[:, 2] - e2[:, 2] * e3[:, 1]) - e1[:, 1] * (e2[:, 0] * e3[:, 2] - e2[:, 2] * e3[:, 0]))
           + e1[:, 2] * (e2[:, 0] * e3[:, 1] - e2[:, 1] * e3[:, 0]))
    V = np.abs(det) / 6.0
    s = ((a + b) + c) + d
    m1 = (V * 0.25)[:, None] * s
    w = V * 0.05
    m2 = np.stack([w * ((((a[:, i] * a[:, j] + b[:, i] * b[:, j]) + c[:, i] * c[:, j]) + d[:, i] * d[:, j]) + s[:, i] * s[:, j])
                   for i, j in PAIRS], 1)
    return V, m1, m2


class Measured:
    """The fields of sdfhip_measure (without the times)"""
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def sums(self):
        return np.concatenate([[self.volume, self.area], self.moment1, self.moment2]).astype(f64)

    def doubles(self):
        """the seventeen doubles in the struct's order"""
        return np.concatenate([self.sums(), self.bounds_min, self.bounds_max]).astype(f64)

    def counts(self):
        """cells, cells_cut, cells_inside, cells_at_depth[13]"""
        return np.concatenate([[self.cells, self.cells_cut, self.cells_inside], self.cells_at_depth]).astype(np.int64)

    @property
    def centroid(self):
        return None if self.volume == 0 else self.moment1 / self.volume


def measure(structs, values, level=-1, walked=None):
    """sdfhip_scene_measure: a Measured.  walked: walk(structs), when the caller has it already."""
    S = np.ascontiguousarray(structs, dtype=np.int32).reshape(-1, 2)
    V8 = np.ascontiguousarray(values, dtype=np.uint8).reshape(-1, 8)
    n = len(S)
    depth, coord = walked if walked is not None else walk(S)
    cell = cells_of(S, level, depth)
    inside8 = V8 <= 63
    full = np.nonzero(cell & inside8.all(1))[0]
    cut = np.nonzero(cell & inside8.any(1) & ~inside8.all(1))[0]
    x = np.zeros((len(SUMS), n), dtype=f64)                                  # every node's contribution: +0.0 unless it is a cell with an inside corner
    lo_all, hi_all = np.full(3, np.inf), np.full(3, -np.inf)

    def bound(p):
        nonlocal lo_all, hi_all
        if len(p):
            lo_all, hi_all = np.minimum(lo_all, p.min(0)), np.maximum(hi_all, p.max(0))

    # -- the cells with all eight bytes <= 63: boxes
    if len(full):
        Sc = np.ldexp(f64(1), -depth[full].astype(np.int64))
        c = coord[full].astype(f64)
        lo, hi = c * Sc[:, None], (c + 1.0) * Sc[:, None]
        Vb = (Sc * Sc) * Sc
        mid = (lo + hi) * 0.5
        x[0, full] = Vb
        for a in range(3):
            x[2 + a, full] = Vb * mid[:, a]
            x[5 + a, full] = Vb * (((lo[:, a] * lo[:, a] + lo[:, a] * hi[:, a]) + hi[:, a] * hi[:, a]) / 3.0)
        for k, (i, j) in enumerate(PAIRS[3:]):
            x[8 + k, full] = Vb * (mid[:, i] * mid[:, j])
        bound(lo)
        bound(hi)

    # -- the cells with mixed bytes: six tetrahedra each, clipped
    m = len(cut)
    acc = np.zeros((len(SUMS), m), dtype=f64)                                # cell-local sums, from +0.0
    if m:
        B = V8[cut]
        cc = coord[cut].astype(np.int64)
        Sc = np.ldexp(f64(1), -depth[cut].astype(np.int64))
        for t in range(6):
            tet = TETS[t]
            ins = B[:, tet] <= 63
            masks = ins[:, 0] + 2 * ins[:, 1] + 4 * ins[:, 2] + 8 * ins[:, 3]
            for mk in range(1, 16):
                sel = np.nonzero(masks == mk)[0]
                if not len(sel):
                    continue
                c, s1, b = cc[sel], Sc[sel][:, None], B[sel]
                made = {}

                def vertex(v):
                    if v not in made:
                        if v[0] == "c":
                            made[v] = (c.astype(f64) + CORNER[tet[v[1]]]) * s1
                        else:
                            lo, hi = int(tet[v[1]]), int(tet[v[2]])          # cube corners: the bits of lo are a subset of hi's
                            tt = (63.75 - b[:, lo].astype(f64)) / (b[:, hi].astype(f64) - b[:, lo].astype(f64))
                            differ = BIT[lo] != BIT[hi]
                            made[v] = ((c + BIT[lo]).astype(f64) + np.where(differ[None, :], tt[:, None], 0.0)) * s1
                    return made[v]

                local = acc[:, sel]                                           # gathered once, scattered once: the order per cell is kept
                for sign, verts in PIECES[mk]:
                    Vt, m1, m2 = _tet(*(vertex(v) for v in verts))
                    if sign > 0:
                        local[0] = local[0] + Vt
                        local[2:5] = local[2:5] + m1.T
                        local[5:11] = local[5:11] + m2.T
                    else:
                        local[0] = local[0] - Vt
                        local[2:5] = local[2:5] - m1.T
                        local[5:11] = local[5:11] - m2.T
                for tri in TABLE[t][mk]:
                    p0, p1, p2 = (vertex(("p", i, j)) for i, j in tri)
                    u, v = p1 - p0, p2 - p0
                    nx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
                    ny = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
                    nz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
                    n2 = (nx * nx + ny * ny) + nz * nz
                    local[1] = local[1] + 0.5 * np.sqrt(n2.astype(np.float32)).astype(f64)
                acc[:, sel] = local
                # the bounds: the inside corners and the cut points
                for i in range(4):
                    if mk >> i & 1:
                        bound(vertex(("c", i)))
                        for o in range(4):
                            if not mk >> o & 1:
                                bound(vertex(("p", min(i, o), max(i, o))))
        x[:, cut] = acc

    sums = np.array([tree_sum(x[k]) for k in range(len(SUMS))], dtype=f64)
    at_depth = np.bincount(depth[cell], minlength=13).astype(np.int64)
    if len(at_depth) > 13:
        raise ValueError("measure restatement: a tree deeper than 12 levels")
    return Measured(volume=sums[0], area=sums[1], moment1=sums[2:5].copy(), moment2=sums[5:11].copy(), bounds_min=lo_all, bounds_max=hi_all,
                    nodes=n, depth=int(depth.max()), cells=int(cell.sum()), cells_cut=m, cells_inside=len(full), cells_at_depth=at_depth)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=f64), np.ascontiguousarray(b, dtype=f64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def mesh_volume_area(tris):
    """Divergence-theorem volume and summed triangle areas of a closed triangle soup (n, 3, >= 3), in float64"""
    p = np.asarray(tris, dtype=f64)[:, :, :3]
    a, b, c = p[:, 0], p[:, 1], p[:, 2]
    vol = np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0
    area = 0.5 * np.sqrt((np.cross(b - a, c - a) ** 2).sum(1)).sum()
    return abs(float(vol)), float(area)

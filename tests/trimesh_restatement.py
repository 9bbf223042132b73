"""CPU restatement of sdfhip_trimesh_prepare / sdfhip_trimesh_build (include/sdfhip.h), numpy.

prepare() is its own double-precision preparation (weld, dropped triangles, face normals, angle-weighted pseudonormals).  The
distance is the pinned rule in np.float32, every operation an array operation of its own in the order written, and the winner is
found by BRUTE FORCE over all records: no candidate lists, no pruning -- so the tests hold the GPU's pruning to the rule.
build_pruned() is the same tree computed the way the GPU computes it -- candidate lists, the pruning threshold in np.float32 -- held to
build() by tests/test_trimesh.py on the adversarial soups at the end of this file; it gives the GPU's `candidate_entries` exactly.

tests/test_trimesh.py holds this file to things it did not make (closed-form box and sphere distances, the cube's known
pseudonormals); tests/test_gpu_trimesh.py holds the GPU to this file, byte for byte."""
import numpy as np

f32 = np.float32
REGION_NORMAL = {0: 9, 1: 12, 2: 15, 3: 18, 4: 21, 5: 24, 6: 27}     # face, edges ab bc ca, vertices a b c -> first float of N


def fit_positions(P, fill=0.8):
    """fit = 1, pinned: fp32, mid = (lo + hi) * 0.5f, s = fill / max(hi - lo), p' = (p - mid) * s + 0.5f"""
    P = np.asarray(P, dtype=f32)
    lo, hi = P.reshape(-1, 3).min(0), P.reshape(-1, 3).max(0)
    mid = (lo + hi) * f32(0.5)
    s = f32(fill) / (hi - lo).max()
    return (P - mid) * s + f32(0.5), s, mid


def prepare(tris, fit=0, fill=0.8):
    """tris (n, 3, 3) -> (records (m, 32) float32, counts dict).  Double precision from the fp32 positions."""
    P = np.ascontiguousarray(tris, dtype=f32).reshape(-1, 3, 3)
    if fit:
        P = fit_positions(P, fill)[0]
    P = P + f32(0.0)                                           # -0 -> +0
    D = P.astype(np.float64)
    a, b, c = D[:, 0], D[:, 1], D[:, 2]
    n = np.cross(b - a, c - a)
    ln = np.sqrt((n * n).sum(1))
    longest = np.maximum(((b - a) ** 2).sum(1), np.maximum(((c - a) ** 2).sum(1), ((c - b) ** 2).sum(1)))
    area = 0.5 * ln
    keep = (area > 0) & ~(area < 2.0 ** -40 * longest)
    kept = np.nonzero(keep)[0]
    P, D, face = P[kept], D[kept], n[kept] / ln[kept, None]
    # weld by bits
    _, vid = np.unique(P.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    vid = vid.reshape(-1, 3)
    nv = int(vid.max()) + 1
    vsum = np.zeros((nv, 3))
    esum, ecount = {}, {}
    for t in range(len(P)):
        for k in range(3):
            u, v = D[t, (k + 1) % 3] - D[t, k], D[t, (k + 2) % 3] - D[t, k]
            cr = np.cross(u, v)
            vsum[vid[t, k]] += np.arctan2(np.sqrt(cr @ cr), u @ v) * face[t]
            e = (min(vid[t, k], vid[t, (k + 1) % 3]), max(vid[t, k], vid[t, (k + 1) % 3]))
            esum[e] = esum.get(e, 0.0) + face[t]
            ecount[e] = ecount.get(e, 0) + 1

    def unit_or(s, fallback):
        l = np.sqrt(s @ s)
        return s / l if l > 0 and np.isfinite(l) else fallback

    R = np.zeros((len(P), 32), dtype=f32)
    R[:, 0:9] = P.reshape(-1, 9)
    R[:, 9:12] = face
    for t in range(len(P)):
        for k in range(3):
            e = (min(vid[t, k], vid[t, (k + 1) % 3]), max(vid[t, k], vid[t, (k + 1) % 3]))
            R[t, 12 + 3 * k:15 + 3 * k] = unit_or(esum[e], face[t])
            R[t, 21 + 3 * k:24 + 3 * k] = unit_or(vsum[vid[t, k]], face[t])
    R[:, 30] = kept.astype(np.uint32).view(f32)
    counts = dict(n_vertices=nv, n_edges=len(esum), n_records=len(P), n_dropped=int((~keep).sum()),
                  open_edges=sum(1 for v in ecount.values() if v != 2))
    return R, counts


def _dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def dist2(R, p):
    """D, r = p - q and the region of points p (m, 3) against records R (n, 32): arrays (m, n).  fp32, the rule's order."""
    R = np.asarray(R, dtype=f32)
    p = np.asarray(p, dtype=f32).reshape(-1, 3)
    return _dist2([R[None, :, k] for k in range(3)], [R[None, :, 3 + k] for k in range(3)], [R[None, :, 6 + k] for k in range(3)],
                  [p[:, k, None] for k in range(3)])


def _dist2(a, b, c, P):
    """the rule on float32 arrays that broadcast against each other: vertices a, b, c and points P, each a list of three"""
    with np.errstate(all="ignore"):
        ab = [b[k] - a[k] for k in range(3)]
        ac = [c[k] - a[k] for k in range(3)]
        ap = [P[k] - a[k] for k in range(3)]
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = [P[k] - b[k] for k in range(3)]
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = [P[k] - c[k] for k in range(3)]
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e0, e1 = d4 - d3, d5 - d6
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e0 >= 0) & (e1 >= 0)]
        regions = [4, 5, 1, 6, 3, 2]
        tab = d1 / (d1 - d3)
        tca = d2 / (d2 - d6)
        tbc = e0 / (e0 + e1)
        den = f32(1.0) / ((va + vb) + vc)
        fv, fw = vb * den, vc * den
        shape = np.broadcast(d1).shape
        qs = [[np.broadcast_to(a[k], shape) for k in range(3)], [np.broadcast_to(b[k], shape) for k in range(3)],
              [a[k] + ab[k] * tab for k in range(3)], [np.broadcast_to(c[k], shape) for k in range(3)],
              [a[k] + ac[k] * tca for k in range(3)], [b[k] + (c[k] - b[k]) * tbc for k in range(3)]]
        q = [(a[k] + ab[k] * fv) + ac[k] * fw for k in range(3)]
        region = np.zeros(shape, dtype=np.int8)
        for cond, reg, qq in reversed(list(zip(conds, regions, qs))):          # the first condition that holds wins
            q = [np.where(cond, qq[k], q[k]) for k in range(3)]
            region = np.where(cond, np.int8(reg), region)
        r = [P[k] - q[k] for k in range(3)]
        D = _dot(r, r)
    assert D.dtype == f32
    return D, r, region


def values(R, p, chunk=None):
    """The signed distance (float32, before quantisation) of points p (m, 3): brute force over all records of R."""
    R = np.asarray(R, dtype=f32)
    p = np.asarray(p, dtype=f32).reshape(-1, 3)
    out = np.empty(len(p), dtype=f32)
    chunk = chunk or max(1, 400_000 // max(1, len(R)))
    for s in range(0, len(p), chunk):
        D, r, region = dist2(R, p[s:s + chunk])
        Dm = np.where(np.isnan(D), f32(np.inf), D)
        win = Dm.argmin(1)                                     # the first minimum: the lowest record index
        rows = np.arange(len(win))
        Dw = Dm[rows, win]
        reg = region[rows, win].astype(np.int64)
        N0 = np.array([REGION_NORMAL[k] for k in range(7)])[reg]
        Nw = [R[win, N0 + k] for k in range(3)]
        sgn = _dot([r[k][rows, win] for k in range(3)], Nw)
        with np.errstate(all="ignore"):
            d = np.sqrt(Dw)
            out[s:s + chunk] = np.where(np.isinf(Dw), f32(np.inf), np.where(sgn < 0, -d, d))
    return out


CORNER = np.array([[k & 1, k >> 1 & 1, k >> 2 & 1] for k in range(8)], dtype=np.int64)


def from_float(d, S):
    """FromFloat, SdfGen/dllmain.cpp:192-196, float32"""
    with np.errstate(all="ignore"):
        normd = d / f32(2) / f32(S)
        sat = np.minimum(np.maximum(normd + f32(0.25), f32(0)), f32(1))
        return np.floor(sat * f32(255)).astype(np.uint8)


def node_values(R, coords, depth):
    """corner values (n, 8) and centre values (n,) of nodes with integer coordinates coords (n, 3) at `depth`: every distinct point
    is evaluated once"""
    S = f32(2.0 ** -depth)
    coords = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    pts = np.concatenate([(2 * (coords[:, None, :] + CORNER[None])).reshape(-1, 3), 2 * coords + 1])     # in units of S / 2
    uniq, inv = np.unique(pts, axis=0, return_inverse=True)
    v = values(R, uniq.astype(f32) * f32(S * f32(0.5)))[inv.reshape(-1)]
    n = len(coords)
    return v[:8 * n].reshape(n, 8), v[8 * n:]


def build(R, max_depth, want_float=False):
    """structs (n, 2) int32, values (n, 8) uint8 in the pinned breadth-first order; with want_float also, per level, (coords,
    corner values, centre values) before quantisation"""
    structs, vals, floats = [[-1, -1]], [], []
    coords = np.zeros((1, 3), dtype=np.int64)
    base = 0
    for depth in range(max_depth + 1):
        S = f32(2.0 ** -depth)
        cv, mv = node_values(R, coords, depth)
        floats.append((coords, cv, mv))
        vals.append(from_float(cv, S))
        if depth == max_depth:
            break
        split = np.nonzero(np.abs(mv) < f32(2) * S)[0]
        if len(split) == 0:
            break
        nxt = base + len(coords)
        for k, node in enumerate(split):
            structs[base + node][1] = nxt + 8 * k
            structs.extend([base + node, -1] for _ in range(8))
        base, coords = nxt, (2 * coords[split][:, None, :] + CORNER[None]).reshape(-1, 3)
    out = (np.array(structs, dtype=np.int32), np.concatenate(vals))
    return out + (floats,) if want_float else out


# point `p` of a block of eight siblings, in units of S / 2 from twice the block's first child: the 27 corners of its 3x3x3 lattice
# (i + 3j + 9k), then the 8 child centres
BLOCK_POINT = np.array([[2 * (p % 3), 2 * (p // 3 % 3), 2 * (p // 9)] for p in range(27)] + (2 * CORNER + 1).tolist(), dtype=np.int64)
CORNER_POINT = np.array([[(c & 1) + (k & 1) + 3 * ((c >> 1 & 1) + (k >> 1 & 1)) + 9 * ((c >> 2 & 1) + (k >> 2 & 1)) for k in range(8)]
                         for c in range(8)])                   # [child, corner] -> lattice point


def build_pruned(R, max_depth, want_lists=False):
    """build()'s tree the way the GPU computes it (csrc/trigen_kernels.h): a node's corners and centre are evaluated
    against its PARENT's candidate list (the root against all records), and a splitting node's own list is the parent-list records
    with sqrt(D(centre, r)) <= T, T = reach + (slack_abs + reach * 2^-10), reach = |value(centre)| + 2 * (S * 0.8660255f),
    slack_abs = max(1, max |coordinate|) * 2^-14, all np.float32 in this order.  Lists stay in ascending record index.
    -> structs, values, candidate_entries (the sum over the blocks of siblings of their list length, the root's block n_records);
    with want_lists also, per level, the blocks' list lengths."""
    R = np.asarray(R, dtype=f32)
    slack_abs = np.maximum(f32(1), np.abs(R[:, :9]).max()) * f32(2.0 ** -14)
    structs, vals, lengths = [[-1, -1]], [], []
    bcoord = np.zeros((1, 3), dtype=np.int64)                   # the blocks' parents (the root's: a cell of edge 2 at the origin)
    lists = [np.arange(len(R), dtype=np.int64)]
    nchild, base, entries = 1, 0, 0
    for depth in range(max_depth + 1):
        S = f32(2.0 ** -depth)
        cnt = np.array([len(l) for l in lists])
        lengths.append(cnt)
        entries += int(cnt.sum())
        cv, mv, keep = [], [], []
        step = max(1, 4_000 // int(cnt.max()))                 # blocks at a time
        for s in range(0, len(lists), step):
            n = cnt[s:s + step]
            rec = np.concatenate(lists[s:s + step])
            blk = np.repeat(np.arange(len(n)), n)
            seg = np.concatenate([[0], np.cumsum(n)[:-1]])
            pts = ((4 * bcoord[s:s + step, None, :] + BLOCK_POINT[None]).astype(f32) * f32(S * f32(0.5)))[blk]      # (entries, 35, 3)
            D, r, region = _dist2([R[rec, k, None] for k in range(3)], [R[rec, 3 + k, None] for k in range(3)],
                                  [R[rec, 6 + k, None] for k in range(3)], [pts[:, :, k] for k in range(3)])
            Dm = np.where(np.isnan(D), f32(np.inf), D)
            Dw = np.minimum.reduceat(Dm, seg, axis=0)           # (blocks, 35)
            row = np.arange(len(rec))[:, None]
            win = np.minimum.reduceat(np.where(Dm == Dw[blk], row, len(rec)), seg, axis=0)     # the first minimum: the lowest index
            col = np.arange(35)[None]
            N0 = np.array([REGION_NORMAL[k] for k in range(7)])[region[win, col]]
            sgn = _dot([r[k][win, col] for k in range(3)], [R[rec[win], N0 + k] for k in range(3)])
            with np.errstate(all="ignore"):
                d = np.sqrt(Dw)
                v = np.where(np.isinf(Dw), f32(np.inf), np.where(sgn < 0, -d, d))
                m = v[:, 27:27 + nchild]
                cv.append(v[:, CORNER_POINT[:nchild]].reshape(-1, 8))
                mv.append(m.reshape(-1))
                reach = np.abs(m) + f32(2) * (S * f32(0.8660255))
                T = reach + (slack_abs + reach * f32(2.0 ** -10))
                keep.append(np.sqrt(D[:, 27:27 + nchild]) <= T[blk])
        cv, mv = np.concatenate(cv), np.concatenate(mv)
        vals.append(from_float(cv, S))
        if depth == max_depth:
            break
        split = np.nonzero(np.abs(mv) < f32(2) * S)[0]
        if len(split) == 0:
            break
        nxt = base + len(mv)
        for k, node in enumerate(split):
            structs[base + node][1] = nxt + 8 * k
            structs.extend([base + node, -1] for _ in range(8))
        keep = np.split(np.concatenate(keep), np.cumsum(cnt)[:-1])
        new = [lists[node // nchild][keep[node // nchild][:, node % nchild]] for node in split]
        bcoord = 2 * bcoord[split // nchild] + CORNER[split % nchild]
        lists, base, nchild = new, nxt, 8
    out = (np.array(structs, dtype=np.int32), np.concatenate(vals), entries)
    return out + (lengths,) if want_lists else out


# ---- the tests' solids: triangle soups (n, 3, 3) float32, counter-clockwise seen from outside -------------------------------------
def _quad(q, first=0):
    q = q[first:] + q[:first]
    return [(q[0], q[1], q[2]), (q[0], q[2], q[3])]


def cube(lo=0.25, hi=0.75):
    """twelve triangles, the faces' diagonals chosen so that the corners meet 3, 3, 4, 4, 5, 5, 6 and 6 triangles"""
    tris = []
    faces = [(a, s) for a in range(3) for s in (0, 1)]
    for (axis, side), first in zip(faces, (0, 0, 0, 0, 0, 1)):
        u, v = [(1, 2), (2, 0), (0, 1)][axis]
        q = []
        for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):
            c = [0, 0, 0]
            c[axis], c[u], c[v] = side, du, dv
            q.append(tuple(c))
        if side == 0:
            q = q[::-1]
        tris += _quad(q, first)
    return (np.array(tris, dtype=np.float64) * (hi - lo) + lo).astype(f32)


def tetrahedron():
    v = np.array([[0.3, 0.3, 0.3], [0.8, 0.35, 0.3], [0.4, 0.8, 0.35], [0.45, 0.45, 0.8]])
    faces = [(0, 2, 1), (0, 1, 3), (1, 2, 3), (0, 3, 2)]
    return np.array([[v[i] for i in f] for f in faces]).astype(f32)


L_REFLEX = 0.21 + 0.29        # the reflex edge of l_prism: x = y = L_REFLEX, z in [0.3, 0.7]


def l_prism():
    """an L-shaped prism along z: 20 triangles, a reflex (concave) edge at x = y = L_REFLEX whose end vertices are saddles"""
    poly = [(0, 0), (2, 0), (2, 1), (1, 1), (1, 2), (0, 2)]
    cap = [(0, 1, 3), (1, 2, 3), (0, 3, 5), (3, 4, 5)]
    z0, z1 = 0.3, 0.7
    P = lambda i, z: (0.21 + 0.29 * poly[i][0], 0.21 + 0.29 * poly[i][1], z)
    tris = [[P(a, z1), P(b, z1), P(c, z1)] for a, b, c in cap] + [[P(a, z0), P(c, z0), P(b, z0)] for a, b, c in cap]
    for i in range(6):
        j = (i + 1) % 6
        tris += _quad([P(i, z0), P(j, z0), P(j, z1), P(i, z1)])
    return np.array(tris).astype(f32)


# ---- adversarial soups (tests/test_trimesh.py, tests/test_gpu_trimesh.py): what the pruning, the tie rule and NaN have to survive ---
def _strips(n, x0, x1, y0, y1, slope_x, slope_y):
    """an open sheet z = 0.5 + slope_x * x + slope_y * (y - 0.5) of n strips along x (two triangles each), facing +z"""
    z = lambda x, y: 0.5 + slope_x * x + slope_y * (y - 0.5)
    tris = []
    for j in range(n):
        ya, yb = y0 + (y1 - y0) * j / n, y0 + (y1 - y0) * (j + 1) / n
        tris += _quad([(x0, ya, z(x0, ya)), (x1, ya, z(x1, ya)), (x1, yb, z(x1, yb)), (x0, yb, z(x0, yb))])
    return np.array(tris).astype(f32)


def strips_far():
    """16 tilted strips from x = -950 to 955 through the cube: 32 long thin triangles, an open mesh, B = 955"""
    return _strips(16, -950.0, 955.0, 0.1, 0.9, 2e-4, 0.25)


def strips_fine():
    """64 tilted strips of width 0.0125 (the depth-5 cell is 0.03125) and length 5"""
    return _strips(64, -2.3, 2.7, 0.1, 0.9, 0.03, -0.2)


def cone_fan(n=200):
    """n triangles around one apex inside the cube, their ring (radius 12) 40 below it: an open fan of valence n"""
    apex = (0.5, 0.5, 0.6)
    ring = [(0.5 + 12.0 * np.cos(2 * np.pi * k / n), 0.5 + 12.0 * np.sin(2 * np.pi * k / n), 0.6 - 40.0) for k in range(n)]
    return np.array([[apex, ring[(k + 1) % n], ring[k]] for k in range(n)]).astype(f32)


def two_sheets(nx=32, ny=17, x0=0.375, y0=0.4375, step=2.0 ** -7):
    """Two open sheets facing +z, B at z = 0.625 and A at z = 0.375, each nx x ny squares of edge `step` from (x0, y0) (dyadic), two
    triangles a square, row by row: m = 2 nx ny triangles a sheet, 1088 by default.  Sheet B comes first, then sheet A in the same
    order, so a triangle of A is 1088 records behind its mirror image: never in the same chunk of 1024, always one wave of 64
    further on, which is a LOWER wave for the 64 of every 1024 that wrap round.  A point on z = 0.5 over the sheets has bit-equal
    D to a record and its image and opposite signs (below B: inside, record i; above A: outside, record m + i)."""
    tris = []
    for z in (0.625, 0.375):
        for j in range(ny):
            for i in range(nx):
                xa, xb, ya, yb = x0 + i * step, x0 + (i + 1) * step, y0 + j * step, y0 + (j + 1) * step
                tris += _quad([(xa, ya, z), (xb, ya, z), (xb, yb, z), (xa, yb, z)])
    return np.array(tris).astype(f32)


def far_away():
    """a closed cube at coordinates 900 .. 1000: the root alone, every byte saturated"""
    return cube(900.0, 1000.0)


def cube_fit():
    """the L-prism scaled and shifted off the cube: for fit = 1"""
    return (l_prism() * f32(37.5) - f32(11.0)) * np.array([1.0, 0.6, 0.3], dtype=f32)


def sliver():
    """The cube and one more triangle that prepare keeps (its area is a quarter of its longest edge squared) and whose fp32 D is
    NaN at the lattice points (0, y, z), y > 0: a right triangle of legs 2^-100 at the origin.  ab . ab = 2^-200 is 0 in fp32, so
    with ab . ap = 0 edge ab's parameter d1 / (d1 - d3) is 0 / 0.
    How it was found: NOT as the thin triangle the name promises.  Three seeded searches (240 M point-triangle pairs: random
    slivers in the cube, c within 10^-8 .. 10^-5 of the line ab; the same along lines through lattice points) met no NaN on the
    depth-4 lattice.  A sliver's (va + vb) + vc does cancel to 0 at hundreds of lattice points, but the face branch is reached only
    past three edge tests, and va + vb + vc = 0 needs one of va, vb, vc <= 0 with the point inside that edge's span, which that
    edge's test takes first.  What is left is 0 / 0 on an edge, which needs |ab|^2 to underflow: a speck, not a sliver."""
    e = 2.0 ** -100
    return np.concatenate([cube(), np.array([[(0, 0, 0), (e, 0, 0), (0, e, 0)]], dtype=f32)])


ADVERSARIAL = dict(strips_far=0, strips_fine=0, cone_fan=0, two_sheets=0, far_away=0, cube_fit=1, sliver=0)          # name -> fit

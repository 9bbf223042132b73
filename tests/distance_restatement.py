"""CPU restatement of sdfhip_scene_distance and sdfhip_scene_offset (include/sdfhip.h), numpy, float32
throughout, every operation an array operation of its own in the order the header writes it -- by BRUTE FORCE: the surface is
mesh_restatement.mesh's triangles, d2 is trimesh_restatement._dist2 against every one of them, folded with the minimum a NaN never
wins, the sign is query_restatement.sample's distance at the clamped point, and the tree is place_restatement's construct loop with
this value.  There is no search and no pruning here: that is the point of it.

tests/test_distance.py holds this file to things it did not come from (a plane's closed form, a sphere's radius, volumes);
tests/test_gpu_distance.py holds the GPU's search to this file, bit for bit."""
import numpy as np

import mesh_restatement as mr
import query_restatement as qr
from edit_restatement import tree_depth
from trimesh_restatement import CORNER, _dist2, from_float

f32 = np.float32
GROW, SHELL = 0, 1
HIT, INVALID = qr.HIT, qr.INVALID

# the C record (include/sdfhip.h), field for field
CLEARANCE = np.dtype({"names": ["distance", "node", "nearest", "status", "visited", "pad_"],
                      "formats": ["<f4", "<u4", ("<f4", (3,)), "<u4", "<u4", "<u4"], "offsets": [0, 4, 8, 20, 24, 28], "itemsize": 32})


class Surface:
    """surface(scene, level): the emitted positions (T, 3, 3) float32 in emitted order, and each triangle's cell (node index)"""

    def __init__(self, structs, values, level=-1):
        self.structs = np.ascontiguousarray(structs, dtype=np.int32).reshape(-1, 2)
        self.values = np.ascontiguousarray(values, dtype=np.uint8).reshape(-1, 8)
        self.level = level
        tris, cells, _ = mr.mesh(self.structs, self.values, level, want_cells=True)
        self.pos = np.ascontiguousarray(tris[:, :, :3], dtype=f32)
        self.cell = np.asarray(cells, dtype=np.int64)

    def __len__(self):
        return len(self.pos)


def nearest(surf, points, budget=1 << 18):
    """d2 (m,), the winning triangle (m,; -1 where d2 is +inf) and r = p - q of that triangle (m, 3), for finite points (m, 3):
    every point against every triangle, `budget` pairs at a time.  Of the triangles that tie the lowest index wins (argmin's first)."""
    p = np.asarray(points, dtype=f32).reshape(-1, 3)
    m, T = len(p), len(surf)
    best = np.full(m, np.inf, dtype=f32)
    win = np.full(m, -1, dtype=np.int64)
    r_out = np.zeros((m, 3), dtype=f32)
    if T == 0 or m == 0:
        return best, win, r_out
    a = [surf.pos[None, :, 0, k] for k in range(3)]
    b = [surf.pos[None, :, 1, k] for k in range(3)]
    c = [surf.pos[None, :, 2, k] for k in range(3)]
    step = max(1, budget // T)
    for s in range(0, m, step):
        P = [p[s:s + step, k, None] for k in range(3)]
        D, r, _ = _dist2(a, b, c, P)
        Dm = np.where(np.isnan(D), f32(np.inf), D)                 # a NaN never wins
        w = Dm.argmin(1)
        rows = np.arange(len(w))
        d = Dm[rows, w]
        found = d < f32(np.inf)                                    # best = t < best ? t : best, from +inf
        best[s:s + step] = d
        win[s:s + step] = np.where(found, w, -1)
        for k in range(3):
            r_out[s:s + step, k] = np.where(found, np.broadcast_to(r[k], D.shape)[rows, w], f32(0))
    return best, win, r_out


def inside(surf, points):
    """sign(p) < 0: the sampled distance at the point clamped to the cube is below zero"""
    p = np.asarray(points, dtype=f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        pc = np.fmin(np.fmax(p, f32(0)), f32(1))
    return qr.sample(surf.structs, surf.values, pc)["distance"].astype(f32) < f32(0)


def dist(surf, points):
    """dist(p) = sign(p) * sqrtf(d2(p)) for finite points (m, 3)"""
    p = np.asarray(points, dtype=f32).reshape(-1, 3)
    best, _, _ = nearest(surf, p)
    with np.errstate(all="ignore"):
        root = np.sqrt(best)
    out = np.where(inside(surf, p), -root, root)
    assert out.dtype == f32
    return out


def distance(structs, values, points, level=-1, surf=None):
    """sdfhip_scene_distance: CLEARANCE records (`visited` is not restated: it stays 0)"""
    surf = surf if surf is not None else Surface(structs, values, level)
    p = np.asarray(points, dtype=f32).reshape(-1, 3)
    out = np.zeros(len(p), CLEARANCE)
    ok = np.isfinite(p).all(1)
    out["status"] = np.where(ok, HIT, INVALID)
    q = p[ok]
    if not len(q):
        return out
    best, win, r = nearest(surf, q)
    with np.errstate(all="ignore"):
        root = np.sqrt(best)
    found = win >= 0
    out["distance"][ok] = np.where(inside(surf, q), -root, root)
    out["node"][ok] = np.where(found, surf.cell[np.maximum(win, 0)] if len(surf) else 0, 0)
    near = np.zeros((len(q), 3), dtype=f32)
    for k in range(3):
        near[:, k] = np.where(found, q[:, k] - r[:, k], f32(0))
    out["nearest"][ok] = near
    return out


def value(surf, points, mode, amount):
    """value(p): GROW dist - amount; SHELL fabsf(dist) - amount * 0.5f"""
    d = dist(surf, points)
    with np.errstate(all="ignore"):
        out = d - f32(amount) if mode == GROW else np.abs(d) - f32(amount) * f32(0.5)
    assert out.dtype == f32
    return out


def construct(value_of, max_depth, want_counts=False):
    """place_restatement.place's construct loop with value_of(points (m, 3) float32) -> (m,) float32 as the value: byte =
    FromFloat(value(corner), S), a node splits iff fabsf(value(centre)) < 2 S && d < max_depth, breadth first; every distinct point
    of a level is evaluated once (a point's value depends on the point alone)."""
    coords = np.zeros((1, 3), dtype=np.int64)
    parent = np.full(1, -1, dtype=np.int64)
    S_out, V_out = [], []
    start, d, points = 0, 0, 0
    while True:
        S = f32(2.0 ** -d)
        n = len(coords)
        points += 9 if d == 0 else 35 * (n // 8)
        pts = np.concatenate([(2 * (coords[:, None, :] + CORNER[None])).reshape(-1, 3), 2 * coords + 1])     # in units of S / 2
        uniq, inv = np.unique(pts, axis=0, return_inverse=True)
        v = value_of(uniq.astype(f32) * f32(S * f32(0.5)))[inv.reshape(-1)]
        assert v.dtype == f32
        cv, mv = v[:8 * n].reshape(n, 8), v[8 * n:]
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
        return structs, values, {"depth_out": d, "levels": d + 1, "points": points}
    return structs, values


def offset(src, mode, amount, depth=-1, level=-1, want_counts=False, surf=None):
    """sdfhip_scene_offset: src = (structs, values) -> (structs, values) of the new tree, breadth first.  want_counts: also
    {"depth_out", "levels", "points"}."""
    surf = surf if surf is not None else Surface(src[0], src[1], level)
    max_depth = tree_depth(surf.structs) if depth < 0 else int(depth)
    return construct(lambda p: value(surf, p, mode, amount), max_depth, want_counts)


def grow(src, delta, depth=-1, level=-1, **kw):
    return offset(src, GROW, delta, depth, level, **kw)


def shell(src, thickness, depth=-1, level=-1, **kw):
    return offset(src, SHELL, thickness, depth, level, **kw)

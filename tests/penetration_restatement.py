"""CPU restatement of sdfhip_instances_penetration (include/sdfhip.h), numpy, float32 throughout, every
operation an array operation of its own in the order the header writes it -- by BRUTE FORCE: the lattice and the containment are
clash_restatement's, the inverse map is place_restatement's, and every contained point of every part is held against every triangle of
distance_restatement.Surface (distance_restatement.nearest).  There is no search tree, no skip, no item list and no atomic here.  The
records are the C dtype.

tests/test_penetration.py holds this file to things it did not come from (the clash restatement's counts, distance_restatement's
distance, the list reversed, the closed form of a lens); tests/test_gpu_penetration.py holds the GPU to this file, byte for byte."""
import numpy as np

import clash_restatement as clr
import distance_restatement as dr
import place_restatement as plr

f32 = np.float32
PENETRATION = np.dtype([("a", "<u4"), ("b", "<u4"), ("points", "<u4"), ("witness", "<u4"), ("depth", "<f4"), ("ra", "<f4"), ("rb", "<f4"),
                        ("node_a", "<u4"), ("node_b", "<u4"), ("nearest_a", "<f4", (3,)), ("nearest_b", "<f4", (3,)), ("pad_", "<u4")])
assert PENETRATION.itemsize == 64

_surfaces = {}


def surface_of(src):
    """distance_restatement.Surface of a source's arrays at full detail, made once per pair of arrays (which the caller keeps alive)"""
    key = (src[0].ctypes.data, src[1].ctypes.data)
    if key not in _surfaces:
        _surfaces[key] = (dr.Surface(src[0], src[1], -1), src)
    return _surfaces[key][0]


def forward_map(x, R, s, t):
    """((R[i][0] x_0 + R[i][1] x_1) + R[i][2] x_2) * s + t_i for points x (n, 3), float32"""
    R, s, t = plr.as_placement(R, s, t)
    with np.errstate(all="ignore"):
        out = np.stack([((R[i, 0] * x[:, 0] + R[i, 1] * x[:, 1]) + R[i, 2] * x[:, 2]) * s + t[i] for i in range(3)], 1)
    assert out.dtype == f32
    return out


def searched(instance, p):
    """(r (m,), node (m,), nearest (m, 3) in world coordinates) of one instance at the world points p (m, 3): r = sqrtf(d2(q)) * s with
    q the inverse map of p; a part without a surface: r = +inf, node 0, nearest 0"""
    src, (R, s, t), _ = instance
    R, s, t = plr.as_placement(R, s, t)
    surf = surface_of(src)
    q = np.stack(plr.inverse_map(p, R, s, t), 1)
    assert q.dtype == f32
    best, win, r = dr.nearest(surf, q)
    with np.errstate(all="ignore"):
        radius = np.sqrt(best) * s
    assert radius.dtype == f32
    found = win >= 0
    node = np.where(found, surf.cell[np.maximum(win, 0)] if len(surf) else 0, 0)
    near = forward_map((q - r).astype(f32), R, s, t)
    near[~found] = f32(0)
    return radius, node, near


def penetration(instances, depth=6, origin=(0.0, 0.0, 0.0), side=1.0, want_counts=False):
    """instances: compose_restatement.as_instances' list, 1..64 of them -> the records of every pair a < b that shares a lattice
    point, in (a, b) order.  want_counts: also {"searches"}: the sum over the points inside two or more parts of the parts holding them"""
    K = len(instances)
    if not 1 <= K <= clr.MAX_INSTANCES:
        raise ValueError(f"{K} instances")
    p = clr.lattice(depth, origin, side)[0]
    inside = clr.contains(instances, p)
    multi = inside.sum(0) >= 2
    at = [np.nonzero(inside[k] & multi)[0] for k in range(K)]
    # an instance that repeats an earlier one -- the same arrays under the same placement -- reuses its answers
    seen, found = {}, []
    for k, (src, (R, s, t), _) in enumerate(instances):
        R, s, t = plr.as_placement(R, s, t)
        key = (src[0].ctypes.data, src[1].ctypes.data, R.tobytes(), s.tobytes(), t.tobytes())
        if key not in seen:
            seen[key] = searched(instances[k], p[at[k]]) if len(at[k]) else (np.zeros(0, f32), np.zeros(0, np.int64), np.zeros((0, 3), f32))
        found.append(seen[key])
    out = []
    for a in range(K):
        for b in range(a + 1, K):
            both = np.nonzero(inside[a] & inside[b])[0]
            if not len(both):
                continue
            ia, ib = np.searchsorted(at[a], both), np.searchsorted(at[b], both)
            assert (at[a][ia] == both).all() and (at[b][ib] == both).all()
            ra, rb = found[a][0][ia], found[b][0][ib]
            m = np.fmin(ra, rb)
            assert not np.isnan(m).any() and (m >= 0).all()
            w = int(m.argmax())                                         # the first of the maxima: the lowest index
            out.append((a, b, len(both), both[w], m[w], ra[w], rb[w], found[a][1][ia[w]], found[b][1][ib[w]], found[a][2][ia[w]], found[b][2][ib[w]], 0))
    rec = np.array(out, dtype=PENETRATION) if out else np.zeros(0, PENETRATION)
    if want_counts:
        return rec, {"searches": int(inside[:, multi].sum())}
    return rec

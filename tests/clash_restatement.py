"""CPU restatement of sdfhip_instances_clash (include/sdfhip.h), numpy, on place_restatement.value: every
instance is looked up at every lattice point -- no skip, no blocks -- and every pair is counted over the whole lattice at once.  The
records are the C dtype.

tests/test_clash.py holds this file to things it did not come from (counts pinned from a prototype written another way, the octant
partition, the list reversed, compose_restatement's fold, the closed form of a lens); tests/test_gpu_clash.py holds the GPU to this
file, byte for byte."""
import numpy as np

import place_restatement as plr
from py_restatement_vec import fma

f32 = np.float32
MAX_INSTANCES, MAX_DEPTH = 64, 10
CLASH = np.dtype([("a", "<u4"), ("b", "<u4"), ("points", "<u4"), ("first", "<u4"), ("lo", "<u4", (3,)), ("hi", "<u4", (3,)), ("sum", "<u8", (3,))])
assert CLASH.itemsize == 64


def pitch_of(depth, side=1.0):
    """pitch = side * 2^-d, float32"""
    return f32(side) * f32(2.0 ** -int(depth))


def lattice(depth, origin=(0.0, 0.0, 0.0), side=1.0):
    """(points (8^d, 3) float32 in linear-index order, x (8^d,), y, z as int64): p_a = fmaf((float)i_a + 0.5f, pitch, origin_a),
    index = (z << 2d) | (y << d) | x"""
    d = int(depth)
    if not 0 <= d <= MAX_DEPTH:
        raise ValueError(f"depth {d}")
    n = 1 << d
    o = np.asarray(origin, dtype=f32).reshape(3)
    half = np.arange(n, dtype=f32) + f32(0.5)
    axis = [fma(half, np.full(n, pitch_of(d, side), f32), np.full(n, o[a], f32)).astype(f32) for a in range(3)]
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    x, y, z = x.reshape(-1), y.reshape(-1), z.reshape(-1)
    return np.stack([axis[0][x], axis[1][y], axis[2][z]], 1), x.astype(np.int64), y.astype(np.int64), z.astype(np.int64)


def contains(instances, p):
    """(K, n) bool: instance k contains p iff u_k(p) < 0 (a NaN contains nothing); the ops are ignored.  An instance that repeats an
    earlier one -- the same arrays under the same placement -- reuses its row: a value depends on the point alone"""
    seen, rows = {}, []
    for src, (R, s, t), _ in instances:
        key = (src[0].ctypes.data, src[1].ctypes.data, R.tobytes(), s.tobytes(), t.tobytes())
        if key not in seen:
            with np.errstate(invalid="ignore"):
                seen[key] = plr.value(src, p, R, s, t) < f32(0)
        rows.append(seen[key])
    return np.stack(rows)


def clash(instances, depth=6, origin=(0.0, 0.0, 0.0), side=1.0):
    """instances: compose_restatement.as_instances' list, 1..64 of them -> the records of every pair a < b that shares a lattice
    point, in (a, b) order"""
    K = len(instances)
    if not 1 <= K <= MAX_INSTANCES:
        raise ValueError(f"{K} instances")
    p, x, y, z = lattice(depth, origin, side)
    inside = contains(instances, p)
    index = (z << (2 * int(depth))) | (y << int(depth)) | x
    assert (index == np.arange(len(p))).all()
    out = []
    for a in range(K):
        for b in range(a + 1, K):
            at = np.nonzero(inside[a] & inside[b])[0]
            if not len(at):
                continue
            c = np.stack([x[at], y[at], z[at]], 1)
            out.append((a, b, len(at), index[at].min(), c.min(0), c.max(0), c.sum(0)))
    return np.array(out, dtype=CLASH) if out else np.zeros(0, CLASH)

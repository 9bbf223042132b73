"""CPU restatement of sdfhip_volume_build and sdfhip_scene_volume (include/sdfhip.h), numpy, float32
throughout, every operation an array operation of its own in the order the header writes it.  The bytes and the corner table are
trimesh_restatement's from_float and CORNER, the construct rule is the one place_restatement.place runs, and the out direction's
distance D is query_restatement.sample's (find from the root + interpol_world: the shader's arithmetic): the contracts cannot drift.
Every distinct point of a level is evaluated once (np.unique): a point's value depends on the point alone.

tests/test_volume.py holds this file to things it did not come from (the analytic builder's sphere, vertex exactness, the
continuation, the structure of the result); tests/test_gpu_volume.py holds the GPU to this file, byte for byte."""
import numpy as np

import query_restatement as qr
from trimesh_restatement import CORNER, from_float

f32 = np.float32


def as_lattice(origin, spacing):
    return np.asarray(origin, dtype=f32).reshape(3), f32(spacing)


def axis(p, o, inv, spacing, n):
    """one axis of the rule for coordinates p (float32 array): the cell i, the weight f in it, and e, how far p lies outside"""
    with np.errstate(all="ignore"):
        g = (p - o) * inv
        gc = np.fmin(np.fmax(g, f32(0)), f32(n - 1))             # (fmaxf / fminf: a NaN becomes 0)
        e = (g - gc) * spacing
        i = np.minimum(gc.astype(np.int64), n - 2)
        f = gc - i.astype(f32)
    return i, f, e


def lerp(u, v, f):
    return u * (f32(1) - f) + v * f


def value(grid, p, origin, spacing, value_scale=1.0):
    """value(p) of the build's rule for points p (n, 3): grid (nz, ny, nx), float32 or float16"""
    grid = np.asarray(grid)
    assert grid.ndim == 3 and grid.dtype in (np.float32, np.float16) and min(grid.shape) >= 2
    nz, ny, nx = grid.shape
    flat = grid.reshape(-1)
    o, spacing = as_lattice(origin, spacing)
    scale = f32(value_scale)
    p = np.asarray(p, dtype=f32).reshape(-1, 3)
    inv = f32(1) / spacing
    i, fx, ex = axis(p[:, 0], o[0], inv, spacing, nx)
    j, fy, ey = axis(p[:, 1], o[1], inv, spacing, ny)
    k, fz, ez = axis(p[:, 2], o[2], inv, spacing, nz)
    at = lambda di, dj, dk: flat[((k + dk) * ny + (j + dj)) * nx + (i + di)].astype(f32)      # (the F16 conversion is exact)
    with np.errstate(all="ignore"):
        c00 = lerp(at(0, 0, 0), at(1, 0, 0), fx)
        c10 = lerp(at(0, 1, 0), at(1, 1, 0), fx)
        c01 = lerp(at(0, 0, 1), at(1, 0, 1), fx)
        c11 = lerp(at(0, 1, 1), at(1, 1, 1), fx)
        c0 = lerp(c00, c10, fy)
        c1 = lerp(c01, c11, fy)
        D = lerp(c0, c1, fz)
        out = D * scale + np.sqrt((ex * ex + ey * ey) + ez * ez)
    assert out.dtype == f32
    return out


def node_values(grid, coords, depth, origin, spacing, value_scale):
    """corner values (n, 8) and centre values (n,) of the nodes with integer coordinates coords (n, 3) at `depth`"""
    S = f32(2.0 ** -depth)
    coords = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    pts = np.concatenate([(2 * (coords[:, None, :] + CORNER[None])).reshape(-1, 3), 2 * coords + 1])     # in units of S / 2
    uniq, inv = np.unique(pts, axis=0, return_inverse=True)
    v = value(grid, uniq.astype(f32) * f32(S * f32(0.5)), origin, spacing, value_scale)[inv.reshape(-1)]
    n = len(coords)
    return v[:8 * n].reshape(n, 8), v[8 * n:]


def build(grid, origin, spacing, depth, value_scale=1.0, want_counts=False):
    """-> (structs, values) of the tree of the grid's value, breadth first.  want_counts: also {"depth_out", "levels", "samples"};
    samples = 9 for the root + 35 for every block of eight siblings."""
    max_depth = int(depth)
    coords = np.zeros((1, 3), dtype=np.int64)
    parent = np.full(1, -1, dtype=np.int64)
    S_out, V_out = [], []
    start, d, samples = 0, 0, 0
    while True:
        S = f32(2.0 ** -d)
        n = len(coords)
        samples += 9 if d == 0 else 35 * (n // 8)
        cv, mv = node_values(grid, coords, d, origin, spacing, value_scale)
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
        return structs, values, {"depth_out": d, "levels": d + 1, "samples": samples}
    return structs, values


def lattice_points(shape, origin, spacing):
    """the positions (n, 3) of a lattice's elements in storage order (x fastest): p_a = origin_a + (float)i_a * spacing"""
    nz, ny, nx = shape
    o, spacing = as_lattice(origin, spacing)
    with np.errstate(all="ignore"):
        x = o[0] + np.arange(nx).astype(f32) * spacing
        y = o[1] + np.arange(ny).astype(f32) * spacing
        z = o[2] + np.arange(nz).astype(f32) * spacing
    p = np.empty((nz, ny, nx, 3), dtype=f32)
    p[..., 0] = x[None, None, :]
    p[..., 1] = y[None, :, None]
    p[..., 2] = z[:, None, None]
    return p.reshape(-1, 3)


def volume_out(src, shape, origin, spacing, dtype=np.float32):
    """sdfhip_scene_volume: src = (structs, values) -> the (nz, ny, nx) array of the placement's value at the identity"""
    p = lattice_points(shape, origin, spacing)
    with np.errstate(all="ignore"):
        qc = [np.fmin(np.fmax(p[:, k], f32(0)), f32(1)) for k in range(3)]
        e = [p[:, k] - qc[k] for k in range(3)]
        D = qr.sample(src[0], src[1], np.stack(qc, 1))["distance"].astype(f32)
        out = D + np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    assert out.dtype == f32
    return out.astype(dtype).reshape(shape)            # (float32 -> float16: round to nearest even, as __float2half_rn)

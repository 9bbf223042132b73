"""CPU restatement of sdfhip_scene_place (include/sdfhip.h), numpy, float32 throughout, every operation an
array operation of its own in the order the header writes it.  The source's distance D is query_restatement.sample's (find from the
root + interpol_world: the shader's arithmetic), the bytes and the corner table are trimesh_restatement's from_float and CORNER, and
the construct rule is the one trimesh_restatement.build runs: the contracts cannot drift.  Every distinct point of a level is
evaluated once (np.unique, as trimesh_restatement.node_values does): a point's value depends on the point alone.

tests/test_place.py holds this file to things it did not come from (conventions, the closed form of a placed sphere, the
structure of the result); tests/test_gpu_place.py holds the GPU to this file, byte for byte."""
import numpy as np

import query_restatement as qr
from edit_restatement import tree_depth
from trimesh_restatement import CORNER, from_float

f32 = np.float32
IDENTITY = np.eye(3, dtype=np.float32)


def as_placement(rotation, scale, translation):
    """(R (3, 3), s, t (3,)) as float32: what the C record holds"""
    return np.asarray(rotation, dtype=f32).reshape(3, 3), f32(scale), np.asarray(translation, dtype=f32).reshape(3)


def inverse_map(p, R, s, t):
    """the source point q (three float32 arrays) of destination points p (n, 3): d = p - t, inv = 1 / s,
    q_a = ((R[0][a] d_0 + R[1][a] d_1) + R[2][a] d_2) * inv"""
    R, s, t = as_placement(R, s, t)
    p = np.asarray(p, dtype=f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        d = [p[:, k] - t[k] for k in range(3)]
        inv = f32(1.0) / s
        return [((R[0, a] * d[0] + R[1, a] * d[1]) + R[2, a] * d[2]) * inv for a in range(3)]


def value(src, p, R, s, t):
    """value(p) of the rule for points p (n, 3): (D(qc) + |q - qc|) * s, qc = q clamped to the source's cube"""
    R, s, t = as_placement(R, s, t)
    q = inverse_map(p, R, s, t)
    with np.errstate(all="ignore"):
        qc = [np.fmin(np.fmax(x, f32(0)), f32(1)) for x in q]            # (fmaxf / fminf: a NaN coordinate becomes 0)
        e = [x - c for x, c in zip(q, qc)]
        D = qr.sample(src[0], src[1], np.stack(qc, 1))["distance"].astype(f32)
        out = (D + np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])) * s
    assert out.dtype == f32
    return out


def node_values(src, coords, depth, R, s, t):
    """corner values (n, 8) and centre values (n,) of the nodes with integer coordinates coords (n, 3) at `depth`"""
    S = f32(2.0 ** -depth)
    coords = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    pts = np.concatenate([(2 * (coords[:, None, :] + CORNER[None])).reshape(-1, 3), 2 * coords + 1])     # in units of S / 2
    uniq, inv = np.unique(pts, axis=0, return_inverse=True)
    v = value(src, uniq.astype(f32) * f32(S * f32(0.5)), R, s, t)[inv.reshape(-1)]
    n = len(coords)
    return v[:8 * n].reshape(n, 8), v[8 * n:]


def place(src, rotation, scale, translation, depth=-1, want_counts=False):
    """src: (structs, values) -> (structs, values) of the placed tree (new arrays), breadth first.  depth: -1 = the source's, else
    0..12.  want_counts: also {"depth_out", "levels", "samples"}; samples = 9 for the root + 35 for every block of eight siblings
    (the 27 corners of its 3 x 3 x 3 lattice and its 8 centres), the look-ups the header counts."""
    SS = np.ascontiguousarray(src[0], dtype=np.int32).reshape(-1, 2)
    SV = np.ascontiguousarray(src[1], dtype=np.uint8).reshape(-1, 8)
    R, s, t = as_placement(rotation, scale, translation)
    max_depth = tree_depth(SS) if depth < 0 else int(depth)
    coords = np.zeros((1, 3), dtype=np.int64)
    parent = np.full(1, -1, dtype=np.int64)
    S_out, V_out = [], []
    start, d, samples = 0, 0, 0
    while True:
        S = f32(2.0 ** -d)
        n = len(coords)
        samples += 9 if d == 0 else 35 * (n // 8)
        cv, mv = node_values((SS, SV), coords, d, R, s, t)
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

"""CPU restatement of sdfhip_scene_slice (include/sdfhip.h), numpy, float32 throughout, built on the mesh's
restatement: the triangles are mesh_restatement.mesh(...)[..., :3], and EVERY triangle is tested against EVERY layer -- no height
range, no candidate layers, no reject -- so the tests hold the GPU's shortcuts to the rule.

tests/test_slice.py holds this file to things it did not make (pinned counts, closed contours, orientation, a float64 route written
another way); tests/test_gpu_slice.py holds the GPU to this file, byte for byte."""
import numpy as np

import mesh_restatement as mr

f32 = np.float32
SEGMENT = np.dtype([("a", "<f4", 3), ("layer", "<u4"), ("b", "<f4", 3), ("node", "<u4")])          # sdfhip_segment, 32 bytes
assert SEGMENT.itemsize == 32


def heights(offset, pitch, layers):
    """h_k = offset + (float)k * pitch, k = 0 .. layers - 1: the product rounded, then the sum"""
    k = np.arange(int(layers), dtype=f32)
    return (f32(offset) + (k * f32(pitch)).astype(f32)).astype(f32)


def vertex_heights(P, normal):
    """d = ((nx * px) + (ny * py)) + (nz * pz) of positions (..., 3), the normal as given"""
    n = np.asarray(normal, dtype=f32)
    P = np.asarray(P, dtype=f32)
    return (((n[0] * P[..., 0]).astype(f32) + (n[1] * P[..., 1]).astype(f32)).astype(f32) + (n[2] * P[..., 2]).astype(f32)).astype(f32)


def _point(a, b, da, db, h):
    """on the edge from its below end a to its above end b (da < h <= db)"""
    sa, sb = (da - h).astype(f32), (db - h).astype(f32)
    t = (sa / (sa - sb).astype(f32)).astype(f32)
    return (a + ((b - a).astype(f32) * t[:, None]).astype(f32)).astype(f32)


def slice_triangles(P, normal, offset, pitch, layers, nodes=None, budget=1 << 22):
    """The records of the triangles P (T, 3, 3) float32 against the planes, in the order triangle, then layer ascending.  nodes: each
    triangle's node index (zeros when not given).  budget: triangle x layer pairs tested at once."""
    P = np.ascontiguousarray(P, dtype=f32).reshape(-1, 3, 3)
    T = len(P)
    node = np.zeros(T, dtype=np.uint32) if nodes is None else np.asarray(nodes).astype(np.uint32)
    h = heights(offset, pitch, layers)
    d = vertex_heights(P, normal)                                            # (T, 3)
    parts = []
    step = max(1, budget // max(1, len(h)))
    for t0 in range(0, T, step):
        t1 = min(T, t0 + step)
        above = d[t0:t1, None, :] >= h[None, :, None]                        # (t, L, 3)
        ti, k = np.nonzero(above.any(2) & ~above.all(2))                     # row-major: triangle, then layer
        if not len(ti):
            continue
        A = above[ti, k]                                                     # (m, 3)
        nxt = np.roll(A, -1, axis=1)                                         # the side of each edge's far end (edges 0->1, 1->2, 2->0)
        down, up = A & ~nxt, ~A & nxt
        assert (down.sum(1) == 1).all() and (up.sum(1) == 1).all()
        ed, eu = down.argmax(1), up.argmax(1)
        tri, dd, hk = P[t0:t1][ti], d[t0:t1][ti], h[k]
        r = np.arange(len(ti))
        # the above -> below edge runs from vertex ed (above) to ed + 1 (below); the below -> above edge from eu (below) to eu + 1 (above)
        ed1, eu1 = (ed + 1) % 3, (eu + 1) % 3
        rec = np.zeros(len(ti), dtype=SEGMENT)
        rec["a"] = _point(tri[r, ed1], tri[r, ed], dd[r, ed1], dd[r, ed], hk)
        rec["b"] = _point(tri[r, eu], tri[r, eu1], dd[r, eu], dd[r, eu1], hk)
        rec["layer"] = k
        rec["node"] = node[t0:t1][ti]
        parts.append(rec)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=SEGMENT)


def slice_scene(structs, values, normal=(0.0, 0.0, 1.0), offset=0.5, pitch=0.0, layers=1, level=-1, meshed=None):
    """sdfhip_scene_slice in the device form's order (node, tetrahedron, triangle, layer): (records, layer_counts, (cells, cells_cut,
    cells_crossed)).  meshed: mesh_restatement.mesh(structs, values, level, want_cells=True), when the caller has it already."""
    tris, nodes, (cells, cut) = meshed if meshed is not None else mr.mesh(structs, values, level, want_cells=True)
    rec = slice_triangles(tris[:, :, :3], normal, offset, pitch, layers, nodes)
    counts = np.bincount(rec["layer"], minlength=int(layers)).astype(np.uint32)
    return rec, counts, (cells, cut, len(np.unique(rec["node"])))


def by_layer(rec, layers):
    """the host form's order: a stable sort on `layer` (node-major within a layer), and the layers + 1 offsets"""
    order = np.argsort(rec["layer"], kind="stable")
    starts = np.concatenate([[0], np.cumsum(np.bincount(rec["layer"], minlength=int(layers)))]).astype(np.int64)
    return rec[order], starts


def balance(rec):
    """points, keyed by their three words, that are the `a` of more or fewer records than they are the `b`"""
    if not len(rec):
        return 0
    pts = np.concatenate([rec["a"], rec["b"]]).view(np.uint32).reshape(-1, 3)
    _, key = np.unique(pts, axis=0, return_inverse=True)
    key = key.reshape(-1)
    m = len(rec)
    net = np.bincount(key[:m], minlength=key.max() + 1) - np.bincount(key[m:], minlength=key.max() + 1)
    return int((net != 0).sum())


def zero_length(rec):
    return int((rec["a"].view(np.uint32) == rec["b"].view(np.uint32)).all(1).sum())

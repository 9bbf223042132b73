"""Host-side helpers for Scene.Slice's records (sdfhip_scene_slice): a basis of the cutting planes, the
signed area of each layer's contours and the chaining of one layer's segments into closed polylines.  numpy only; nothing here
touches the library."""
import numpy as np

# sdfhip_segment, 32 bytes: the solid lies on the left of a -> b, seen from the tip of the normal
SEGMENT = np.dtype([("a", "<f4", 3), ("layer", "<u4"), ("b", "<f4", 3), ("node", "<u4")])


def slice_basis(normal):
    """(u, v): float64 unit vectors with (u, v, normal / |normal|) right-handed.  u is the coordinate axis the normal is least
    aligned with (the first of equals), made perpendicular to the normal; v = normal x u.  (0, 0, 1) gives u = x and v = y."""
    n = np.asarray(normal, dtype=np.float64).reshape(3)
    length = np.linalg.norm(n)
    if not np.isfinite(length) or length == 0.0:
        raise ValueError("slice_basis: the normal must be finite and not zero")
    n = n / length
    axis = np.zeros(3)
    axis[int(np.argmin(np.abs(n)))] = 1.0
    u = axis - (axis @ n) * n
    u /= np.linalg.norm(u)
    return u, np.cross(n, u)


def slice_areas(segments, layer_starts, normal):
    """The signed area each layer's contours enclose, float64: 0.5 * sum((a.u)(b.v) - (b.u)(a.v)) over the layer's records with
    (u, v) = slice_basis(normal).  Positive for a solid region (outer loops counter-clockwise, holes clockwise, so holes subtract).
    It is the area in the plane itself, whatever the normal's length; nothing is divided by |normal|."""
    u, v = slice_basis(normal)
    a, b = segments["a"].astype(np.float64), segments["b"].astype(np.float64)
    term = (a @ u) * (b @ v) - (b @ u) * (a @ v)
    starts = np.asarray(layer_starts, dtype=np.int64)
    return np.array([0.5 * term[starts[k]:starts[k + 1]].sum() for k in range(len(starts) - 1)], dtype=np.float64)


def slice_loops(segments_of_one_layer):
    """One layer's records as closed polylines: zero-length records are dropped, the rest are chained a -> b -> the record that starts
    where this one ends, points keyed by their three words.  Returns a list of (m + 1, 3) float32 arrays, first point == last point.
    Where several records start at one point (contours that touch) the lowest unused one is taken.  Raises ValueError when a chain
    cannot be closed -- where cells of different depth meet in a T-junction the contour of a layer may be open."""
    seg = np.asarray(segments_of_one_layer)
    a, b = np.ascontiguousarray(seg["a"], dtype=np.float32), np.ascontiguousarray(seg["b"], dtype=np.float32)
    keep = ~(a.view(np.uint32) == b.view(np.uint32)).all(1)
    a, b = a[keep], b[keep]
    m = len(a)
    if not m:
        return []
    _, key = np.unique(np.concatenate([a, b]).view(np.uint32).reshape(-1, 3), axis=0, return_inverse=True)
    key = key.reshape(-1)
    ka, kb = key[:m], key[m:]
    order = np.argsort(ka, kind="stable")                 # records by their start point, ascending index within a point
    first = np.searchsorted(ka[order], np.arange(key.max() + 2))
    taken = np.zeros(m, dtype=bool)
    cursor = first[:-1].copy()                            # per point: the next record starting there that may be unused
    loops = []
    for s in range(m):
        if taken[s]:
            continue
        chain, cur = [s], s
        taken[s] = True
        while kb[cur] != ka[s]:
            p = kb[cur]
            while cursor[p] < first[p + 1] and taken[order[cursor[p]]]:
                cursor[p] += 1
            if cursor[p] == first[p + 1]:
                raise ValueError("slice_loops: an open chain (no unused record starts where record %d ends)" % cur)
            cur = int(order[cursor[p]])
            taken[cur] = True
            chain.append(cur)
        loops.append(np.concatenate([a[chain], a[chain[:1]]]))
    return loops

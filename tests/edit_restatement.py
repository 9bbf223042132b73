"""CPU restatement of sdfhip_scene_edit (include/sdfhip.h), numpy, float32 throughout, vectorised by
level.  It visits EVERY node of every level -- the GPU's cull (a node and its subtree skipped where the brush cannot reach) is not
restated, so the tests hold the GPU to the rule, not to its shortcut.  `region=True` is the one exception, for trees too large to
walk whole in a test: an original node whose box lies more than 2 S outside the brush's bounding box is skipped with its subtree
(there s(centre) >= 2.5 S, beyond the GPU's cull of either op, so the result is the same)."""
import numpy as np

F = np.float32
EDIT_CARVE, EDIT_ADD = 0, 1
BRUSH_SPHERE, BRUSH_BOX = 0, 1
HALF = F(0.5)

# corner k and child i: (k & 1, k >> 1 & 1, k >> 2 & 1)
BITS = np.array([[k & 1, (k >> 1) & 1, (k >> 2) & 1] for k in range(8)], dtype=np.int64)
# t of child i's corner k along each axis: ((i >> a & 1) + (k >> a & 1)) * 0.5, shape (8 children, 8 corners, 3)
CHILD_T = ((BITS[:, None, :] + BITS[None, :, :]).astype(F) * HALF).astype(F)


def brush_distance(brush, params, px, py, pz):
    p = [F(v) for v in params]
    dx, dy, dz = px - p[0], py - p[1], pz - p[2]
    if brush == BRUSH_SPHERE:
        return np.sqrt((dx * dx + dy * dy) + dz * dz) - p[3]
    qx, qy, qz = np.abs(dx) - p[3], np.abs(dy) - p[4], np.abs(dz) - p[5]
    ox, oy, oz = np.maximum(qx, F(0)), np.maximum(qy, F(0)), np.maximum(qz, F(0))
    return np.sqrt((ox * ox + oy * oy) + oz * oz) + np.minimum(np.maximum(qx, np.maximum(qy, qz)), F(0))


def quantise(f, S):
    """SdfGen's FromFloat (dllmain.cpp:192-196): floorf(saturate(f/2/S + 0.25f) * 255)"""
    normd = (f / F(2)) / S
    sat = np.minimum(np.maximum(normd + F(0.25), F(0)), F(1))
    return np.floor(sat * F(255)).astype(np.uint8)


def decode(b, S):
    """o_sample_at's formula: ((b / 255.0f) - 0.25f) * S * 2.0f"""
    return ((b.astype(F) / F(255)) - F(0.25)) * S * F(2)


def lerp(a, b, t):
    return a + (b - a) * t


def trilerp(c, tx, ty, tz):
    """c[..., x + 2y + 4z]: along x, then y, then z"""
    e00, e10 = lerp(c[..., 0], c[..., 1], tx), lerp(c[..., 2], c[..., 3], tx)
    e01, e11 = lerp(c[..., 4], c[..., 5], tx), lerp(c[..., 6], c[..., 7], tx)
    return lerp(lerp(e00, e10, ty), lerp(e01, e11, ty), tz)


def tree_depth(structs):
    level, d = np.zeros(1, dtype=np.int64), 0
    while True:
        kids = structs[level, 1]
        kids = kids[kids >= 0].astype(np.int64)
        if not len(kids):
            return d
        level = (kids[:, None] + np.arange(8)).reshape(-1)
        d += 1


def brush_box(brush, params):
    c = np.array(params[:3], dtype=np.float64)
    h = np.array([params[3]] * 3 if brush == BRUSH_SPHERE else params[3:6], dtype=np.float64)
    return c - h, c + h


def edit_one(structs, values, op, brush, params, max_depth, region=False):
    """One brush: -> (structs, values) of the result (new arrays; the inputs are not modified)."""
    carve = op == EDIT_CARVE
    Sarr, V = structs.copy(), values.copy()
    n_total = len(Sarr)
    lo, hi = brush_box(brush, params)
    idx = np.zeros(1, dtype=np.int64)
    cell = np.zeros((1, 3), dtype=np.int64)
    new = np.zeros(1, dtype=bool)
    pre_new = np.zeros((0, 8), dtype=F)                    # pre-edit values of the level's new nodes, in their order
    d = 0
    while len(idx):
        S = F(2.0 ** -d)
        if region:                                         # (original nodes only; see the module's docstring)
            Ld = cell.astype(np.float64) * float(S)
            far = ((Ld > hi + 2 * float(S)) | (Ld + float(S) < lo - 2 * float(S))).any(1) & ~new
            keep = ~far
            idx, cell, new = idx[keep], cell[keep], new[keep]
        L = cell.astype(F) * S
        n = len(idx)
        orig = ~new
        pre = np.empty((n, 8), dtype=F)
        p = np.empty((n, 8), dtype=np.uint8)
        if orig.any():
            b = V[idx[orig]]
            p[orig] = b
            pre[orig] = decode(b, S)
        if new.any():
            pre[new] = pre_new
            p[new] = quantise(pre_new, S)
        corners = L[:, None, :] + BITS[None, :, :].astype(F) * S
        s = brush_distance(brush, params, corners[..., 0], corners[..., 1], corners[..., 2])
        qg = quantise(-s if carve else s, S)
        V[idx] = np.maximum(p, qg) if carve else np.minimum(p, qg)
        centre = L + HALF * S
        sc = brush_distance(brush, params, centre[:, 0], centre[:, 1], centre[:, 2])
        vc = trilerp(pre, HALF, HALF, HALF)
        leaf = Sarr[idx, 1] < 0
        wins = (-sc > vc) if carve else (sc < vc)
        split = leaf & (d < max_depth) & (np.abs(sc) < F(2) * S) & wins
        inner = ~leaf
        # the next level's original nodes: children of internal nodes
        kids = Sarr[idx[inner], 1].astype(np.int64)
        nidx = (kids[:, None] + np.arange(8)).reshape(-1)
        ncell = (2 * cell[inner][:, None, :] + BITS[None]).reshape(-1, 3)
        # the splits, in the order of their indices -> blocks appended
        order = np.argsort(idx[split], kind="stable")
        sp_idx, sp_cell, sp_pre = idx[split][order], cell[split][order], pre[split][order]
        m = len(sp_idx)
        if m:
            base = n_total
            Sarr[sp_idx, 1] = base + 8 * np.arange(m)
            blk = np.empty((8 * m, 2), dtype=np.int32)
            blk[:, 0] = np.repeat(sp_idx, 8)
            blk[:, 1] = -1
            Sarr = np.concatenate([Sarr, blk])
            V = np.concatenate([V, np.zeros((8 * m, 8), dtype=np.uint8)])
            n_total += 8 * m
            c = sp_pre[:, None, None, :]
            pre_new = trilerp(c, CHILD_T[None, :, :, 0], CHILD_T[None, :, :, 1], CHILD_T[None, :, :, 2]).reshape(-1, 8).astype(F)
            nidx = np.concatenate([nidx, base + np.arange(8 * m)])
            ncell = np.concatenate([ncell, (2 * sp_cell[:, None, :] + BITS[None]).reshape(-1, 3)])
            nnew = np.concatenate([np.zeros(len(kids) * 8, dtype=bool), np.ones(8 * m, dtype=bool)])
        else:
            pre_new = np.zeros((0, 8), dtype=F)
            nnew = np.zeros(len(nidx), dtype=bool)
        idx, cell, new = nidx, ncell, nnew
        d += 1
    return Sarr, V


def edit(structs, values, edits, max_depth=-1, region=False):
    """edits: [(op, brush, params)], applied in order; max_depth -1 = the input's depth."""
    structs = np.ascontiguousarray(structs, dtype=np.int32).reshape(-1, 2)
    values = np.ascontiguousarray(values, dtype=np.uint8).reshape(-1, 8)
    maxd = tree_depth(structs) if max_depth < 0 else max_depth
    for op, brush, params in edits:
        structs, values = edit_one(structs, values, op, brush, params, maxd, region)
    return structs, values


def deepest_leaf_centres(structs):
    """(centres (n, 3) float64, scale) of the leaves of the tree's deepest level: points on or next to the surface"""
    level, cell, d = np.zeros(1, dtype=np.int64), np.zeros((1, 3), dtype=np.int64), 0
    while True:
        kids = structs[level, 1].astype(np.int64)
        inner = kids >= 0
        if not inner.any():
            return (cell + 0.5) * 2.0 ** -d, 2.0 ** -d
        level = (kids[inner][:, None] + np.arange(8)).reshape(-1)
        cell = (2 * cell[inner][:, None, :] + BITS[None]).reshape(-1, 3)
        d += 1


def surface_point_under(structs, position, heading_rows):
    """A deepest-level leaf centre near the camera's central ray (direction = the third column of the Info heading rows): among
    those within two leaf scales of the ray, the nearest to the camera"""
    c, scale = deepest_leaf_centres(structs)
    pos = np.asarray(position, dtype=np.float64)
    h = np.asarray(heading_rows, dtype=np.float64)
    ray = np.array([h[0][2], h[1][2], h[2][2]])
    ray /= np.linalg.norm(ray)
    rel = c - pos
    t = rel @ ray
    off = np.linalg.norm(rel - t[:, None] * ray, axis=1)
    near = np.nonzero((off < 2 * scale) & (t > 0))[0]
    if not len(near):
        near = np.argsort(off)[:1]
    return tuple(float(v) for v in c[near[np.argmin(t[near])]])

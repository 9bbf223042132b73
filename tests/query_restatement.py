"""The three queries of include/sdfhip.h (sdfhip_scene_sample / _raycast / _pick) restated in numpy on top of
py_restatement_vec.ShaderV: its find, interpol_world, gradient, ray, fma, dot and normalize are the contract's arithmetic already,
vectorised under lane masks, and tests/test_oracle.py holds them to the C oracle.  What is added here is only what the header pins
for a query: which lanes are refused (SDFHIP_QUERY_INVALID), the loop of Compute.hlsl:194-203 with a caller's margin, limit and
step count, the fp32 sum t, and the status a lane ends with.

tests/test_query.py holds this file to the frozen oracle (distance_at, the golden frames); tests/test_gpu_query.py holds the GPU to
this file, bit for bit."""
import numpy as np

from py_restatement_vec import ShaderV, dot, fma, normalize

f32 = np.float32
HIT, ESCAPED, EXHAUSTED, INVALID = 0, 1, 2, 3

# the C records (include/sdfhip.h), field for field
PROBE = np.dtype({"names": ["distance", "node", "scale", "status", "gradient", "pad_"],
                  "formats": ["<f4", "<u4", "<f4", "<u4", ("<f4", (3,)), "<u4"], "offsets": [0, 4, 8, 12, 16, 28], "itemsize": 32})
HIT_REC = np.dtype({"names": ["position", "t", "normal", "prox", "status", "steps", "node", "scale"],
                    "formats": [("<f4", (3,)), "<f4", ("<f4", (3,)), "<f4", "<u4", "<u4", "<u4", "<f4"],
                    "offsets": [0, 12, 16, 28, 32, 36, 40, 44], "itemsize": 48})


def _shader(structs, values, info=None, lanes=0):
    sh = ShaderV(structs, values, bytes(info) if info is not None else bytes(112))
    _cursor_at_root(sh, lanes)
    return sh


def _cursor_at_root(sh, n):
    sh.index = np.zeros(n, np.int64)
    sh.lower = [np.zeros(n, f32) for _ in range(3)]
    sh.scale = np.ones(n, f32)
    sh.nodes = np.zeros(n, np.int64)
    sh.samples = np.zeros(n, np.int64)


def _finite(v):
    return np.isfinite(v[0]) & np.isfinite(v[1]) & np.isfinite(v[2])


def sample(structs, values, points):
    """sdfhip_scene_sample: every point looked up from the root."""
    p = np.asarray(points, f32).reshape(-1, 3)
    n = len(p)
    out = np.zeros(n, PROBE)
    if n == 0:
        return out
    pos = [p[:, k].copy() for k in range(3)]
    ok = _finite(pos)
    sh = _shader(structs, values, lanes=n)
    with np.errstate(all="ignore"):
        sh.find(pos, ok)
        d = sh.interpol_world(pos, ok)
        g = sh.gradient(pos)
    out["distance"] = np.where(ok, d, f32(0))
    out["node"] = np.where(ok, sh.index, 0)
    out["scale"] = np.where(ok, sh.scale, f32(0))
    out["status"] = np.where(ok, HIT, INVALID)
    for k in range(3):
        out["gradient"][:, k] = np.where(ok, g[k], f32(0))
    return out


def _march(sh, pos, d, margin, limit, max_steps):
    """The loop of Compute.hlsl:194-203 for the lanes of pos / d (lists of three float32 arrays).  Lanes that have left the loop are
    taken out of the arrays now and then (every operation is per lane: the bytes do not depend on it) -- a frame's longest pixels
    take 100 steps, most take a dozen."""
    n = len(pos[0])
    out = np.zeros(n, HIT_REC)
    valid = _finite(pos) & _finite(d) & ~((d[0] == 0) & (d[1] == 0) & (d[2] == 0))
    m2 = f32(f32(margin) * f32(2))
    limit = f32(limit)
    # the state of the lanes still in the arrays; `lane` = where each came from
    lane = np.nonzero(valid)[0]
    pos = [a[lane] for a in pos]
    d = [a[lane] for a in d]
    k = len(lane)
    _cursor_at_root(sh, k)
    prox, t, i, esc = np.ones(k, f32), np.zeros(k, f32), np.zeros(k, np.int64), np.zeros(k, bool)
    fin = {"pos": [np.zeros(n, f32) for _ in range(3)], "prox": np.ones(n, f32), "t": np.zeros(n, f32), "i": np.zeros(n, np.int64),
           "esc": np.zeros(n, bool), "index": np.zeros(n, np.int64), "lower": [np.zeros(n, f32) for _ in range(3)], "scale": np.ones(n, f32)}

    def retire(which):
        """the lanes `which` (a mask over the current arrays) leave: their state goes to the result"""
        w = lane[which]
        for a in range(3):
            fin["pos"][a][w] = pos[a][which]
            fin["lower"][a][w] = sh.lower[a][which]
        fin["prox"][w] = prox[which]; fin["t"][w] = t[which]; fin["i"][w] = i[which]; fin["esc"][w] = esc[which]
        fin["index"][w] = sh.index[which]; fin["scale"][w] = sh.scale[which]

    run = np.ones(k, bool)
    with np.errstate(all="ignore"):
        while True:
            run = run & ((prox > m2) | (prox < 0)) & (i < max_steps)
            if run.any():
                e = run & (dot(pos, pos) > limit)
                esc |= e
                run = run & ~e
            if not run.any():
                retire(np.ones(len(lane), bool))
                break
            if run.sum() * 2 < len(run):
                retire(~run)
                lane = lane[run]
                pos = [a[run] for a in pos]; d = [a[run] for a in d]
                prox, t, i, esc = prox[run], t[run], i[run], esc[run]
                sh.index = sh.index[run]; sh.lower = [a[run] for a in sh.lower]; sh.scale = sh.scale[run]
                sh.nodes = sh.nodes[run]; sh.samples = sh.samples[run]
                run = np.ones(len(lane), bool)
            sh.find(pos, run)
            pr = sh.interpol_world(pos, run)
            prox = np.where(run, pr, prox)
            pos = [np.where(run, fma(di, prox, p), p) for p, di in zip(pos, d)]
            t = np.where(run, (t + prox).astype(f32), t)
            i += run
        # the end state of every lane, back in the caller's order
        sh.index, sh.lower, sh.scale = fin["index"], fin["lower"], fin["scale"]
        sh.nodes = np.zeros(n, np.int64); sh.samples = np.zeros(n, np.int64)
        prox = fin["prox"]
        status = np.where(fin["esc"], ESCAPED, np.where((prox > m2) | (prox < 0), EXHAUSTED, HIT))
        nrm = normalize(sh.gradient(fin["pos"]))
    shaded = valid & (status != ESCAPED)
    for a in range(3):
        out["position"][:, a] = np.where(valid, fin["pos"][a], f32(0))
        out["normal"][:, a] = np.where(shaded, nrm[a], f32(0))
    out["t"] = np.where(valid, fin["t"], f32(0))
    out["prox"] = np.where(valid, prox, f32(0))
    out["status"] = np.where(valid, status, INVALID)
    out["steps"] = np.where(valid, fin["i"], 0)
    out["node"] = np.where(valid, fin["index"], 0)
    out["scale"] = np.where(valid, fin["scale"], f32(0))
    return out


def raycast(structs, values, origins, dirs, margin, limit, max_steps=100):
    """sdfhip_scene_raycast: directions used as given."""
    o = np.asarray(origins, f32).reshape(-1, 3)
    d = np.asarray(dirs, f32).reshape(-1, 3)
    if len(o) == 0:
        return np.zeros(0, HIT_REC)
    sh = _shader(structs, values)
    return _march(sh, [o[:, k].copy() for k in range(3)], [d[:, k].copy() for k in range(3)], margin, limit, int(max_steps))


def pick(structs, values, info, pixels, max_steps=100):
    """sdfhip_scene_pick: from info's position along the shader's ray() for each pixel {x, y}, margin and limit info's."""
    px = np.asarray(pixels, np.int64).reshape(-1, 2)
    if len(px) == 0:
        return np.zeros(0, HIT_REC)
    sh = _shader(structs, values, info)
    with np.errstate(all="ignore"):
        d = sh.ray(px[:, 0], px[:, 1])
    pos = [np.full(len(px), p, f32) for p in sh.position]
    return _march(sh, pos, d, sh.margin, sh.limit, int(max_steps))


def camera_rays(structs, values, info, pixels):
    """(origins, dirs) (n, 3) float32 of the pixels' rays, for a raycast that must equal a pick"""
    px = np.asarray(pixels, np.int64).reshape(-1, 2)
    sh = _shader(structs, values, info)
    with np.errstate(all="ignore"):
        d = sh.ray(px[:, 0], px[:, 1])
    return np.tile(np.asarray(sh.position, f32), (len(px), 1)), np.stack(d, 1).astype(f32)


def records_differ(got, want):
    """names of the fields in which two record arrays differ (floats by bits, NaN == NaN), with the first differing element"""
    bad = []
    for name in want.dtype.names:
        if name.startswith("pad"):
            continue
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        if a.dtype.kind == "f":
            same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
        else:
            same = a == b
        if not same.all():
            w = np.nonzero(~same.reshape(len(a), -1).all(1))[0]
            bad.append((name, int(len(w)), int(w[0]), a[w[0]].tolist(), b[w[0]].tolist()))
    return bad

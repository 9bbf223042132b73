"""CPU restatement of the sdfhip_instances_* calls (include/sdfhip.h), numpy, float32 throughout, every
operation an array operation of its own in the order the header writes it.  F is compose_restatement.value, imported and not
rewritten; what is added here is what the header pins on top of it: the winner tracked beside the fold, the six-tap gradient G, the
march of sdfhip_scene_raycast with F in the place of find + interpol_world, and main() of Compute.hlsl with F and G in the places of
find + interpol_world and gradient().  The camera ray, fma, dot and normalize are the shader restatement's
(tests/py_restatement_vec.py).  The skip is NOT restated: every instance is evaluated at every point.  F depends on the point alone,
so lanes are evaluated only while they are in a loop and the winner of a march is looked up once, at the last point it evaluated.

tests/test_instances.py holds this file to things it did not come from; tests/test_gpu_instances.py holds the GPU to this file, bit
for bit, and tests/test_gpu_instances_zoo.py does on the tree zoo and at the calls' edges (a tie of signed zeros among them: the fold
is compose_restatement's fminf / fmaxf, which order -0 below +0 as the header pins it)."""
import numpy as np

import compose_restatement as cr
import place_restatement as plr
from py_restatement_vec import ShaderV, dot, fma, normalize
from query_restatement import ESCAPED, EXHAUSTED, HIT, INVALID

f32 = np.float32
H_DEFAULT = f32(2.0 ** -10)
SKIP_FLOOR = f32(-0.5625)

# the C records (include/sdfhip.h), field for field
PART_PROBE = np.dtype({"names": ["value", "instance", "status", "pad0_", "gradient", "pad1_"],
                       "formats": ["<f4", "<u4", "<u4", "<u4", ("<f4", (3,)), "<u4"], "offsets": [0, 4, 8, 12, 16, 28], "itemsize": 32})
PART_HIT = np.dtype({"names": ["position", "t", "normal", "prox", "status", "steps", "instance", "pad_"],
                     "formats": [("<f4", (3,)), "<f4", ("<f4", (3,)), "<f4", "<u4", "<u4", "<u4", "<u4"],
                     "offsets": [0, 12, 16, 28, 32, 36, 40, 44], "itemsize": 48})


class Folded(list):
    """Instances of a list so long that few distinct (source, placement) pairs repeat in it (compose_cases.limit_parts): u_k is
    evaluated once per distinct pair, and the value and the winner are folded over the whole list in list order -- the same floats
    in the same order of operations, so the same bits (tests/test_instances_zoo.py holds the route to the plain one)."""


def value(instances, p):
    """F(p): compose_restatement.value; of a Folded list, the fold that winner() runs"""
    return winner(instances, p)[1] if isinstance(instances, Folded) else cr.value(instances, p)


def _finite(v):
    return np.isfinite(v[0]) & np.isfinite(v[1]) & np.isfinite(v[2])


def winner(instances, p):
    """(w(p), v(p)) for points p (n, 3): w = 0; UNION w = k iff u_k < v before the fold, INTERSECT iff u_k > v, SUBTRACT iff -u_k > v"""
    p = np.asarray(p, f32).reshape(-1, 3)
    v, w = None, np.zeros(len(p), np.int64)
    seen = {} if isinstance(instances, Folded) else None
    with np.errstate(all="ignore"):
        for k, (src, (R, s, t), op) in enumerate(instances):
            if seen is None:
                u = plr.value(src, p, R, s, t)
            else:
                key = (src[0].ctypes.data, src[1].ctypes.data, R.tobytes(), s.tobytes(), t.tobytes())
                if key not in seen:
                    seen[key] = plr.value(src, p, R, s, t)
                u = seen[key]
            if v is None:
                v = u
            elif op == cr.COMBINE_UNION:
                w = np.where(u < v, k, w); v = cr.fminf(v, u)
            elif op == cr.COMBINE_INTERSECT:
                w = np.where(u > v, k, w); v = cr.fmaxf(v, u)
            else:
                nu = -u
                w = np.where(nu > v, k, w); v = cr.fmaxf(v, nu)
    return w, v


def gradient(instances, p, h=H_DEFAULT, trace=None):
    """G(p) for points p (n, 3) -> three float32 arrays: F(p + h e_a) - F(p - h e_a), the offsets added and subtracted as vectors.
    trace: a list that receives the (6 n, 3) taps"""
    p = np.asarray(p, f32).reshape(-1, 3)
    n = len(p)
    if n == 0:
        return [np.zeros(0, f32) for _ in range(3)]
    taps = []
    with np.errstate(all="ignore"):
        for a in range(3):
            off = np.zeros(3, f32)
            off[a] = f32(h)
            taps.append((p + off).astype(f32))
            taps.append((p - off).astype(f32))
        taps = np.concatenate(taps)
        if trace is not None:
            trace.append(taps)
        f = value(instances, taps).reshape(6, n)
        return [(f[0] - f[1]).astype(f32), (f[2] - f[3]).astype(f32), (f[4] - f[5]).astype(f32)]


def _gradient_where(instances, pos, mask, h, trace=None):
    """G at the lanes of `mask` of pos (three arrays), zeros elsewhere"""
    k = np.nonzero(mask)[0]
    g = gradient(instances, np.stack([a[k] for a in pos], 1), h, trace)
    out = [np.zeros(len(mask), f32) for _ in range(3)]
    for a in range(3):
        out[a][k] = g[a]
    return out


def _value_where(instances, pos, mask, trace):
    k = np.nonzero(mask)[0]
    p = np.stack([a[k] for a in pos], 1)
    if trace is not None:
        trace.append(p)
    return k, value(instances, p)


def sample(instances, points, h=H_DEFAULT):
    """sdfhip_instances_sample"""
    p = np.asarray(points, f32).reshape(-1, 3)
    out = np.zeros(len(p), PART_PROBE)
    ok = _finite([p[:, 0], p[:, 1], p[:, 2]])
    out["status"] = np.where(ok, HIT, INVALID)
    k = np.nonzero(ok)[0]
    if len(k):
        w, v = winner(instances, p[k])
        F = value(instances, p[k])
        assert np.array_equal(F.view(np.uint32), v.view(np.uint32)), "the winner's fold is not compose_restatement.value"
        g = gradient(instances, p[k], h)
        out["value"][k] = F
        out["instance"][k] = w
        for a in range(3):
            out["gradient"][k, a] = g[a]
    return out


def _march(instances, pos, d, margin, limit, max_steps, h, trace=None):
    n = len(pos[0])
    out = np.zeros(n, PART_HIT)
    valid = _finite(pos) & _finite(d) & ~((d[0] == 0) & (d[1] == 0) & (d[2] == 0))
    m2 = f32(f32(margin) * f32(2))
    limit = f32(limit)
    prox, t, i, esc = np.ones(n, f32), np.zeros(n, f32), np.zeros(n, np.int64), np.zeros(n, bool)
    last = [np.zeros(n, f32) for _ in range(3)]
    run = valid.copy()
    with np.errstate(all="ignore"):
        while True:
            run = run & ((prox > m2) | (prox < 0)) & (i < max_steps)
            if run.any():
                e = run & (dot(pos, pos) > limit)
                esc |= e
                run = run & ~e
            if not run.any():
                break
            k, pr = _value_where(instances, pos, run, trace)
            for a in range(3):
                last[a][k] = pos[a][k]
            prox[k] = pr
            pos = [np.where(run, fma(di, prox, p), p) for p, di in zip(pos, d)]
            t = np.where(run, (t + prox).astype(f32), t)
            i += run
        status = np.where(esc, ESCAPED, np.where((prox > m2) | (prox < 0), EXHAUSTED, HIT))
        shaded = valid & (status != ESCAPED)
        nrm = normalize(_gradient_where(instances, pos, shaded, h, trace))
        w = np.zeros(n, np.int64)
        stepped = valid & (i > 0)
        if stepped.any():
            k = np.nonzero(stepped)[0]
            w[k] = winner(instances, np.stack([a[k] for a in last], 1))[0]
    for a in range(3):
        out["position"][:, a] = np.where(valid, pos[a], f32(0))
        out["normal"][:, a] = np.where(shaded, nrm[a], f32(0))
    out["t"] = np.where(valid, t, f32(0))
    out["prox"] = np.where(valid, prox, f32(0))
    out["status"] = np.where(valid, status, INVALID)
    out["steps"] = np.where(valid, i, 0)
    out["instance"] = np.where(valid, w, 0)
    return out


def raycast(instances, origins, dirs, margin, limit, max_steps=100, h=H_DEFAULT, trace=None):
    """sdfhip_instances_raycast: directions used as given.  trace: a list that receives the (n, 3) points of every evaluation, G's taps included"""
    o = np.asarray(origins, f32).reshape(-1, 3)
    d = np.asarray(dirs, f32).reshape(-1, 3)
    if len(o) == 0:
        return np.zeros(0, PART_HIT)
    return _march(instances, [o[:, k].copy() for k in range(3)], [d[:, k].copy() for k in range(3)], margin, limit, int(max_steps), h, trace)


def _camera(info):
    return ShaderV(np.full((1, 2), -1), np.zeros((1, 8), np.uint8), bytes(info))


def camera_rays(info, pixels):
    """(origins, dirs) (n, 3) float32 of the pixels' rays: the shader restatement's ray()"""
    px = np.asarray(pixels, np.int64).reshape(-1, 2)
    sh = _camera(info)
    with np.errstate(all="ignore"):
        d = sh.ray(px[:, 0], px[:, 1])
    return np.tile(np.asarray(sh.position, f32), (len(px), 1)), np.stack(d, 1).astype(f32)


def pick(instances, info, pixels, max_steps=100, h=H_DEFAULT, trace=None):
    """sdfhip_instances_pick: from info's position along the shader's ray() for each pixel {x, y}, margin and limit info's"""
    px = np.asarray(pixels, np.int64).reshape(-1, 2)
    if len(px) == 0:
        return np.zeros(0, PART_HIT)
    sh = _camera(info)
    o, d = camera_rays(info, px)
    return _march(instances, [o[:, k].copy() for k in range(3)], [d[:, k].copy() for k in range(3)], sh.margin, sh.limit, int(max_steps), h, trace)


def frame(instances, info, width, height, max_steps=100, h=H_DEFAULT, trace=None):
    """sdfhip_instances_render: (height, width, 4) float32, row 0 at the top.  ShaderV._main line for line, with F for find +
    interpol_world, G for gradient() and max_steps for 100"""
    sh = _camera(info)
    ys, xs = np.mgrid[0:height, 0:width]
    cx, cy = xs.ravel().astype(np.int64), ys.ravel().astype(np.int64)
    N = len(cx)
    out = np.zeros((N, 4), f32)
    if N == 0:
        return out.reshape(height, width, 4)
    with np.errstate(all="ignore"):
        done = np.zeros(N, bool)
        pos = [np.full(N, p, f32) for p in sh.position]
        d = sh.ray(cx, cy)
        prox = np.ones(N, f32)
        m = f32(sh.margin)
        m2 = f32(m * f32(2))
        i = np.zeros(N, np.int64)
        run = ~done
        while True:
            run = run & ((prox > m2) | (prox < 0)) & (i < max_steps)
            if not run.any():
                break
            esc = run & (dot(pos, pos) > sh.limit)
            out[esc] = np.stack([np.full(N, 0.005, f32), np.full(N, 0.01, f32), np.full(N, 0.2, f32), i.astype(f32)], 1)[esc]
            done |= esc
            run = run & ~esc
            if not run.any():
                break
            k, pr = _value_where(instances, pos, run, trace)
            prox[k] = pr
            pos = [np.where(run, fma(di, prox, p), p) for p, di in zip(pos, d)]
            i += run
        live = ~done
        dl = normalize([(f32(l) - p).astype(f32) for l, p in zip(sh.light, pos)])
        d = [np.where(live, a, b) for a, b in zip(dl, d)]
        pos = [np.where(live, fma(di, np.full(N, m, f32), p), p) for p, di in zip(pos, d)]
        angle = dot(d, normalize(_gradient_where(instances, pos, live, h, trace)))
        back = live & (angle < 0)
        out[back] = np.stack([np.zeros(N, f32)] * 3 + [i.astype(f32)], 1)[back]
        done |= back
        diff = [(f32(l) - p).astype(f32) for l, p in zip(sh.light, pos)]
        dist = (np.sqrt(dot(diff, diff)) / f32(2)).astype(f32)
        kk = f32(f32(2.0 ** float(sh.strength)) - f32(1))
        j = np.zeros(N, np.int64)
        run = ~done
        while True:
            run = run & (j < 40) & (prox > -m)
            if not run.any():
                break
            lit = run & ((prox > dist) | (pos[0] < 0) | (pos[1] < 0) | (pos[2] < 0) | (pos[0] > 1) | (pos[1] > 1) | (pos[2] > 1))
            a = ((angle / (dist * dist).astype(f32)).astype(f32) * kk).astype(f32)
            out[lit] = np.stack([a, a, a, (i + j).astype(f32)], 1)[lit]
            done |= lit
            run = run & ~lit
            near = run & (prox < m)
            if near.any():
                brk = near & (dot(_gradient_where(instances, pos, near, h, trace), d) < 0)
                run = run & ~brk                       # break: falls through to the black write below
            if not run.any():
                break
            k, pr = _value_where(instances, pos, run, trace)
            prox[k] = pr
            pos = [np.where(run, fma(di, (prox + m).astype(f32), p), p) for p, di in zip(pos, d)]
            j += run
        rest = ~done
        out[rest] = np.stack([np.zeros(N, f32)] * 3 + [(i + j).astype(f32)], 1)[rest]
    return out.reshape(height, width, 4)


def bound(instance, p):
    """b_k(p) = (-0.5625 + e) * s of the header's skip and u_k(p), for the test of b_k <= u_k: e restated from place_restatement's
    inverse map"""
    src, (R, s, t), _ = instance
    p = np.asarray(p, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        q = plr.inverse_map(p, R, s, t)
        qc = [np.fmin(np.fmax(x, f32(0)), f32(1)) for x in q]
        e = [x - c for x, c in zip(q, qc)]
        b = ((SKIP_FLOOR + np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])) * s).astype(f32)
    return b, plr.value(src, p, R, s, t)

"""The restatement of the sdfhip_instances_* calls (tests/instances_restatement.py) held to things it did not come from -- the
placement's own restatement, a list with a repeated or a far instance, the closed form of two spheres, the bound the exact skip
leans on -- and what the bindings refuse before a handle exists.  No GPU: tests/test_gpu_instances.py holds the GPU to the
restatement, bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest

import compose_cases as cc
import compose_restatement as cr
import instances_cases as ic
import instances_restatement as ir
import place_restatement as plr
import query_restatement as qr
import tree_zoo as tz
from conftest import REPO

f32 = np.float32


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def same_records(got, want):
    return not qr.records_differ(got, want)


def all_answers(inst, name, trace=None):
    cam, (W, H), steps = ic.camera(name).State, ic.size(name), ic.max_steps(name)
    return (ir.sample(inst, ic.points(name)), ir.raycast(inst, *ic.rays(name), cam.margin, cam.limit, steps, trace=trace),
            ir.pick(inst, cam, ic.pixels(name), steps, trace=trace), ir.frame(inst, cam, W, H, steps, trace=trace))


def test_the_cases_are_what_they_are_for():
    assert len(ic.parts("many")) == 65 and len(ic.parts("eight")) == 8 and len({src for src, _, _ in ic.parts("eight")}) == 1
    assert [op for _, _, op in ic.parts("csg")] == [cr.COMBINE_UNION, cr.COMBINE_SUBTRACT, cr.COMBINE_INTERSECT]
    assert all(W % 8 and H % 8 for W, H in (ic.FRAME, ic.FRAME_LONG))
    assert np.linalg.det(ic.parts("one:sphere_d4:mirror")[0][1][0]) < 0
    # the statuses a batch must hold: hits, escapes, a ray that escapes before its first step, the refused elements in the middle
    hits = ic.restated("csg", "raycast")
    m = len(hits) // 2
    assert hits["status"][m] == qr.ESCAPED and hits["steps"][m] == 0 and hits["prox"][m] == 1
    assert (hits["status"][m + 1:m + 4] == qr.INVALID).all() and not hits["position"][m + 1:m + 4].any()
    assert {qr.HIT, qr.ESCAPED} <= set(hits["status"].tolist()) and (hits["status"][m + 4:] != qr.INVALID).all()
    probes = ic.restated("csg", "sample")
    n = len(probes)
    assert probes["status"][n // 2] == qr.INVALID and probes["status"][n // 2 + 3] == qr.INVALID and (probes["status"] == qr.HIT).sum() == n - 2
    assert set(probes["instance"].tolist()) == {0, 2}, "a difference never wins outside the solid it carves, an intersection does"
    # one step: nothing can have converged from a camera outside
    one = ic.restated("steps1", "pick")
    assert (one["steps"] == 1).all() and (one["status"] == qr.EXHAUSTED).all()
    # the camera inside the solid reads a negative value first and marches backwards
    inside = ic.restated("inside", "pick")
    cam = ic.camera("inside").State
    assert ir.value(ic.instances("inside"), np.asarray(cam.position, f32)[None])[0] < 0
    assert (inside["t"][inside["steps"] > 0] < 0).any()
    # every kind of pixel in a frame: sky, lit, black; alpha = steps
    frame = ic.restated("csg", "frame")
    sky = frame[..., 2] == f32(0.2)
    assert sky.any() and (~sky & (frame[..., 0] > 0)).any() and (~sky & (frame[..., 0] == 0)).any()
    assert frame.shape == (ic.FRAME[1], ic.FRAME[0], 4) and frame[..., 3].max() > 40
    # more winners than a wave has lanes cannot be seen from one camera, but many are
    assert len(set(ic.restated("many", "pick")["instance"].tolist())) > 8


def test_one_instance_is_the_placements_value():
    p = ic.points("csg")
    p = p[np.isfinite(p).all(1)]
    for name in ("one:sphere_d4:identity", "one:sphere_d4:generic_half", "one:sphere_d4:mirror", "one:nine:mirror"):
        (src, (R, s, t), op), = ic.instances(name)
        want = plr.value(src, p, R, s, t)
        assert same_bits(ir.value(ic.instances(name), p), want), name
        got = ir.sample(ic.instances(name), p)
        assert same_bits(got["value"], want) and not got["instance"].any(), name
    # under the identity, inside the cube, that is the source's own distance
    inside = p[((p >= 0) & (p <= 1)).all(1)]
    src = cc.tree("sphere_d4")
    assert same_bits(ir.value(ic.instances("one:sphere_d4:identity"), inside), qr.sample(*src, inside)["distance"])


def test_a_repeated_instance_changes_nothing():
    name = "one:sphere_d4:generic_half"
    once = ic.instances(name)
    twice = cr.as_instances(cc.with_trees(ic.parts(name) * 2))
    for a, b in zip(all_answers(twice, name)[:3], (ic.restated(name, w) for w in ("sample", "raycast", "pick"))):
        assert same_records(a, b) and not a["instance"].any(), "ties keep the earlier instance"
    assert same_bits(all_answers(twice, name)[3], ic.restated(name, "frame"))
    assert len(once) == 1 and len(twice) == 2


def test_a_far_instance_changes_nothing_and_never_wins():
    name = "csg"
    far = ("sphere_d4", (plr.IDENTITY, 1.0, (100.0, 0.0, 0.0)), cr.COMBINE_UNION)
    inst = cr.as_instances(cc.with_trees(ic.parts(name) + [far]))
    trace = []
    sample, rays, pick, frame = all_answers(inst, name, trace)
    for got, what in ((sample, "sample"), (rays, "raycast"), (pick, "pick")):
        assert same_records(got, ic.restated(name, what)), what
        assert (got["instance"] < 3).all(), what
    assert same_bits(frame, ic.restated(name, "frame"))
    # ... because at every point a march or a gradient visited -- the camera's limit keeps them within sqrt(limit) of the origin --
    # the far instance's value exceeds the fold of the others
    visited = np.concatenate(trace)
    cam = ic.camera(name).State
    assert len(visited) > 10000 and cam.limit < 4
    src, (R, s, t), _ = inst[-1]
    assert (plr.value(src, visited, R, s, t) > ir.value(inst[:-1], visited)).all()


def test_the_winner_inside_one_of_two_disjoint_spheres():
    inst = ic.instances("two_spheres")
    centres = [f32(0.5) * np.full(3, 0.5) + np.asarray(t, np.float64) for _, (_, _, t), _ in inst]
    radius = 0.5 * 0.3
    assert np.linalg.norm(centres[0] - centres[1]) > 2 * radius
    rng = np.random.default_rng(5)
    for k, c in enumerate(centres):
        d = rng.normal(size=(200, 3))
        p = (c + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0, 0.8 * radius, size=(200, 1))).astype(f32)
        got = ir.sample(inst, p)
        assert (got["instance"] == k).all() and (got["value"] < 0).all(), k
        # just outside the surface, where the bytes are not saturated, the part still wins and G points away from ITS centre: the
        # assembly's gradient there is the winning part's
        shell = (c + d / np.linalg.norm(d, axis=1, keepdims=True) * (radius + 0.01)).astype(f32)
        got = ir.sample(inst, shell)
        assert (got["instance"] == k).all() and (got["value"] > 0).all(), k
        g = got["gradient"].astype(np.float64)
        cos = (g * (shell - c)).sum(1) / (np.linalg.norm(g, axis=1) * np.linalg.norm(shell - c, axis=1))
        assert (cos > 0.9).all(), (k, cos.min())


def test_the_skips_bound_holds_wherever_the_cases_go():
    # b_k = (-0.5625 + e) * s <= u_k at every point the cases' restatements evaluate F -- the sample points, the marches of raycast,
    # pick and frame, the frames' shadow rays, and every tap of G -- for every instance of the list
    for name in ic.NAMES:
        inst = ic.instances(name)
        visited = ic.visited(name)
        assert len(visited) > 1000, name
        for k, one in enumerate(inst):
            b, u = ir.bound(one, visited)
            assert (b <= u).all(), (name, k)


def test_no_source_reads_below_the_skips_floor():
    # D >= -0.5625 on every zoo source (random bytes and hostile shapes included) and on the cases' sources: at random points, at
    # points on the lattice of the deepest level, and in the cube's corners
    rng = np.random.default_rng(11)
    p = np.concatenate([rng.uniform(0, 1, size=(4000, 3)), rng.integers(0, 4097, size=(2000, 3)) / 4096.0,
                        np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], float)]).astype(f32)
    sources = dict(tz.zoo())
    sources.update({name: cc.tree(name) for name in ("leaf", "nine", "sphere_d4", "torus_d6")})
    lowest = 0.0
    for name, (S, V) in sources.items():
        D = qr.sample(S, V, p)["distance"]
        assert (D >= ir.SKIP_FLOOR).all(), name
        lowest = min(lowest, float(D.min()))
    assert lowest >= -0.5 - 2.0 ** -20, lowest          # the decode's own floor: (0 - 0.25) * 2 * scale, scale <= 1
    # and the bytes alone: the least a texel decodes to is 0
    assert (np.arange(256, dtype=f32) / f32(255)).min() == 0


def test_hits_lie_on_the_closed_form_of_two_spheres():
    inst = ic.instances("two_spheres")
    cam = ic.camera("two_spheres").State
    W, H = ic.size("two_spheres")
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    hits = ir.pick(inst, cam, np.stack([xs.ravel(), ys.ravel()], 1), 100)
    hit = hits[hits["status"] == qr.HIT]
    assert len(hit) > 300 and set(hit["instance"].tolist()) == {0, 1}
    centres = np.array([0.5 * np.full(3, 0.5) + np.asarray(t, np.float64) for _, (_, _, t), _ in inst])
    s, radius = 0.5, 0.5 * 0.3
    pos = hit["position"].astype(np.float64)
    err = np.abs(np.linalg.norm(pos - centres[hit["instance"]], axis=1) - radius)
    # The tolerance: a HIT's last value lies in [0, 2 margin] and the step that follows moves the point by it, so the point is
    # within 2 margin of where the FIELD says the surface is; the field is the source's bytes -- quantum 2 S / 255 of its leaf level
    # S = 2^-4 -- interpolated over leaves of edge S, times the placement's scale.  The interpolation error of a sphere's distance
    # over such a leaf, in quanta, is not derived here: the restatement's own worst case is 10.14 quanta, 0.003286 in all (measured on the CPU, this
    # camera, every pixel of the frame; a chord of a sphere of radius 0.15 across a leaf of edge 1/32 sags by 0.0008 per axis); C is
    # 1.5 x that for the change of platform
    quantum = s * 2.0 * 2.0 ** -4 / 255.0
    measured = (err.max() - 2.0 * float(cam.margin)) / quantum
    print(f"worst |distance to the closed form| {err.max():.6f} = 2 margin + {measured:.2f} quanta of {quantum:.6f}")
    C = 1.5 * 10.14
    assert err.max() <= 2.0 * float(cam.margin) + C * quantum, (err.max(), measured)
    # the part under the cursor is the sphere the point lies on
    nearest = np.argmin(np.linalg.norm(pos[:, None, :] - centres[None], axis=2), axis=1)
    assert (nearest == hit["instance"]).all()


def test_the_python_layer_refuses_what_needs_no_handle(sb):
    cam = sb.Logic(16, 16)
    for call in (lambda parts: sb.Scene.SampleParts(parts, np.zeros((1, 3))), lambda parts: sb.Scene.RaycastParts(parts, np.zeros((1, 3)), np.ones((1, 3)), 0.001, 3.0),
                 lambda parts: sb.Scene.PickParts(parts, cam, [[0, 0]]), lambda parts: sb.Scene.DrawParts(parts, cam, 16, 16),
                 lambda parts: sb.Scene.SamplePartsDevice(parts, 0, 0, 0), lambda parts: sb.Scene.RaycastPartsDevice(parts, 0, 0, 0.001, 3.0, 0),
                 lambda parts: sb.Scene.DrawPartsDevice(parts, cam, 16, 16, 0)):
        for bad in ([], [7], [("not a scene", (np.eye(3), 1.0, (0, 0, 0)))], [(None, (np.eye(3), 1.0, (0, 0, 0)), 0, 0)]):
            with pytest.raises(ValueError):
                call(bad)
    with pytest.raises(ValueError):
        sb.Scene.RaycastParts([], np.zeros((2, 3)), np.ones((1, 3)), 0.001, 3.0)
    # a negative count or side is refused by the device forms as by the host forms, before it can wrap (no handle is read: the
    # part's scene is never uploaded)
    class Unloaded(sb.Scene):
        def __init__(self):
            self._h = None
    part = [(Unloaded(), (np.eye(3), 1.0, (0, 0, 0)))]
    for call in (lambda: sb.Scene.DrawParts(part, cam, -1, 16), lambda: sb.Scene.DrawPartsDevice(part, cam, -1, 16, 0),
                 lambda: sb.Scene.DrawPartsDevice(part, cam, 16, -1, 0), lambda: sb.Scene.SamplePartsDevice(part, 0, -1, 0),
                 lambda: sb.Scene.RaycastPartsDevice(part, 0, -1, 0.001, 3.0, 0)):
        with pytest.raises(ValueError):
            call()


def test_the_library_refuses_what_needs_no_handle(sb):
    L = sb._lib
    R, s, t = cc.ONE_PLACEMENTS["generic_half"]()
    # (a list is checked to its end before its first handle is read: the address of a zeroed block stands in for the handles)
    block = (ctypes.c_uint8 * 4096)()
    fake = ctypes.c_void_p(ctypes.addressof(block))
    good = lambda **kw: sb.Instance(**dict(dict(scene=fake, op=0, rotation=R.tolist(), scale=s, translation=t.tolist()), **kw))
    cam = sb.Logic(16, 16).State
    buf = (ctypes.c_float * 64)()

    def calls(arr, n, opt, info=cam, margin=0.001, width=2, height=2):
        o = ctypes.byref(opt) if opt is not None else None
        i = ctypes.byref(info) if info is not None else None
        return {"sample": lambda: L.lib.sdfhip_instances_sample(arr, n, o, buf, 1, buf),
                "sample_device": lambda: L.lib.sdfhip_instances_sample_device(arr, n, o, buf, 1, buf, None),
                "raycast": lambda: L.lib.sdfhip_instances_raycast(arr, n, o, buf, 1, margin, 3.0, buf),
                "raycast_device": lambda: L.lib.sdfhip_instances_raycast_device(arr, n, o, buf, 1, margin, 3.0, buf, None),
                "pick": lambda: L.lib.sdfhip_instances_pick(arr, n, o, i, buf, 1, buf),
                "render": lambda: L.lib.sdfhip_instances_render(arr, n, o, i, width, height, buf),
                "render_device": lambda: L.lib.sdfhip_instances_render_device(arr, n, o, i, width, height, buf, None)}

    def refused(word, items, n=None, opt=None, only=None, **kw):
        arr = (sb.Instance * max(1, len(items)))(*items) if items is not None else None
        for name, call in calls(arr, len(items or []) if n is None else n, opt, **kw).items():
            if only and name not in only:
                continue
            rc, msg = call(), L.lib.sdfhip_last_error()
            assert rc == L.ERR_ARG and word in msg and b"instances_" + name.encode() + b":" in msg, (name, word, msg)

    # whatever is refused below is refused before any handle is looked at
    refused(b"null instance list", None, n=1)
    for n in (0, 4097):
        refused(b"1..4096", [good()], n=n)
    five = lambda bad: [good(), good(op=2), good(), bad, good()]
    for bad, word in ((good(op=3), b"unknown op"), (good(op=-1), b"unknown op"),
                      (good(rotation=((1, 0, 0), (0, 1, 0), (0, 0, 1.001))), b"orthogonal"), (good(scale=0.0), b"scale"),
                      (good(scale=float("nan")), b"finite"), (good(translation=(0.0, float("inf"), 0.0)), b"finite")):
        refused(b"instance 3", five(bad))
        refused(word, five(bad))
    refused(b"instance 0", [good(op=1), good()])
    refused(b"instance 0: null scene", [good(scene=None)])
    refused(b"instance 3: null scene", five(good(scene=None)))
    refused(b"null info", [good()], info=None, only=("pick", "render", "render_device"))
    refused(b"finite", [good()], margin=float("nan"), only=("raycast", "raycast_device"))
    dark = sb.Logic(16, 16).State
    dark.limit = float("inf")
    refused(b"finite", [good()], info=dark, only=("pick", "render", "render_device"))
    refused(b"16384", [good()], width=16385, only=("render", "render_device"))
    refused(b"16384", [good()], height=16385, only=("render", "render_device"))
    small = sb.InstancesOptions()
    small.size = 8
    refused(b"bytes", [good()], opt=small)
    refused(b"flags", [good()], opt=sb.InstancesOptions(flags=2))
    refused(b"max_steps", [good()], opt=sb.InstancesOptions(max_steps=4097))
    for h in (float("nan"), float("inf"), -1.0):
        refused(b"normal_step", [good()], opt=sb.InstancesOptions(normal_step=h))

    class Newer(ctypes.Structure):
        _fields_ = sb.InstancesOptions._fields_ + [("unknown", ctypes.c_int32)]
    newer = Newer()
    newer.size, newer.unknown = 20, 3
    as_options = ctypes.cast(ctypes.pointer(newer), ctypes.POINTER(sb.InstancesOptions)).contents
    refused(b"", [good()], opt=as_options)                     # an unknown field that is set
    newer.unknown = -1
    refused(b"null scene", [good(scene=None)], opt=as_options) # ... and one that says "default": the call goes on to the list


def test_the_records_are_the_headers():
    import sdfbox_amd as sb
    text = open(os.path.join(REPO, "include", "sdfhip.h")).read()
    for c_name, cls, dtype, size in (("sdfhip_part_probe", sb.PartProbe, ir.PART_PROBE, 32), ("sdfhip_part_hit", sb.PartHit, ir.PART_HIT, 48),
                                     ("sdfhip_instances_options", sb.InstancesOptions, None, 16)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (c_name, c_name), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            words = decl.split()
            if not words:
                continue
            base, names = words[0], " ".join(words[1:]).split(",")
            for n in names:
                m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", n)
                fields.append((m.group(1), base, int(m.group(2) or 1)))
        assert ctypes.sizeof(cls) == size == sum(4 * k for _, _, k in fields), c_name
        assert [f[0] for f in cls._fields_] == [f[0] for f in fields], c_name
        off = 0
        for name, base, count in fields:
            assert getattr(cls, name).offset == off, (c_name, name)
            if dtype is not None:
                assert dtype.fields[name][1] == off and dtype.fields[name][0].base == np.dtype({"float": "<f4", "uint32_t": "<u4"}[base]), (c_name, name)
            off += 4 * count
        if dtype is not None:
            assert dtype.itemsize == size and np.dtype(cls).itemsize == size
    assert sb.INSTANCES_NO_SKIP == int(re.search(r"SDFHIP_INSTANCES_NO_SKIP\s*=\s*(\d+)", text).group(1))


def test_the_cpp_mirror_compiles_and_fails_loudly_without_a_gpu(tmp_path):
    # Program::DrawParts / PickParts / SampleParts (include/sdfbox.hpp) through tests/cpp_parts.cpp; with a GPU the bytes are
    # tests/test_gpu_instances.py's
    import shutil
    import subprocess
    import torch
    from conftest import GOLDEN
    exe, libdir = str(tmp_path / "cpp_parts"), os.path.join(REPO, "sdfbox_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "cpp_parts.cpp"),
                           "-o", exe, "-L", libdir, "-lsdfhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    shutil.copy(os.path.join(GOLDEN, "sphere_d4.asdf"), tmp_path / "sphere.asdf")
    ic.pixels("two_spheres").tofile(tmp_path / "pixels.bin")
    ic.points("two_spheres").tofile(tmp_path / "points.bin")
    W, H = ic.size("two_spheres")
    out = subprocess.run([exe, str(tmp_path / "sphere.asdf"), str(W), str(H), str(tmp_path / "pixels.bin"), str(tmp_path / "points.bin"),
                          str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    if torch.cuda.is_available():
        assert out.returncode == 0, out.stderr
    else:
        assert out.returncode == 3 and "sdfhip:" in out.stderr, (out.returncode, out.stderr)

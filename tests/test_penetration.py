"""The restatement of sdfhip_instances_penetration (tests/penetration_restatement.py) held to things it did not come from -- the clash
restatement's pairs and counts, distance_restatement's distance at the witness, the list reversed, the closed form of the lens of two
balls -- and what the bindings refuse before a handle exists.  No GPU: tests/test_gpu_penetration.py holds the GPU to the
restatement, byte for byte."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import clash_cases as ca
import clash_restatement as clr
import compose_cases as cc
import distance_restatement as dr
import penetration_cases as pc
import penetration_restatement as pr
import place_restatement as plr
from conftest import REPO

f32 = np.float32


@pytest.mark.parametrize("name, d, box", [("lens", 5, pc.UNIT), ("lens", 6, pc.UNIT), ("csg", 5, pc.UNIT), ("csg", pc.OFF_CUBE_DEPTH, pc.OFF_CUBE),
                                          ("chain64", 5, pc.UNIT), ("same64", 3, pc.UNIT), ("three_forms", 5, pc.UNIT), ("deepest", 5, pc.UNIT),
                                          ("eight", 5, pc.UNIT), ("one", 3, pc.UNIT)])
def test_the_pairs_and_their_points_are_the_clash_checks(name, d, box):
    rec, counts = pc.restated(name, d, box)
    want = ca.restated(name, d, box)
    assert len(rec) == len(want)
    for field in ("a", "b", "points"):
        assert np.array_equal(rec[field], want[field]), (name, field)
    # every shared point is in two parts at least: a pair's points are searched once for each of its two parts, or more
    assert counts["searches"] >= (2 * int(want["points"].max()) if len(want) else 0)
    assert (counts["searches"] == 0) == (len(want) == 0)


@pytest.mark.parametrize("name, d", [("lens", 5), ("csg", 5), ("three_forms", 5)])
def test_the_witness_is_what_the_distance_restatement_says(name, d):
    # ra, rb = |sdfhip_scene_distance's distance| at the inverse-mapped witness, times s; nearest = its nearest point mapped forward;
    # the witness is inside both parts, depth = fminf(ra, rb), and no shared point has a larger fminf(r_a, r_b)
    rec, _ = pc.restated(name, d)
    inst = pc.instances(name)
    p = clr.lattice(d)[0]
    inside = clr.contains(inst, p)
    assert len(rec) >= 1
    for r in rec:
        w = int(r["witness"])
        assert inside[r["a"], w] and inside[r["b"], w]
        assert r["depth"] == np.fmin(r["ra"], r["rb"]) and r["depth"] > 0
        for side in "ab":
            src, (R, s, t), _ = inst[r[side]]
            R, s, t = plr.as_placement(R, s, t)
            q = np.stack(plr.inverse_map(p[w:w + 1], R, s, t), 1)
            c = dr.distance(src[0], src[1], q, -1, surf=pr.surface_of(src))[0]
            assert c["status"] == dr.HIT and c["distance"] < 0                # (the clash rule put the point inside)
            assert (np.abs(c["distance"]) * s).view(np.uint32) == r["r" + side].view(np.uint32), (name, side)
            assert c["node"] == r["node_" + side]
            assert np.array_equal(pr.forward_map(c["nearest"][None], R, s, t)[0].view(np.uint32), r["nearest_" + side].view(np.uint32))
            # the nearest point is r away from the witness, as far as fp32 carries it through two maps
            assert abs(np.linalg.norm(r["nearest_" + side].astype(np.float64) - p[w]) - float(r["r" + side])) < 1e-5
    if name == "lens":
        # the maximum and its tie rule, from the definition, over all 60 points
        r = rec[0]
        both = np.nonzero(inside[0] & inside[1])[0]
        m = np.fmin(pr.searched(inst[0], p[both])[0], pr.searched(inst[1], p[both])[0])
        assert m.max() == r["depth"] and both[np.nonzero(m == m.max())[0][0]] == r["witness"] and (m[both < r["witness"]] < r["depth"]).all()


@pytest.mark.parametrize("name, d", [("lens", 5), ("three_forms", 5)])
def test_the_list_reversed_gives_the_records_mirrored(name, d):
    inst = pc.instances(name)
    K = len(inst)
    back = pr.penetration(inst[::-1], d)
    want = {(K - 1 - int(r["b"]), K - 1 - int(r["a"])): r for r in pc.restated(name, d)[0]}
    assert sorted(want) == [(int(r["a"]), int(r["b"])) for r in back]
    for r in back:
        w = want[(int(r["a"]), int(r["b"]))]
        for field, other in (("points", "points"), ("witness", "witness"), ("depth", "depth"), ("ra", "rb"), ("rb", "ra"), ("node_a", "node_b"),
                             ("node_b", "node_a"), ("nearest_a", "nearest_b"), ("nearest_b", "nearest_a")):
            assert r[field].tobytes() == w[other].tobytes(), (name, field)


def lens_geometry():
    """the two balls of "lens" as placed: their centres, and the eps of the restatement's own mesh -- eps_out = the largest excess of
    a placed mesh vertex's radius over 0.15, eps_in = 0.15 - sqrtf(d2) * s at the ball's centre -- the larger of the two balls' each"""
    inst = pc.instances("lens")
    centres, eps_out, eps_in = [], 0.0, 0.0
    for src, (R, s, t), _ in inst:
        R, s, t = plr.as_placement(R, s, t)
        c = pr.forward_map(np.full((1, 3), 0.5, f32), R, s, t)[0].astype(np.float64)
        surf = pr.surface_of(src)
        v = pr.forward_map(surf.pos.reshape(-1, 3), R, s, t).astype(np.float64)
        eps_out = max(eps_out, float((np.linalg.norm(v - c, axis=1) - 0.15).max()), 0.0)
        d2 = dr.nearest(surf, np.full((1, 3), 0.5, f32))[0]
        eps_in = max(eps_in, 0.15 - float(np.sqrt(d2)[0] * s))
        centres.append(c)
    return centres, eps_out, eps_in


def test_the_lens_of_two_balls_has_its_closed_form_depth():
    # Two balls of radius 0.15 whose centres are 0.2 apart: the largest ball inside both sits at the midpoint and has radius 0.05.
    # A part's mesh lies between the spheres of radius 0.15 - eps_in and 0.15 + eps_out round its centre, so at any point p inside
    # r_k(p) <= 0.15 + eps_out - |p - c_k| and r_k(p) >= 0.15 - eps_in - |p - c_k|.  max(|p - c_a|, |p - c_b|) >= 0.1 gives the upper bound;
    # a lattice point within pitch sqrt(3) / 2 of the midpoint, inside both, gives the lower one.
    # Measured: eps_out = 0.000393, eps_in = 0.011479; depth 0.036095 at lattice depth 5 (bounds 0.011458 .. 0.050393), 0.045509 at 6
    # (0.024990 .. 0.050393).
    (ca_, cb_), eps_out, eps_in = lens_geometry()
    assert abs(np.linalg.norm(cb_ - ca_) - 0.2) < 1e-6 and eps_out >= 0.0 and eps_in > 0.0
    mid = (ca_ + cb_) * 0.5
    got = {}
    for d in (5, 6):
        rec = pc.restated("lens", d)[0]
        pitch = float(clr.pitch_of(d))
        reach = pitch * np.sqrt(3.0) / 2.0
        p = clr.lattice(d)[0]
        near = np.nonzero(np.linalg.norm(p.astype(np.float64) - mid, axis=1) <= reach)[0]
        inside = clr.contains(pc.instances("lens"), p[near])
        assert len(near) >= 1 and (inside[0] & inside[1]).any(), d
        got[d] = float(rec["depth"][0])
        print(f"lens depth {d}: {got[d]:.6f} in [{0.05 - eps_in - reach:.6f}, {0.05 + eps_out:.6f}], eps_out {eps_out:.6f} eps_in {eps_in:.6f}")
        assert got[d] <= 0.05 + eps_out
        assert got[d] >= 0.05 - eps_in - reach
    assert got[5] < got[6]                       # the finer lattice comes nearer the midpoint


def test_the_push_of_the_lens_lies_along_the_axis_of_centres(sb):
    # The ideal nearest points are n_k* = c_k + 0.15 (p - c_k) / |p - c_k|.  The mesh's nearest point n_k lies in the shell above, rho in
    # [R_in, R_out] from c_k, and no further from p than R_out - u, u = |p - c_k|: the angle theta at c_k between n_k and p has
    # cos theta >= (rho^2 + u^2 - (R_out - u)^2) / (2 rho u).  |n_k - n_k*|^2 = rho^2 + 0.15^2 - 0.3 rho cos theta grows with theta, so its
    # largest value eta_k^2 over that region lies on the curve theta = theta_max(rho): taken over 2001 values of rho, plus 1e-5.
    # The push n_a - n_b is within eta_a + eta_b of the ideal push: its angle from +x is at most the ideal's plus
    # asin((eta_a + eta_b) / |ideal|).  The eps of this mesh (0.0004 and 0.0115) allow 63 and 57 degrees at lattice depths 5 and 6;
    # the restatement's pushes are 1.9 and 1.3 degrees off.
    (ca_, cb_), eps_out, eps_in = lens_geometry()
    R_in, R_out = 0.15 - eps_in, 0.15 + eps_out
    for d in (5, 6):
        r = pc.restated("lens", d)[0][0]
        p = clr.lattice(d)[0][int(r["witness"])].astype(np.float64)
        ideal, eta = [], 0.0
        for c in (ca_, cb_):
            u = float(np.linalg.norm(p - c))
            assert 0 < u < R_in
            rho = np.linspace(R_in, R_out, 2001)
            cos_t = np.clip((rho ** 2 + u ** 2 - (R_out - u) ** 2) / (2 * rho * u), -1.0, 1.0)
            eta += float(np.sqrt((rho ** 2 + 0.15 ** 2 - 0.3 * rho * cos_t).max())) + 1e-5
            ideal.append(c + 0.15 * (p - c) / u)
        ideal = ideal[0] - ideal[1]
        push = sb.penetration_push(r)
        assert np.array_equal(push, r["nearest_a"].astype(np.float64) - r["nearest_b"].astype(np.float64))
        assert np.linalg.norm(push - ideal) <= eta + 1e-6
        allowed = float(np.arccos(ideal[0] / np.linalg.norm(ideal))) + float(np.arcsin(min(1.0, eta / np.linalg.norm(ideal))))
        angle = float(np.arccos(push[0] / np.linalg.norm(push)))
        print(f"lens depth {d}: push {push}, {np.degrees(angle):.2f} deg from +x, allowed {np.degrees(allowed):.2f}; |push| {np.linalg.norm(push):.5f}, "
              f"ra + rb {float(r['ra']) + float(r['rb']):.5f}")
        assert push[0] > 0 and angle <= allowed
        # |n_a - n_b| <= |n_a - p| + |p - n_b| = ra + rb, and about that
        assert np.linalg.norm(push) <= (float(r["ra"]) + float(r["rb"])) * (1 + 1e-5)
        assert np.linalg.norm(push) >= float(r["ra"]) + float(r["rb"]) - 2 * eta


def test_the_records_are_the_headers(sb):
    text = open(os.path.join(REPO, "include", "sdfhip.h")).read()
    widths = {"float": 4, "uint32_t": 4, "uint64_t": 8}
    for c_name, cls, dtype, size in (("sdfhip_penetration", sb.Penetration, pr.PENETRATION, 64), ("sdfhip_penetration_options", sb.PenetrationOptions, None, 28),
                                     ("sdfhip_penetration_stats", sb.PenetrationStats, None, 72)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (c_name, c_name), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        off = 0
        names = []
        for decl in body.split(";"):
            words = decl.split()
            if not words:
                continue
            for n in " ".join(words[1:]).split(","):
                m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", n)
                name, count = m.group(1), int(m.group(2) or 1)
                assert getattr(cls, name).offset == off, (c_name, name)
                if dtype is not None:
                    assert dtype.fields[name][1] == off and dtype.fields[name][0].base.itemsize == widths[words[0]], (c_name, name)
                names.append(name)
                off += widths[words[0]] * count
        assert off == size == ctypes.sizeof(cls) and names == [f[0] for f in cls._fields_], c_name
    assert np.dtype(sb.Penetration) == pr.PENETRATION
    assert sb.PENETRATION_NO_SKIP == int(re.search(r"SDFHIP_PENETRATION_NO_SKIP\s*=\s*(\d+)", text).group(1)) == sb.CLASH_NO_SKIP
    # the options have the clash check's layout; the defaults, from the library and from the Python class
    assert [(n, t) for n, t in sb.PenetrationOptions._fields_] == [(n, t) for n, t in sb.ClashOptions._fields_]
    opt = sb.PenetrationOptions(flags=7, depth=1, origin=(1, 2, 3), side=9.0)
    sb._lib.lib.sdfhip_penetration_options_default(ctypes.byref(opt))
    for o in (opt, sb.PenetrationOptions()):
        assert (o.size, o.flags, o.depth, tuple(o.origin), o.side) == (28, 0, 6, (0.0, 0.0, 0.0), 1.0)
    sb._lib.lib.sdfhip_penetration_options_default(None)           # a null argument is a message, never a crash
    assert b"penetration_options_default" in sb._lib.lib.sdfhip_last_error()


def test_the_library_refuses_what_the_clash_check_refuses_word_for_word(sb):
    L = sb._lib
    R, s, t = cc.ONE_PLACEMENTS["generic_half"]()
    # (a list is checked to its end before its first handle is read: the address of a zeroed block stands in for the handles)
    block = (ctypes.c_uint8 * 4096)()
    fake = ctypes.c_void_p(ctypes.addressof(block))
    good = lambda **kw: sb.Instance(**dict(dict(scene=fake, op=0, rotation=R.tolist(), scale=s, translation=t.tolist()), **kw))
    out = np.zeros(4, np.dtype(sb.Penetration))
    clash_out = np.zeros(4, np.dtype(sb.Clash))
    n = ctypes.c_uint32(77)

    def refused(word, items, count=None, opt=None, out_ptr=True, capacity=4, n_pairs=True):
        arr = (sb.Instance * max(1, len(items)))(*items) if items is not None else None
        k = len(items or []) if count is None else count
        rc = L.lib.sdfhip_instances_penetration(arr, k, ctypes.byref(opt) if opt is not None else None, out.ctypes.data if out_ptr else None, capacity,
                                                ctypes.byref(n) if n_pairs else None, None)
        msg = L.lib.sdfhip_last_error()
        assert rc == L.ERR_ARG and word in msg and b"instances_penetration:" in msg, (word, rc, msg)
        assert n.value == 77 and not out.view(np.uint8).any()                          # nothing was written
        # ... and the clash check says the same of the same arguments, but for the names
        copt = None
        if opt is not None:
            copt = ctypes.cast(ctypes.pointer(opt), ctypes.POINTER(sb.ClashOptions)).contents
        assert L.lib.sdfhip_instances_clash(arr, k, ctypes.byref(copt) if copt is not None else None, clash_out.ctypes.data if out_ptr else None, capacity,
                                            ctypes.byref(n) if n_pairs else None, None) == L.ERR_ARG
        said = L.lib.sdfhip_last_error().replace(b"instances_clash", b"instances_penetration").replace(b"sdfhip_clash_options", b"sdfhip_penetration_options")
        assert said == msg, (said, msg)

    refused(b"null instance list", None, count=1)
    refused(b"1..64", [good()], count=0)
    refused(b"1..64", [good()] * 65)
    refused(b"SDFHIP_CLASH_MAX_INSTANCES", [good()] * 65)
    refused(b"65 instances", [good()] * 65)
    refused(b"null n_pairs", [good()], n_pairs=False)
    refused(b"null out", [good()], out_ptr=False)
    five = lambda bad: [good(), good(op=2), good(), bad, good()]
    for bad, word in ((good(op=3), b"unknown op"), (good(op=-1), b"unknown op"),
                      (good(rotation=((1, 0, 0), (0, 1, 0), (0, 0, 1.001))), b"orthogonal"), (good(scale=0.0), b"scale"),
                      (good(scale=float("nan")), b"finite"), (good(translation=(0.0, float("inf"), 0.0)), b"finite")):
        refused(b"instance 3", five(bad))
        refused(word, five(bad))
    refused(b"instance 0", [good(op=1), good()])
    refused(b"instance 0: null scene", [good(scene=None)])
    refused(b"instance 3: null scene", five(good(scene=None)))
    # the options
    refused(b"depth", [good()], opt=sb.PenetrationOptions(depth=11))
    refused(b"flags", [good()], opt=sb.PenetrationOptions(flags=2))
    for bad in (float("nan"), float("inf")):
        refused(b"origin", [good()], opt=sb.PenetrationOptions(origin=(0.0, bad, 0.0)))
    for bad in (float("nan"), float("inf"), 0.0, -1.0):
        refused(b"side", [good()], opt=sb.PenetrationOptions(side=bad))
    small = sb.PenetrationOptions()
    small.size = 8
    refused(b"bytes", [good()], opt=small)

    class Newer(ctypes.Structure):
        _fields_ = sb.PenetrationOptions._fields_ + [("unknown", ctypes.c_int32)]
    newer = Newer()
    ctypes.memmove(ctypes.byref(newer), ctypes.byref(sb.PenetrationOptions()), 28)
    newer.size, newer.unknown = 32, 3
    as_options = ctypes.cast(ctypes.pointer(newer), ctypes.POINTER(sb.PenetrationOptions)).contents
    refused(b"", [good()], opt=as_options)                     # an unknown field that is set
    newer.unknown = -1
    refused(b"null scene", [good(scene=None)], opt=as_options) # ... and one that says "default": the call goes on to the list


def test_the_python_layer_refuses_what_needs_no_handle(sb):
    for bad in ([], [7], [("not a scene", (np.eye(3), 1.0, (0, 0, 0)))], [(None, (np.eye(3), 1.0, (0, 0, 0)), 0, 0)]):
        with pytest.raises(ValueError):
            sb.Scene.PenetrationParts(bad)

    class Unloaded(sb.Scene):
        def __init__(self):
            self._h = None
    part = (Unloaded(), (np.eye(3), 1.0, (0, 0, 0)))
    with pytest.raises(sb.SdfHipError) as e:
        sb.Scene.PenetrationParts([part] * 65)
    assert e.value.code == sb._lib.ERR_ARG and "64" in str(e.value)
    with pytest.raises(sb.SdfHipError) as e:
        sb.Scene.PenetrationParts([part], depth=11)
    assert e.value.code == sb._lib.ERR_ARG


def test_the_cpp_mirror_checks_its_arguments_and_fails_loudly_without_a_gpu(tmp_path):
    # Program::PenetrationParts (include/sdfbox.hpp) through tests/cpp_penetration.cpp: what it refuses needs no GPU; with one the
    # bytes are tests/test_gpu_penetration.py's
    import shutil
    import torch
    from conftest import GOLDEN
    exe, libdir = str(tmp_path / "cpp_penetration"), os.path.join(REPO, "sdfbox_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "cpp_penetration.cpp"),
                           "-o", exe, "-L", libdir, "-lsdfhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    shutil.copy(os.path.join(GOLDEN, "sphere_d4.asdf"), tmp_path / "sphere.asdf")
    out = subprocess.run([exe, str(tmp_path / "sphere.asdf"), "5", str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert "argument checks ok" in out.stderr, (out.returncode, out.stderr)
    if torch.cuda.is_available():
        assert out.returncode == 0, out.stderr
    else:
        assert out.returncode == 3 and "sdfhip:" in out.stderr, (out.returncode, out.stderr)

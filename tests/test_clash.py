"""The restatement of sdfhip_instances_clash (tests/clash_restatement.py) held to things it did not come from -- counts pinned from a
prototype written another way, the lattice's partition into octants, the list reversed, compose_restatement's fold, the closed form
of a lens -- and what the bindings refuse before a handle exists.  No GPU: tests/test_gpu_clash.py holds the GPU to the restatement,
byte for byte."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import clash_cases as ca
import clash_restatement as clr
import compose_cases as cc
import compose_restatement as cr
from conftest import REPO

f32 = np.float32


def test_the_counts_a_prototype_written_another_way_gave():
    # (that prototype placed the points as i * pitch + origin on the half-shifted cube, which is exact at these sizes)
    assert ca.as_dict(ca.restated("csg", 5)) == {(0, 1): 150, (0, 2): 948, (1, 2): 363}
    assert ca.as_dict(ca.restated("csg", 2)) == {(0, 2): 2}
    assert len(ca.restated("csg", 0)) == 0 and len(ca.restated("csg", 1)) == 0
    assert ca.as_dict(ca.restated("lens", 5)) == {(0, 1): 60} and ca.as_dict(ca.restated("lens", 6)) == {(0, 1): 504}
    chain = ca.as_dict(ca.restated("chain64", 5))
    assert len(chain) == 480 and min(chain.values()) == 4 and max(b - a for a, b in chain) == 9 and chain[(0, 1)] == 32
    same = ca.restated("same64", 3)
    assert len(same) == 2016 and (same["points"] == 8).all()
    assert [(int(r["a"]), int(r["b"])) for r in same] == [(a, b) for a in range(64) for b in range(a + 1, 64)]        # (a, b) order
    assert ca.as_dict(ca.restated("deepest", 5)) == {(0, 1): 80}
    for name in ("eight", "far", "two_spheres", "one"):
        assert len(ca.restated(name, 5 if name != "one" else 3)) == 0, name
    assert len(ca.parts(ca.REFUSED)) == 65
    with pytest.raises(ValueError):
        clr.clash(cr.as_instances(cc.with_trees(ca.parts(ca.REFUSED))), 0)


def test_a_record_is_what_its_fields_say():
    # first is a witness inside both and inside the bounds; the bounds are tight to the sums' means; the off-cube box moves them
    d = 5
    for box in (ca.UNIT, ca.OFF_CUBE):
        rec = ca.restated("csg", d, box)
        assert len(rec) >= 1
        p, x, y, z = clr.lattice(d, *box)
        inside = clr.contains(ca.instances("csg"), p)
        for r in rec:
            assert inside[r["a"], r["first"]] and inside[r["b"], r["first"]] and r["a"] < r["b"] and r["points"] >= 1
            c = np.array([x[r["first"]], y[r["first"]], z[r["first"]]])
            assert (r["lo"] <= c).all() and (c <= r["hi"]).all()
            mean = r["sum"] / float(r["points"])
            assert (r["lo"] <= mean).all() and (mean <= r["hi"]).all()
            assert r["points"] <= np.prod(r["hi"].astype(np.int64) - r["lo"] + 1)
    assert ca.as_dict(ca.restated("csg", d, ca.OFF_CUBE)) != ca.as_dict(ca.restated("csg", d))


def test_the_eight_octants_partition_the_lattice():
    # depth d on the unit cube = the eight calls (origin in {0, 0.5}^3, side 0.5, depth d - 1): the points coincide exactly in fp32
    d = 5
    whole = ca.restated("csg", d)
    half = 1 << (d - 1)
    acc = {}
    for o in range(8):
        off = np.array([o & 1, o >> 1 & 1, o >> 2], dtype=np.int64)
        p_oct = clr.lattice(d - 1, tuple(0.5 * off), 0.5)[0]
        p_all, x, y, z = clr.lattice(d)
        sel = ((x >= half) == bool(off[0])) & ((y >= half) == bool(off[1])) & ((z >= half) == bool(off[2]))
        assert np.array_equal(p_oct.view(np.uint32), p_all[sel].view(np.uint32))
        for r in clr.clash(ca.instances("csg"), d - 1, tuple(0.5 * off), 0.5):
            f = int(r["first"])
            fx, fy, fz = (f & (half - 1)) + half * off[0], (f >> (d - 1) & (half - 1)) + half * off[1], (f >> (2 * (d - 1))) + half * off[2]
            first = int(fz) << (2 * d) | int(fy) << d | int(fx)
            got = acc.setdefault((int(r["a"]), int(r["b"])), dict(points=0, first=1 << 32, lo=np.full(3, 1 << 32), hi=np.zeros(3, np.int64), sum=np.zeros(3, np.int64)))
            got["points"] += int(r["points"])
            got["first"] = min(got["first"], first)
            got["lo"] = np.minimum(got["lo"], r["lo"].astype(np.int64) + half * off)
            got["hi"] = np.maximum(got["hi"], r["hi"].astype(np.int64) + half * off)
            got["sum"] = got["sum"] + r["sum"].astype(np.int64) + half * off * int(r["points"])
    assert sorted(acc) == [(int(r["a"]), int(r["b"])) for r in whole]
    for r in whole:
        got = acc[(int(r["a"]), int(r["b"]))]
        assert got["points"] == r["points"] and got["first"] == r["first"]
        assert (got["lo"] == r["lo"]).all() and (got["hi"] == r["hi"]).all() and (got["sum"] == r["sum"].astype(np.int64)).all()


@pytest.mark.parametrize("name, d", [("csg", 5), ("three_forms", 5), ("lens", 5)])
def test_the_list_reversed_gives_the_pairs_mirrored(name, d):
    inst = ca.instances(name)
    K = len(inst)
    back = clr.clash(inst[::-1], d)
    want = {(K - 1 - int(r["b"]), K - 1 - int(r["a"])): r for r in ca.restated(name, d)}
    assert sorted(want) == [(int(r["a"]), int(r["b"])) for r in back]
    for r in back:
        w = want[(int(r["a"]), int(r["b"]))]
        for field in ("points", "first", "lo", "hi", "sum"):
            assert np.array_equal(r[field], w[field]), (name, field)


def test_two_parts_share_what_their_intersection_holds():
    # points = the lattice points at which compose_restatement's fold of [a, (b, INTERSECT)] is below 0
    d = 5
    p = clr.lattice(d)[0]
    inst = ca.instances("csg")
    want = ca.as_dict(ca.restated("csg", d))
    for a in range(3):
        for b in range(a + 1, 3):
            pair = [(inst[a][0], inst[a][1], cr.COMBINE_UNION), (inst[b][0], inst[b][1], cr.COMBINE_INTERSECT)]
            assert int((cr.value(pair, p) < 0).sum()) == want.get((a, b), 0), (a, b)
    lens = ca.instances("lens")
    pair = [lens[0], (lens[1][0], lens[1][1], cr.COMBINE_INTERSECT)]
    assert int((cr.value(pair, p) < 0).sum()) == 60


def test_the_lens_of_two_balls_has_its_closed_form_volume():
    # Two balls of radius r whose centres are c = 0.2 apart share V = pi (4 r + c) (2 r - c)^2 / 12.  r is the radius of a ball
    # with the first part's own counted volume on the same lattice: the depth-4 source's surface is about 1.4 % short of 0.15,
    # which moves the thin lens by 8 %.  Measured here: -3.70 % at depth 5 and +1.38 % at depth 6 (the prototype: -3.5 % and +1.4 %);
    # the bound is twice the measured difference, and the finer lattice is the closer one.
    c = 0.2
    diff = {}
    for d in (5, 6):
        pitch = float(clr.pitch_of(d))
        part = int(clr.contains(ca.instances("lens")[:1], clr.lattice(d)[0]).sum()) * pitch ** 3
        r = (3.0 * part / (4.0 * np.pi)) ** (1.0 / 3.0)
        assert abs(r - 0.15) < 0.02 * 0.15
        V = np.pi * (4.0 * r + c) * (2.0 * r - c) ** 2 / 12.0
        diff[d] = (int(ca.restated("lens", d)["points"][0]) * pitch ** 3 - V) / V
    assert abs(diff[5]) < 2 * 0.0370 and abs(diff[6]) < 2 * 0.0138, diff
    assert abs(diff[6]) < abs(diff[5]), diff


def test_the_python_helpers_read_a_record(sb):
    d, (origin, side) = ca.OFF_CUBE_DEPTH, ca.OFF_CUBE
    r = ca.restated("csg", d, ca.OFF_CUBE)[0]
    pitch = side * 2.0 ** -d
    assert sb.clash_volume(r, d, side) == pytest.approx(int(r["points"]) * pitch ** 3, rel=1e-12)
    want = np.array(origin) + (r["sum"] / float(r["points"]) + 0.5) * pitch
    assert np.allclose(sb.clash_centroid(r, d, origin, side), want, rtol=0, atol=1e-12)
    o, s = sb.clash_box(r, d, origin, side)
    lo, hi = np.array(origin) + r["lo"] * pitch, np.array(origin) + (r["hi"] + 1.0) * pitch
    assert s == pytest.approx(float((hi - lo).max()), rel=1e-12)
    assert (np.array(o) <= lo + 1e-12).all() and (np.array(o) + s >= hi - 1e-12).all()           # the cube holds the cells lo..hi
    assert np.allclose(np.array(o) + s / 2, (lo + hi) / 2, rtol=0, atol=1e-12)                       # ... centred on them
    assert (sb.clash_centroid(r, d, origin, side) >= lo).all() and (sb.clash_centroid(r, d, origin, side) <= hi).all()


def test_the_records_are_the_headers(sb):
    text = open(os.path.join(REPO, "include", "sdfhip.h")).read()
    widths = {"float": 4, "uint32_t": 4, "uint64_t": 8}
    for c_name, cls, dtype, size in (("sdfhip_clash", sb.Clash, clr.CLASH, 64), ("sdfhip_clash_options", sb.ClashOptions, None, 28),
                                     ("sdfhip_clash_stats", sb.ClashStats, None, 32)):
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
    assert np.dtype(sb.Clash) == clr.CLASH
    assert sb.CLASH_NO_SKIP == int(re.search(r"SDFHIP_CLASH_NO_SKIP\s*=\s*(\d+)", text).group(1)) == 1
    assert sb.CLASH_MAX_INSTANCES == int(re.search(r"SDFHIP_CLASH_MAX_INSTANCES\s*=\s*(\d+)", text).group(1)) == clr.MAX_INSTANCES == 64
    # the defaults, from the library and from the Python class
    opt = sb.ClashOptions(flags=7, depth=1, origin=(1, 2, 3), side=9.0)
    sb._lib.lib.sdfhip_clash_options_default(ctypes.byref(opt))
    for o in (opt, sb.ClashOptions()):
        assert (o.size, o.flags, o.depth, tuple(o.origin), o.side) == (28, 0, 6, (0.0, 0.0, 0.0), 1.0)
    sb._lib.lib.sdfhip_clash_options_default(None)                 # a null argument is a message, never a crash
    assert b"clash_options_default" in sb._lib.lib.sdfhip_last_error()


def test_the_library_refuses_what_needs_no_handle(sb):
    L = sb._lib
    R, s, t = cc.ONE_PLACEMENTS["generic_half"]()
    # (a list is checked to its end before its first handle is read: the address of a zeroed block stands in for the handles)
    block = (ctypes.c_uint8 * 4096)()
    fake = ctypes.c_void_p(ctypes.addressof(block))
    good = lambda **kw: sb.Instance(**dict(dict(scene=fake, op=0, rotation=R.tolist(), scale=s, translation=t.tolist()), **kw))
    out = np.zeros(4, np.dtype(sb.Clash))
    n = ctypes.c_uint32(77)

    def refused(word, items, count=None, opt=None, out_ptr=out.ctypes.data, capacity=4, n_pairs=n):
        arr = (sb.Instance * max(1, len(items)))(*items) if items is not None else None
        k = len(items or []) if count is None else count
        rc = L.lib.sdfhip_instances_clash(arr, k, ctypes.byref(opt) if opt is not None else None, out_ptr, capacity,
                                          ctypes.byref(n_pairs) if n_pairs is not None else None, None)
        msg = L.lib.sdfhip_last_error()
        assert rc == L.ERR_ARG and word in msg and b"instances_clash:" in msg, (word, rc, msg)
        assert n.value == 77 and not out.view(np.uint8).any()                          # nothing was written

    refused(b"null instance list", None, count=1)
    refused(b"1..64", [good()], count=0)
    refused(b"1..64", [good()] * 65)
    refused(b"SDFHIP_CLASH_MAX_INSTANCES", [good()] * 65)
    refused(b"65 instances", [good()] * 65)
    refused(b"null n_pairs", [good()], n_pairs=None)
    refused(b"null out", [good()], out_ptr=None)
    five = lambda bad: [good(), good(op=2), good(), bad, good()]
    for bad, word in ((good(op=3), b"unknown op"), (good(op=-1), b"unknown op"),
                      (good(rotation=((1, 0, 0), (0, 1, 0), (0, 0, 1.001))), b"orthogonal"), (good(scale=0.0), b"scale"),
                      (good(scale=float("nan")), b"finite"), (good(translation=(0.0, float("inf"), 0.0)), b"finite")):
        refused(b"instance 3", five(bad))
        refused(word, five(bad))
    refused(b"instance 0", [good(op=1), good()])
    refused(b"instance 0: null scene", [good(scene=None)])
    refused(b"instance 3: null scene", five(good(scene=None)))
    # ... word for word what sdfhip_instances_sample says of the same list
    buf = (ctypes.c_float * 64)()
    arr = (sb.Instance * 5)(*five(good(scale=-1.0)))
    assert L.lib.sdfhip_instances_sample(arr, 5, None, buf, 1, buf) == L.ERR_ARG
    said = L.lib.sdfhip_last_error().replace(b"instances_sample", b"instances_clash")
    assert L.lib.sdfhip_instances_clash(arr, 5, None, out.ctypes.data, 4, ctypes.byref(n), None) == L.ERR_ARG and L.lib.sdfhip_last_error() == said
    # the options
    refused(b"depth", [good()], opt=sb.ClashOptions(depth=11))
    refused(b"flags", [good()], opt=sb.ClashOptions(flags=2))
    for bad in (float("nan"), float("inf")):
        refused(b"origin", [good()], opt=sb.ClashOptions(origin=(0.0, bad, 0.0)))
    for bad in (float("nan"), float("inf"), 0.0, -1.0):
        refused(b"side", [good()], opt=sb.ClashOptions(side=bad))
    small = sb.ClashOptions()
    small.size = 8
    refused(b"bytes", [good()], opt=small)

    class Newer(ctypes.Structure):
        _fields_ = sb.ClashOptions._fields_ + [("unknown", ctypes.c_int32)]
    newer = Newer()
    ctypes.memmove(ctypes.byref(newer), ctypes.byref(sb.ClashOptions()), 28)
    newer.size, newer.unknown = 32, 3
    as_options = ctypes.cast(ctypes.pointer(newer), ctypes.POINTER(sb.ClashOptions)).contents
    refused(b"", [good()], opt=as_options)                     # an unknown field that is set
    newer.unknown = -1
    refused(b"null scene", [good(scene=None)], opt=as_options) # ... and one that says "default": the call goes on to the list


def test_the_python_layer_refuses_what_needs_no_handle(sb):
    for bad in ([], [7], [("not a scene", (np.eye(3), 1.0, (0, 0, 0)))], [(None, (np.eye(3), 1.0, (0, 0, 0)), 0, 0)]):
        with pytest.raises(ValueError):
            sb.Scene.ClashParts(bad)

    class Unloaded(sb.Scene):
        def __init__(self):
            self._h = None
    part = (Unloaded(), (np.eye(3), 1.0, (0, 0, 0)))
    with pytest.raises(sb.SdfHipError) as e:
        sb.Scene.ClashParts([part] * 65)
    assert e.value.code == sb._lib.ERR_ARG and "64" in str(e.value)
    with pytest.raises(sb.SdfHipError) as e:
        sb.Scene.ClashParts([part], depth=11)
    assert e.value.code == sb._lib.ERR_ARG


def test_the_cpp_mirror_checks_its_arguments_and_fails_loudly_without_a_gpu(tmp_path):
    # Program::ClashParts (include/sdfbox.hpp) through tests/cpp_clash.cpp: what it refuses needs no GPU; with one the bytes are
    # tests/test_gpu_clash.py's
    import shutil
    import torch
    from conftest import GOLDEN
    exe, libdir = str(tmp_path / "cpp_clash"), os.path.join(REPO, "sdfbox_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "cpp_clash.cpp"),
                           "-o", exe, "-L", libdir, "-lsdfhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    shutil.copy(os.path.join(GOLDEN, "sphere_d4.asdf"), tmp_path / "sphere.asdf")
    out = subprocess.run([exe, str(tmp_path / "sphere.asdf"), "5", str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert "argument checks ok" in out.stderr, (out.returncode, out.stderr)
    if torch.cuda.is_available():
        assert out.returncode == 0, out.stderr
    else:
        assert out.returncode == 3 and "sdfhip:" in out.stderr, (out.returncode, out.stderr)

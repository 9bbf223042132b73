"""The restatement of sdfhip_instances_gap (tests/gap_restatement.py) held to things it did not come from -- the list reversed, the
limit on either side of a gap, two balls in closed form, and that the witness is the emitted vertex `corner` of its node -- the cases
held to what they are for, and what the bindings refuse before a handle exists.  (The comparison with distance_restatement.distance
at the witness is a check of the record's bookkeeping, not an independent one: both rest on distance_restatement.nearest.)  No GPU: tests/test_gpu_gap.py holds the GPU to the restatement, byte
for byte."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import compose_cases as cc
import distance_restatement as dr
import gap_cases as gc
import gap_restatement as gr
import penetration_restatement as pr
import place_restatement as plr
from conftest import REPO

f32 = np.float32


def bits(x):
    return np.asarray(x, dtype=f32).view(np.uint32)


def test_the_cases_are_what_they_are_for():
    # apart: the two directions differ in the last bits, so the minimum over both is exercised
    inst = gc.instances("apart")
    ca, cb = gr.candidates(inst[0]), gr.candidates(inst[1])
    d0, d1 = pr.searched(inst[1], ca[0])[0].min(), pr.searched(inst[0], cb[0])[0].min()
    assert (d0, d1) == (f32(0.10523171), f32(0.10523173)) and int(bits(d1)) - int(bits(d0)) == 3
    rec = gc.restated("apart")[0]
    assert len(rec) == 1 and rec["gap"][0] == d0 and rec["flags"][0] == 0
    # same2: gap 0.0 exactly, a tie at every vertex; the witness is the first vertex emitted
    rec = gc.restated("same2")[0]
    assert len(rec) == 1 and bits(rec["gap"])[0] == 0 and not rec["flags"][0] & gr.WITNESS_OF_B and rec["corner"][0] == 0
    inst = gc.instances("same2")
    c = gr.candidates(inst[0])
    assert (pr.searched(inst[1], c[0])[0] == 0).all() and rec["node_a"][0] == c[1][0] and (rec["point_a"][0] == rec["point_b"][0]).all()
    # nested: the small ball lies inside the large one
    rec = gc.restated("nested")[0]
    assert len(rec) == 1 and rec["gap"][0] == f32(0.20306647) and rec["flags"][0] & gr.CONTAINED
    # generic: the part without a surface gives no record
    rec = gc.restated("generic")[0]
    assert len(gr.candidates(gc.instances("generic")[2])[0]) == 0
    assert [(int(r["a"]), int(r["b"])) for r in rec] == [(0, 1)] and rec["gap"][0] == f32(0.30939227)
    # row64: every pair has a record, and the limit the GPU test uses lies between two of the gaps
    rec = gc.restated("row64")[0]
    assert len(rec) == 2016 and 0 < (rec["gap"] <= f32(gc.ROW64_LIMIT)).sum() < 2016 and not (rec["gap"] == f32(gc.ROW64_LIMIT)).any()
    assert len(gc.restated("row64", gc.ROW64_LIMIT)[0]) == int((rec["gap"] <= f32(gc.ROW64_LIMIT)).sum())
    # lens: overlapping surfaces; far: a part three cubes away; big_list: 31 880 triangles against 12 -- a cut-cell list of many
    # workgroups' counts, each thread of the shared scan with more than one chunk or none; zoo: depth 12
    assert gc.restated("lens")[0]["gap"][0] < 0.01
    assert gc.restated("far")[0]["gap"][0] > 2
    assert len(pr.surface_of(gc.instances("big_list")[0][0])) == 31880 and len(pr.surface_of(gc.instances("big_list")[1][0])) == 12
    from edit_restatement import tree_depth
    assert tree_depth(gc.tree(gc.ZOO_TREE)[0]) == 12 and len(gc.restated("zoo")[0]) == 1
    # the closed count: 3 x the triangles of the first part of every ordered pair with two surfaces
    T = [len(pr.surface_of(i[0])) for i in gc.instances("generic")]
    assert T[2] == 0 and gc.restated("generic")[1]["searches"] == 3 * (T[0] + T[1])


@pytest.mark.parametrize("name", gc.NAMES)
def test_the_witness_is_what_the_distance_restatement_says(name):
    # |sdfhip_scene_distance's distance| at the inverse-mapped witness vertex, times s, is the gap; its nearest point mapped forward
    # and its node are the record's other side.  NOT independent of the restatement: penetration_restatement.searched and
    # distance_restatement.distance both rest on distance_restatement.nearest, so this holds the record's bookkeeping (which side,
    # which map, which fields) and no more.  Independent: the witness vertex is the emitted vertex `corner` of its node, by the
    # mesh restatement's own order
    inst = gc.instances(name)
    rec = gc.restated(name)[0]
    assert len(rec) >= 1
    for r in rec[::97]:
        second = bool(r["flags"] & gr.WITNESS_OF_B)
        mine, other = (r["b"], r["a"]) if second else (r["a"], r["b"])
        w, far = (r["point_b"], r["point_a"]) if second else (r["point_a"], r["point_b"])
        node, far_node = (r["node_b"], r["node_a"]) if second else (r["node_a"], r["node_b"])
        src, (R, s, t), _ = inst[other]
        q = np.stack(plr.inverse_map(w[None], R, s, t), 1)
        c = dr.distance(src[0], src[1], q, surf=pr.surface_of(src))[0]
        assert bits(np.abs(c["distance"]) * s) == bits(r["gap"]) and c["node"] == far_node
        assert bits(pr.forward_map(c["nearest"][None], R, s, t)[0]).tolist() == bits(far).tolist()
        # the witness: vertex corner % 3 of triangle corner // 3 among its node's triangles
        src, (R, s, t), _ = inst[mine]
        surf = pr.surface_of(src)
        tri = np.nonzero(surf.cell == node)[0][int(r["corner"]) // 3]
        assert bits(pr.forward_map(surf.pos[tri, int(r["corner"]) % 3][None], R, s, t)[0]).tolist() == bits(w).tolist()
        assert bits(gr.gap_vector(r)).tolist() == bits(r["point_b"] - r["point_a"]).tolist()


@pytest.mark.parametrize("name", ["apart", "nested", "generic", "lens", "big_list", "zoo", "row8"])
def test_the_list_reversed_gives_the_same_gaps_with_a_and_b_swapped(name):
    inst = gc.instances("row64")[:8] if name == "row8" else gc.instances(name)
    K = len(inst)
    fwd = gr.gap(inst) if name == "row8" else gc.restated(name)[0]
    back = gr.gap(inst[::-1])
    assert len(fwd) == len(back) >= 1
    mirrored = {(K - 1 - int(r["b"]), K - 1 - int(r["a"])): bits(r["gap"]) for r in back}
    for r in fwd:
        assert mirrored[(int(r["a"]), int(r["b"]))] == bits(r["gap"]), (name, r)


@pytest.mark.parametrize("name", ["generic", "zoo", "lens"])
def test_a_limit_at_the_gap_keeps_the_record_and_one_just_below_drops_it(name):
    inst = gc.instances(name)
    full = gc.restated(name)[0]
    g = full["gap"][0]
    for limit in (g, np.nextafter(g, f32(np.inf)), f32(1e30)):
        assert gr.gap(inst, limit).tobytes() == full[full["gap"] <= limit].tobytes() == gc.restated(name, limit)[0].tobytes()
    assert len(gr.gap(inst, np.nextafter(g, f32(-np.inf)))) == len(full) - int((full["gap"] == g).sum())
    for bad in (np.nan, -1.0, -np.inf):
        with pytest.raises(ValueError):
            gr.gap(inst, bad)


def test_two_balls_in_closed_form():
    # Part k's mesh lies between the spheres of radius m_k (the exact in-radius: the distance from its centre to its nearest triangle)
    # and M_k (its farthest vertex; a triangle is no farther than its vertices) round its centre c_k.  Every vertex v of a has
    # r_b(v) >= |v - c_b| - M_b >= D - M_a - M_b, and the vertex of a nearest to c_b has r_b(v) <= |v - c_b| - m_b: the segment from v
    # to c_b crosses b's closed mesh at or beyond m_b from c_b.  All in float64 from the restated meshes; eps = 1e-6 covers a handful
    # of fp32 roundings of coordinates below 2
    eps = 1e-6
    inst = gc.instances("apart")
    g = float(gc.restated("apart")[0]["gap"][0])
    centre, M, m, verts = [], [], [], []
    for src, (R, s, t), _ in inst:
        c = np.asarray(t, np.float64) + float(s) * np.full(3, 0.5)
        w = gr.candidates((src, (R, s, t), 0))[0].astype(np.float64)
        best, win, _ = dr.nearest(pr.surface_of(src), np.full((1, 3), 0.5, f32))
        assert win[0] >= 0
        centre.append(c); verts.append(w)
        M.append(np.linalg.norm(w - c, axis=1).max())
        m.append(np.sqrt(float(best[0])) * float(s))
    D = np.linalg.norm(centre[0] - centre[1])
    upper = min(np.linalg.norm(verts[0] - centre[1], axis=1).min() - m[1], np.linalg.norm(verts[1] - centre[0], axis=1).min() - m[0])
    assert D - M[0] - M[1] - eps <= g <= upper + eps, (D - M[0] - M[1], g, upper)
    assert 0 < upper - (D - M[0] - M[1]) < 0.05          # the bracket is not vacuous


def test_the_records_are_the_headers(sb):
    text = open(os.path.join(REPO, "include", "sdfhip.h")).read()
    widths = {"float": 4, "uint32_t": 4, "uint64_t": 8}
    for c_name, cls, dtype, size in (("sdfhip_gap", sb.Gap, gr.GAP, 64), ("sdfhip_gap_options", sb.GapOptions, None, 12), ("sdfhip_gap_stats", sb.GapStats, None, 56)):
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
    assert np.dtype(sb.Gap) == gr.GAP
    assert sb.GAP_NO_PRUNE == int(re.search(r"SDFHIP_GAP_NO_PRUNE\s*=\s*(\d+)", text).group(1))
    assert (sb.GAP_WITNESS_OF_B, sb.GAP_CONTAINED) == (gr.WITNESS_OF_B, gr.CONTAINED) == (1, 2)
    assert re.search(r"SDFHIP_GAP_WITNESS_OF_B\s*=\s*1,\s*SDFHIP_GAP_CONTAINED\s*=\s*2", text)
    opt = sb.GapOptions(flags=7, limit=3.0)
    sb._lib.lib.sdfhip_gap_options_default(ctypes.byref(opt))
    for o in (opt, sb.GapOptions()):
        assert (o.size, o.flags, o.limit) == (12, 0, float("inf"))
    sb._lib.lib.sdfhip_gap_options_default(None)           # a null argument is a message, never a crash
    assert b"gap_options_default" in sb._lib.lib.sdfhip_last_error()
    # what the header must say of the value and of the counters
    section = text[text.index("clearance: how far apart"):text.index("SDFHIP_API void sdfhip_gap_options_default")]
    for words in ("VERTEX-TO-SURFACE", "edge-to-edge", "never below the distance between the two triangle sets", "sqrt(3) / 2 * s * 2^-depth",
                  "DIFFER FROM CALL TO CALL"):
        assert words in section, words


def test_the_library_refuses_what_the_clash_check_refuses_word_for_word(sb):
    L = sb._lib
    R, s, t = cc.ONE_PLACEMENTS["generic_half"]()
    # (a list is checked to its end before its first handle is read: the address of a zeroed block stands in for the handles)
    block = (ctypes.c_uint8 * 4096)()
    fake = ctypes.c_void_p(ctypes.addressof(block))
    good = lambda **kw: sb.Instance(**dict(dict(scene=fake, op=0, rotation=R.tolist(), scale=s, translation=t.tolist()), **kw))
    out = np.zeros(4, np.dtype(sb.Gap))
    clash_out = np.zeros(4, np.dtype(sb.Clash))
    n = ctypes.c_uint32(77)

    def refused(word, items, count=None, opt=None, out_ptr=True, capacity=4, n_pairs=True, clash_too=True):
        arr = (sb.Instance * max(1, len(items)))(*items) if items is not None else None
        k = len(items or []) if count is None else count
        rc = L.lib.sdfhip_instances_gap(arr, k, ctypes.byref(opt) if opt is not None else None, out.ctypes.data if out_ptr else None, capacity,
                                        ctypes.byref(n) if n_pairs else None, None)
        msg = L.lib.sdfhip_last_error()
        assert rc == L.ERR_ARG and word in msg and b"instances_gap:" in msg, (word, rc, msg)
        assert n.value == 77 and not out.view(np.uint8).any()                          # nothing was written
        if not clash_too:
            return
        # ... and the clash check says the same of the same list, but for the name (and for what it says of the limit's reason)
        assert L.lib.sdfhip_instances_clash(arr, k, None, clash_out.ctypes.data if out_ptr else None, capacity, ctypes.byref(n) if n_pairs else None,
                                            None) == L.ERR_ARG
        said = L.lib.sdfhip_last_error().replace(b"instances_clash", b"instances_gap")
        assert said.split(b" (SDFHIP_CLASH_MAX_INSTANCES")[0] == msg.split(b" (SDFHIP_CLASH_MAX_INSTANCES")[0], (said, msg)

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
    refused(b"flags", [good()], opt=sb.GapOptions(flags=2), clash_too=False)
    for bad in (float("nan"), -1.0, float("-inf"), -1e-30):
        refused(b"limit", [good()], opt=sb.GapOptions(limit=bad), clash_too=False)
    small = sb.GapOptions()
    small.size = 8
    refused(b"bytes", [good()], opt=small, clash_too=False)

    class Newer(ctypes.Structure):
        _fields_ = sb.GapOptions._fields_ + [("unknown", ctypes.c_int32)]
    newer = Newer()
    ctypes.memmove(ctypes.byref(newer), ctypes.byref(sb.GapOptions()), 12)
    newer.size, newer.unknown = 16, 3
    as_options = ctypes.cast(ctypes.pointer(newer), ctypes.POINTER(sb.GapOptions)).contents
    refused(b"", [good()], opt=as_options, clash_too=False)                     # an unknown field that is set
    newer.unknown = -1
    refused(b"null scene", [good(scene=None)], opt=as_options, clash_too=False) # ... and one that says "default": the call goes on to the list
    # a limit of 0 and of +inf are taken: the call goes on to the list
    for fine in (0.0, float("inf")):
        refused(b"null scene", [good(scene=None)], opt=sb.GapOptions(limit=fine), clash_too=False)


def test_the_python_layer_refuses_what_needs_no_handle(sb):
    for bad in ([], [7], [("not a scene", (np.eye(3), 1.0, (0, 0, 0)))], [(None, (np.eye(3), 1.0, (0, 0, 0)), 0, 0)]):
        with pytest.raises(ValueError):
            sb.Scene.GapParts(bad)

    class Unloaded(sb.Scene):
        def __init__(self):
            self._h = None
    part = (Unloaded(), (np.eye(3), 1.0, (0, 0, 0)))
    with pytest.raises(sb.SdfHipError) as e:
        sb.Scene.GapParts([part] * 65)
    assert e.value.code == sb._lib.ERR_ARG and "64" in str(e.value)
    with pytest.raises(sb.SdfHipError) as e:
        sb.Scene.GapParts([part], limit=-1.0)
    assert e.value.code == sb._lib.ERR_ARG
    rec = np.zeros(1, gr.GAP)[0]
    rec["point_a"], rec["point_b"] = (1, 2, 3), (1.5, 2, 2)
    assert sb.gap_vector(rec).tolist() == [0.5, 0.0, -1.0]


def test_the_cpp_mirror_checks_its_arguments_and_fails_loudly_without_a_gpu(tmp_path):
    # Program::GapParts (include/sdfbox.hpp) through tests/cpp_gap.cpp: what it refuses needs no GPU; with one the bytes are
    # tests/test_gpu_gap.py's
    import shutil
    import torch
    from conftest import GOLDEN
    exe, libdir = str(tmp_path / "cpp_gap"), os.path.join(REPO, "sdfbox_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "cpp_gap.cpp"),
                           "-o", exe, "-L", libdir, "-lsdfhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    shutil.copy(os.path.join(GOLDEN, "sphere_d4.asdf"), tmp_path / "sphere.asdf")
    out = subprocess.run([exe, str(tmp_path / "sphere.asdf"), str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert "argument checks ok" in out.stderr, (out.returncode, out.stderr)
    if torch.cuda.is_available():
        assert out.returncode == 0, out.stderr
    else:
        assert out.returncode == 3 and "sdfhip:" in out.stderr, (out.returncode, out.stderr)

"""Smooth blends and morphs on the GPU (sdfhip_scene_blend), both flavours of the library: every Blend and Morph result below is the
brute-force restatement's (tests/blend_restatement.py: every point against every triangle of both restated meshes, no search, no
pruning) byte for byte, links and values -- a sphere against a torus, against itself with a crease carved into it, against an
off-centre sphere of another depth, and against the small hostile trees of tests/tree_zoo.py; all four operations; blend radii of
zero, a fraction of a cell and more than a leaf's band; t of 0, 0.5 and 1; results coarser than, as deep as and deeper than the
operands; operand surfaces of different levels; an operand blended with itself -- with the counters the call reports, the same call
twice, the chain into render, prune, combine and measure, and every refusal as its status code."""
import contextlib
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import blend_restatement as br
import combine_restatement as cr
import distance_restatement as dr
import measure_restatement as msr
import prune_restatement as pr
import tree_zoo
from conftest import REPO, assert_frames_identical, make_camera
from test_gpu_distance import surface
from test_gpu_distance import tree as distance_tree
from test_gpu_prune import assert_same_tree

pytestmark = pytest.mark.gpu
f32 = np.float32
U, I, SUB, M = br.UNION, br.INTERSECT, br.SUBTRACT, br.MORPH
OPS = {U: "union", I: "intersect", SUB: "subtract", M: "morph"}


@pytest.fixture(scope="module", params=["product", "lab"])
def sb(request):
    import sdfbox_amd
    if request.param == "product":
        return sdfbox_amd
    import sdfbox_amd.lab
    return sdfbox_amd.lab.load()


_own = {}


def tree(name):
    """the sources of tests/test_gpu_distance.py (its cache, its surfaces), and one more: a generated sphere of depth 3 off the centre"""
    if name == "sphere_off_d3":
        if name not in _own:
            import sdfbox_amd as base
            od = base.OctData.Generate(base._lib.SHAPE_SPHERE, [0.7, 0.58, 0.42, 0.2], 3)
            _own[name] = (od.Structs, od.Values)
        return _own[name]
    return distance_tree(name)


def surf(name, level=-1):
    if name == "sphere_off_d3":
        if (name, level) not in _own:
            _own[(name, level)] = dr.Surface(*tree(name), level)
        return _own[(name, level)]
    return surface(name, level)


# (op, amount, depth, level_a, level_b) per pair (A, B).  The brute force costs points x triangles x 2: results of depth 3 and 4 run
# against full surfaces; depth 5 only against level-2 surfaces, or where a SUBTRACT / INTERSECT leaves little to refine.  k: 0 (the hard
# operation), a fraction of a cell, and 0.2 -- more than the band of a depth-4 leaf (2 S = 0.125); t: 0, 0.5, 1.
CASES = {
    ("sphere_d4", "torus_d4"): [(U, 0.0, 3, -1, -1), (U, 0.03, 3, -1, -1), (U, 0.2, 3, -1, -1), (I, 0.03, 4, -1, -1), (SUB, 0.05, 3, -1, -1),
                                (M, 0.0, 3, -1, -1), (M, 0.5, 3, -1, -1), (M, 1.0, 3, -1, -1), (U, 0.03, 4, 2, -1), (I, 0.02, 5, 2, 2)],
    ("sphere_d4", "carved"): [(U, 0.03, 3, -1, -1), (I, 0.2, 3, -1, -1), (SUB, 0.0, 4, -1, -1), (M, 0.5, 4, 2, 2)],
    ("sphere_d4", "sphere_off_d3"): [(U, 0.05, -1, -1, -1), (SUB, 0.0, 3, -1, -1), (M, 0.5, 3, -1, -1), (I, 0.2, 4, -1, 2)],
    ("sphere_off_d3", "sphere_d4"): [(SUB, 0.03, 3, -1, -1), (M, 1.0, -1, -1, 2), (SUB, 0.02, 5, -1, -1)],
    ("leaf", "sphere_d4"): [(U, 0.03, 3, -1, -1), (I, 0.0, 3, -1, -1), (SUB, 0.2, 3, -1, -1), (M, 0.5, 3, -1, -1), (U, 0.02, 4, -1, 2)],
    ("chain12", "sphere_d4"): [(U, 0.03, 3, -1, -1), (M, 1.0, 3, -1, -1), (I, 0.03, 4, -1, 2)],
    ("blocks_65", "sphere_d4"): [(U, 0.0, 3, -1, -1), (SUB, 0.03, 3, -1, -1), (M, 0.5, 3, -1, 2)],
    ("blocks_257", "sphere_d4"): [(I, 0.03, 3, -1, -1), (U, 0.2, 3, -1, -1), (M, 0.0, 3, -1, -1), (SUB, 0.02, 5, 2, 2)],
    # an operand with itself: one bitmap where the levels agree, two where they do not
    ("sphere_d4", "sphere_d4"): [(SUB, 0.0, 3, -1, -1), (M, 0.5, 3, -1, -1), (U, 0.05, 3, -1, 2), (I, 0.03, 3, 2, 2)],
}
BIG = (("leaf", "empty"), (U, 0.02, 7, -1, -1))


def restated(pair, op, amount, depth, level_a, level_b):
    """(structs, values, counts) of the restatement, made once per process and left unchanged"""
    a, b = pair
    return tree_zoo.restated(("blend", a, b, op, float(amount), depth, level_a, level_b),
                             lambda: br.blend(tree(a), tree(b), op, amount, depth, level_a, level_b, want_counts=True,
                                              surf_a=surf(a, level_a), surf_b=surf(b, level_b)))


def upload(sb, name, **kw):
    return sb.Scene(sb.OctData(*tree(name)), **kw)


def describe(pair, case):
    op, amount, depth, la, lb = case
    return f"{OPS[op]}({pair[0]}, {pair[1]}, {amount}) depth={depth} levels={la},{lb}"


def check_call(sb, A, B, pair, case):
    """one call against its restatement: the tree byte for byte, and everything the call reports"""
    S, V, counts = restated(pair, *case)
    op, amount, depth, la, lb = case
    res, got, st = A.Blend(B, op, amount, None if depth < 0 else depth, la, lb, want_octdata=True, want_stats=True)
    what = describe(pair, case)
    with res:
        assert_same_tree(got, S, V, what)
        assert (st.nodes_a, st.nodes_b, st.nodes_out) == (len(tree(pair[0])[0]), len(tree(pair[1])[0]), len(S)), what
        assert (st.depth_out, st.levels, st.points) == (counts["depth_out"], counts["levels"], counts["points"]), what
        assert st.points == 9 + 35 * ((len(S) - 1) // 8), what
        assert res.Length == len(S) and res.depth == st.depth_out and res.stack_kernel_ok and st.pad0_ == 0 and st.pad_ == 0, what
        for visited, name, level in ((st.visited_a, pair[0], la), (st.visited_b, pair[1], lb)):
            assert visited == 0 if len(surf(name, level)) == 0 else visited >= st.points, what
    return st


@pytest.mark.parametrize("pair", list(CASES), ids=lambda p: f"{p[0]}-{p[1]}")
def test_blend_and_morph_bytes_are_the_restatements(sb, pair):
    with upload(sb, pair[0]) as A, (contextlib.nullcontext(A) if pair[0] == pair[1] else upload(sb, pair[1])) as B:
        for case in CASES[pair]:
            check_call(sb, A, B, pair, case)


def test_the_cases_are_what_they_are_for():
    cases = [(p, c) for p in CASES for c in CASES[p]]
    assert {c[0] for _, c in cases} == {U, I, SUB, M}
    assert {c[1] for _, c in cases if c[0] != M} >= {0.0, 0.03, 0.2} and {c[1] for _, c in cases if c[0] == M} == {0.0, 0.5, 1.0}
    assert {restated(p, *c)[2]["depth_out"] for p, c in cases} >= {3, 4, 5}
    assert any(c[3] != c[4] for _, c in cases) and any(p[0] == p[1] and c[3] == c[4] for p, c in cases) and any(p[0] == p[1] and c[3] != c[4] for p, c in cases)
    # depth 5 only against level-2 surfaces or where a SUBTRACT / INTERSECT leaves little
    assert all((c[3], c[4]) == (2, 2) or c[0] in (SUB, I) for _, c in cases if c[2] == 5)
    # operands of different depths, and depth = -1 is the deeper of the two
    from edit_restatement import tree_depth
    assert (tree_depth(tree("sphere_d4")[0]), tree_depth(tree("sphere_off_d3")[0])) == (4, 3)
    assert restated(("sphere_d4", "sphere_off_d3"), U, 0.05, -1, -1, -1)[2]["depth_out"] == 4
    assert restated(("sphere_off_d3", "sphere_d4"), M, 1.0, -1, -1, 2)[2]["depth_out"] == 4
    # the operands overlap partly: the hard pieces differ from either operand and from each other
    for other in ("torus_d4", "sphere_off_d3"):
        va, vb = msr.measure(*tree("sphere_d4")).volume, msr.measure(*tree(other)).volume
        both = msr.measure(*cr.combine(tree("sphere_d4"), tree(other), cr.COMBINE_INTERSECT)).volume
        assert 0 < both < 0.9 * min(va, vb), other
    assert msr.measure(*tree("carved")).volume < 0.95 * msr.measure(*tree("sphere_d4")).volume
    # a fillet adds material to a union: the larger k has the larger solid
    vols = [msr.measure(*restated(("sphere_d4", "torus_d4"), U, k, 3, -1, -1)[:2]).volume for k in (0.0, 0.03, 0.2)]
    assert vols[0] < vols[1] < vols[2], vols
    # a morph's ends: t = 0 is Offset(A, 0), t = 1 is b but for (b - a) + a's rounding -- the same split nodes at least
    S0, V0, _ = restated(("sphere_d4", "torus_d4"), M, 0.0, 3, -1, -1)
    want = tree_zoo.restated(("offset", "sphere_d4", dr.GROW, 0.0, 3, -1), lambda: dr.offset(tree("sphere_d4"), dr.GROW, 0.0, 3, -1, want_counts=True, surf=surf("sphere_d4")))
    assert np.array_equal(S0, want[0]) and np.array_equal(V0, want[1])


def test_blend_bytes_on_a_result_whose_arrays_grow(sb):
    pair, case = BIG
    S, V, counts = restated(pair, *case)
    level_sizes = [len(level) for level in pr.levels(S)]
    # the arrays start at max(1.5 x the operands together, 4096) nodes: this result makes them grow several times, and its last level
    # takes the first pass more than one sweep of its grid
    assert 8 * 4096 < len(S) < 400_000 and max(level_sizes) > 65536, (len(S), level_sizes)
    with upload(sb, pair[0]) as A, upload(sb, pair[1]) as B:
        st = check_call(sb, A, B, pair, case)
        assert st.depth_out == 7 and st.visited_b == 0 and st.visited_a == st.points         # (the leaf is its own cut cell: one record a search)
        # UNION(A, nothing) is Offset(A, 0), handle against handle
        res, got = A.Offset(0.0, 7, want_octdata=True)
        with res:
            assert_same_tree(got, S, V, "offset(leaf, 0) to depth 7")


def test_a_union_with_nothing_is_the_offset_by_zero_handle_against_handle(sb):
    with upload(sb, "sphere_d4") as A, upload(sb, "empty") as B:
        for k in (0.0, 0.07):
            r1, got = A.Blend(B, U, k, 4, want_octdata=True)
            r2, want = A.Offset(0.0, 4, want_octdata=True)
            with r1, r2:
                assert_same_tree(got, want.Structs, want.Values, f"union(sphere_d4, empty, {k}) against offset(sphere_d4, 0)")
                assert r1.Length == r2.Length > 1000
        # nothing with nothing: the root alone, no NaN in a byte
        for op in (U, I, SUB):
            res, got = B.Blend(B, op, 0.1, 4, want_octdata=True)
            with res:
                assert got.Length == 1 and (got.Values == 255).all()


def test_the_same_blend_twice_gives_the_same_bytes_and_the_same_work(sb):
    with upload(sb, "sphere_d4") as A, upload(sb, "carved") as B:
        x = A.Blend(B, U, 0.05, 3, want_octdata=True, want_stats=True)
        y = A.Blend(B, U, 0.05, 3, want_octdata=True, want_stats=True)
        with x[0], y[0]:
            assert x[1].Structs.tobytes() == y[1].Structs.tobytes() and x[1].Values.tobytes() == y[1].Values.tobytes()
            assert x[2].visited_a == y[2].visited_a > 0 and x[2].visited_b == y[2].visited_b > 0 and x[2].points == y[2].points


def test_blend_chains_with_render_prune_combine_and_measure(sb, oracle_mod):
    W, H = 64, 48
    pair, case = ("sphere_d4", "torus_d4"), (U, 0.03, 3, -1, -1)
    S, V, _ = restated(pair, *case)
    cam = make_camera("rotated", W, H)
    with upload(sb, pair[0]) as A, upload(sb, pair[1]) as B:
        before = A.Draw(cam, W, H), B.Draw(cam, W, H)
        with A.Blend(B, U, 0.03, 3) as res:
            assert_frames_identical(A.Draw(cam, W, H), before[0], "A after the call")
            assert_frames_identical(B.Draw(cam, W, H), before[1], "B after the call")
            ref, _ = oracle_mod.render(S, V, cam.State, W, H)
            assert_frames_identical(res.Draw(cam, W, H), ref, "the blended solid")
            m, want = res.Measure(), msr.measure(S, V)
            assert msr.same_bits(np.array(m.volume), np.array(want.volume)) and msr.same_bits(np.array(m.area), np.array(want.area))
            r2, got = res.Prune(0, None, want_octdata=True)
            with r2:
                assert_same_tree(got, *pr.prune(S, V, 0), "blend -> prune(0)")
            r2, got = res.Combine(A, cr.COMBINE_SUBTRACT, want_octdata=True)
            with r2:
                assert_same_tree(got, *cr.combine((S, V), tree(pair[0]), cr.COMBINE_SUBTRACT), "blend -> subtract A")
        with A.Morph(B, 0.5, 3) as res:
            Sm, Vm, _ = restated(pair, M, 0.5, 3, -1, -1)
            ref, _ = oracle_mod.render(Sm, Vm, cam.State, W, H)
            assert_frames_identical(res.Draw(cam, W, H), ref, "the morph")


def test_errors_are_status_codes(sb):
    L = sb._lib

    def call(a, b, opt, want_out=True):
        h = ctypes.c_void_p()
        rc = L.lib.sdfhip_scene_blend(a._h if a is not None else None, b._h if b is not None else None, ctypes.byref(opt) if opt is not None else None,
                                      ctypes.byref(h) if want_out else None, None, None)
        if h.value:
            L.lib.sdfhip_scene_free(h)
        assert rc == L.OK or not h.value, "*out is not null after a failure"
        return rc

    good = lambda **kw: sb.BlendOptions(**dict(dict(op=L.BLEND_UNION, amount=0.03, depth=3, level_a=-1, level_b=-1), **kw))
    W, H = 32, 24
    cam = make_camera("default", W, H)
    with upload(sb, "sphere_d4") as A, upload(sb, "torus_d4") as B, upload(sb, "empty") as E:
        before = A.Draw(cam, W, H), B.Draw(cam, W, H)
        assert call(A, B, good()) == L.OK and call(A, A, good(depth=0)) == L.OK and call(A, B, good(op=L.BLEND_MORPH, amount=1.0, level_a=12)) == L.OK
        assert call(A, B, good(amount=0.0)) == L.OK and call(A, B, good(op=L.BLEND_MORPH, amount=0.0)) == L.OK
        assert call(None, B, good()) == L.ERR_ARG and call(A, None, good()) == L.ERR_ARG and call(A, B, None) == L.ERR_ARG
        assert call(A, B, good(), want_out=False) == L.ERR_ARG
        for bad in (good(op=4), good(op=-1), good(amount=float("nan")), good(amount=float("inf")), good(amount=-0.01),
                    good(op=L.BLEND_INTERSECT, amount=-1.0), good(op=L.BLEND_SUBTRACT, amount=float("-inf")),
                    good(op=L.BLEND_MORPH, amount=-0.01), good(op=L.BLEND_MORPH, amount=1.01), good(op=L.BLEND_MORPH, amount=float("nan")),
                    good(depth=13), good(depth=-2), good(level_a=13), good(level_a=-2), good(level_b=13), good(level_b=-2)):
            assert call(A, B, bad) == L.ERR_ARG, (bad.op, bad.amount, bad.depth, bad.level_a, bad.level_b)
        small = good()
        small.size = 20
        assert call(A, B, small) == L.ERR_ARG

        class Newer(ctypes.Structure):
            _fields_ = sb.BlendOptions._fields_ + [("unknown", ctypes.c_int32)]
        newer = Newer()
        ctypes.memmove(ctypes.byref(newer), ctypes.byref(good()), 24)
        as_options = ctypes.cast(ctypes.pointer(newer), ctypes.POINTER(sb.BlendOptions)).contents
        newer.size, newer.unknown = 28, 3
        assert call(A, B, as_options) == L.ERR_ARG                      # an unknown field that is set
        newer.unknown = -1
        assert call(A, B, as_options) == L.OK                           # ... and one that says "default"
        # host_out alone is an output
        raw = L.COctData()
        assert L.lib.sdfhip_scene_blend(A._h, B._h, ctypes.byref(good()), None, ctypes.byref(raw), None) == L.OK
        assert raw.length == len(restated(("sphere_d4", "torus_d4"), U, 0.03, 3, -1, -1)[0])
        L.lib.sdfhip_octdata_free(ctypes.byref(raw))
        # the morph's refusal of an empty surface: either operand, and a surface that is empty at its level only -- the smooth
        # operations take the same operands
        morph = good(op=L.BLEND_MORPH, amount=0.5)
        assert call(A, E, morph) == L.ERR_ARG and b"empty surface" in L.lib.sdfhip_last_error()
        assert call(E, A, morph) == L.ERR_ARG and call(E, E, morph) == L.ERR_ARG
        assert len(surface("sphere_d4", 0)) == 0
        assert call(A, B, good(op=L.BLEND_MORPH, amount=0.5, level_a=0)) == L.ERR_ARG
        assert call(A, E, good()) == L.OK and call(E, A, good(op=L.BLEND_SUBTRACT)) == L.OK
        with pytest.raises(sb.SdfHipError) as e:
            A.Morph(E, 0.5)
        assert e.value.code == L.ERR_ARG
        # operands on different devices
        if sb.device_count() >= 2:
            with upload(sb, "torus_d4", device=1) as far:
                assert call(A, far, good()) == L.ERR_ARG
        assert_frames_identical(A.Draw(cam, W, H), before[0], "A after the refusals")
        assert_frames_identical(B.Draw(cam, W, H), before[1], "B after the refusals")
        # an operand the mesh refuses: an inconsistent tree, and one deeper than twelve levels, on either side
        S0, V0 = tree("sphere_d4")
        Sb = S0.copy()
        Sb[int(S0[0, 1]) + 3, 0] = int(S0[0, 1])
        for arrays in ((Sb, V0), tree("chain14")):
            with sb.Scene(sb.OctData(*arrays)) as bad:
                frame = bad.Draw(cam, W, H, sb.KERNEL_GENERIC)
                assert call(bad, A, good()) == L.ERR_BAD_TREE and call(A, bad, good()) == L.ERR_BAD_TREE and call(bad, bad, good()) == L.ERR_BAD_TREE
                assert_frames_identical(bad.Draw(cam, W, H, sb.KERNEL_GENERIC), frame, "the refused operand still renders")


def test_an_allocation_that_fails_is_nomem_and_leaves_the_operands():
    # in a fresh process of its own, so that neither the variable nor a failed call can reach the tests beside this one: every
    # allocation the blend reaches fails once (k = 0, 1, ... until a call gets through), each is SDFHIP_ERR_NOMEM with no handle, and
    # afterwards both operands render as before and a plain call gives the restatement's bytes (tests/blend_fault_child.py)
    S, V, _ = restated(("sphere_d4", "torus_d4"), U, 0.03, 3, -1, -1)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    child = os.path.join(REPO, "tests", "blend_fault_child.py")
    out = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    report = json.loads(out.stdout.strip().splitlines()[-1])
    # the two bitmaps, the counters, the two arrays, the blocks and the three scan buffers at the least
    assert report["codes_ok"] and 9 <= report["blend_failed"] < 64, report
    assert report["frames_unchanged"] and report["nodes_after"] == len(S), report
    assert report["structs_sha"] == sha(S) and report["values_sha"] == sha(V), report
    assert report["product_reads_no_variable"], report

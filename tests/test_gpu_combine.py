"""Combination on the GPU (sdfhip_scene_combine), both flavours of the library: the combined tree is the CPU restatement's
(tests/combine_restatement.py) byte for byte -- every op, both operand orders, with and without a depth cut -- its statistics are the
restatement's counts, its frames are the oracle's on the restated arrays, both inputs are untouched, combinations chain with prune
and edit as the restatements do, and the errors are status codes."""
import ctypes

import numpy as np
import pytest

import combine_restatement as cr
import edit_restatement as er
import prune_restatement as pr
from conftest import assert_frames_identical, make_camera
from test_gpu_prune import assert_same_tree, tree as prune_tree

pytestmark = pytest.mark.gpu

OP_NAMES = {cr.COMBINE_UNION: "union", cr.COMBINE_INTERSECT: "intersect", cr.COMBINE_SUBTRACT: "subtract"}
# two handles each: one node each (the same tree behind two handles), one node against a tree, a tree that collapses, different
# depths, edit order in (breadth first out); a == b, ONE handle as both operands, is SELF's
PAIRS = [("leaf", "leaf"), ("leaf", "sphere_d4"), ("nine", "sphere_d4"), ("sphere_d4", "torus_d6"), ("torus_edited", "off_d7")]
SELF = ["leaf", "torus_d6"]
CARVE = [(er.EDIT_CARVE, er.BRUSH_SPHERE, (0.6, 0.5, 0.45, 0.12))]


@pytest.fixture(scope="module", params=["product", "lab"])
def sb(request):
    import sdfbox_amd
    if request.param == "product":
        return sdfbox_amd
    import sdfbox_amd.lab
    return sdfbox_amd.lab.load()


_trees, _restated = {}, {}


def tree(name):
    """(structs, values) of the test trees (the same for both flavours), made once; test_gpu_prune's where it has them"""
    if name == "off_d7":
        if name not in _trees:
            import sdfbox_amd as base
            od = base.OctData.Generate(base._lib.SHAPE_SPHERE, [0.66, 0.5, 0.42, 0.17], 7)
            _trees[name] = (od.Structs, od.Values)
        return _trees[name]
    return prune_tree(name)


def restated(a, b, op, max_depth=-1):
    """(structs, values, counts) of the restatement, made once and left unchanged"""
    key = (a, b, op, max_depth)
    if key not in _restated:
        _restated[key] = cr.combine(tree(a), tree(b), op, max_depth, want_counts=True)
    return _restated[key]


def upload(sb, name):
    return sb.Scene(sb.OctData(*tree(name)))


def check_case(sa, sb_, a, b, op, max_depth):
    S, V, counts = restated(a, b, op, max_depth)
    res, got, st = sa.Combine(sb_, op, None if max_depth < 0 else max_depth, want_octdata=True, want_stats=True)
    with res:
        what = f"{OP_NAMES[op]}({a}, {b}) max_depth={max_depth}"
        assert_same_tree(got, S, V, what)
        assert (st.nodes_a, st.nodes_b, st.nodes_out) == (len(tree(a)[0]), len(tree(b)[0]), len(S)), what
        assert (st.nodes_shared, st.depth_out) == (counts["nodes_shared"], counts["depth_out"]) and st.depth_out == er.tree_depth(S), what
        assert res.Length == len(S) and res.depth == st.depth_out and res.stack_kernel_ok, what


def cuts(a, b):
    """no cut, the root alone, one level inside the shallower operand"""
    return sorted({-1, 0, max(min(er.tree_depth(tree(a)[0]), er.tree_depth(tree(b)[0])) - 1, 0)})


@pytest.mark.parametrize("pair", PAIRS, ids="-".join)
def test_combined_bytes_are_the_restatements(sb, pair):
    a, b = pair
    with upload(sb, a) as sa, upload(sb, b) as sb_:
        for op in cr.OPS:
            for max_depth in cuts(a, b):
                check_case(sa, sb_, a, b, op, max_depth)
                check_case(sb_, sa, b, a, op, max_depth)


@pytest.mark.parametrize("name", SELF)
def test_a_scene_combined_with_itself(sb, name):
    with upload(sb, name) as scene:                 # a == b: one handle, one lock
        for op in cr.OPS:
            for max_depth in cuts(name, name):
                check_case(scene, scene, name, name, op, max_depth)


def test_the_pairs_are_what_they_are_for():
    assert len(tree("nine")[0]) == 9 and len(tree("leaf")[0]) == 1
    assert er.tree_depth(tree("sphere_d4")[0]) == 4 and er.tree_depth(tree("torus_d6")[0]) == 6 and er.tree_depth(tree("off_d7")[0]) == 7
    S = restated("torus_edited", "off_d7", cr.COMBINE_UNION)[0]
    level_sizes = [len(level) for level in pr.levels(S)]
    # level lists that end inside a wave of the first pass (64 items) and inside a workgroup of the second (eight lanes per item: 32)
    assert any(m > 64 and m % 64 for m in level_sizes) and any(m > 32 and m % 32 for m in level_sizes), level_sizes
    assert not np.array_equal(tree("torus_edited")[0][:, 1] >= 0, cr.combine(tree("torus_edited"), tree("leaf"), cr.COMBINE_UNION)[0][:, 1] >= 0), \
        "edit order in is not breadth first out"


@pytest.mark.parametrize("a, b", [("gyroid_d8", "torus_d6"), ("torus_d6", "gyroid_d8")], ids=["gyroid_d8-torus_d6", "torus_d6-gyroid_d8"])
@pytest.mark.parametrize("op", cr.OPS, ids=OP_NAMES.get)
def test_combined_bytes_on_a_result_past_the_scans_chunk(sb, op, a, b):
    S = restated(a, b, op)[0]
    level_sizes = [len(level) for level in pr.levels(S)]
    # (a workgroup of the first pass takes 256 items; the second pass's, eight lanes per item, are held by test_the_pairs_are_...)
    assert len(S) > 4 * 32768 and any(m > 256 and m % 256 for m in level_sizes), "past the scan's chunk, a level list that ends inside a workgroup"
    with upload(sb, a) as sa, upload(sb, b) as sb_:
        for max_depth in cuts(a, b):
            check_case(sa, sb_, a, b, op, max_depth)


@pytest.mark.parametrize("op", cr.OPS, ids=OP_NAMES.get)
def test_combined_frames_are_the_oracles_and_the_inputs_are_untouched(sb, oracle_mod, op):
    W, H = 64, 48
    a, b = "torus_edited", "off_d7"
    S, V, _ = restated(a, b, op)
    cams = [make_camera(name, W, H) for name in ("default", "rotated")]
    with upload(sb, a) as sa, upload(sb, b) as sb_:
        before = [(sa.Draw(cam, W, H), sb_.Draw(cam, W, H)) for cam in cams]
        res = sa.Combine(sb_, op)
        for cam, (fa, fb) in zip(cams, before):
            assert_frames_identical(sa.Draw(cam, W, H), fa, f"{OP_NAMES[op]}: operand a after the call")
            assert_frames_identical(sb_.Draw(cam, W, H), fb, f"{OP_NAMES[op]}: operand b after the call")
    # (both inputs are freed: the result stands alone)
    with res:
        for cam in cams:
            ref, _ = oracle_mod.render(S, V, cam.State, W, H)
            for flags in (sb.KERNEL_AUTO, sb.KERNEL_GENERIC):
                assert_frames_identical(res.Draw(cam, W, H, flags), ref, f"{OP_NAMES[op]} flags {flags}")


def test_a_combination_beside_frames_in_flight(sb):
    import torch
    W, H = 64, 48
    cam = make_camera("rotated", W, H)
    with upload(sb, "torus_edited") as sa, upload(sb, "off_d7") as sb_:
        before = sa.Draw(cam, W, H), sb_.Draw(cam, W, H)
        frames = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(6)]
        torch.cuda.synchronize()
        s_frames = torch.cuda.Stream()
        results = []
        for k, buf in enumerate(frames):
            (sa, sb_)[k & 1].DrawDevice(cam, W, H, buf.data_ptr(), stream=s_frames.cuda_stream)
            results.append(sa.Combine(sb_, cr.COMBINE_SUBTRACT, want_octdata=True))
        torch.cuda.synchronize()
        for k, buf in enumerate(frames):
            assert_frames_identical(buf.cpu().numpy(), before[k & 1], "a frame in flight beside a combination")
        S, V, _ = restated("torus_edited", "off_d7", cr.COMBINE_SUBTRACT)
        for res, got in results:
            assert_same_tree(got, S, V, "one of several combinations of the same inputs")
            res.close()


def test_chains_are_the_restatements_chained(sb):
    a, b = "torus_d6", "off_d7"
    union = restated(a, b, cr.COMBINE_UNION)[:2]
    pruned = pr.prune(*union, 0)
    edited = er.edit(*union, CARVE, 7)
    carved_first = er.edit(*tree(a), CARVE, 7)
    then_cut = cr.combine(carved_first, tree(b), cr.COMBINE_SUBTRACT)
    assert len(pruned[0]) < len(union[0]) and len(edited[0]) > len(union[0]) and len(carved_first[0]) > len(tree(a)[0])
    with upload(sb, a) as sa, upload(sb, b) as sb_:
        with sa.Combine(sb_, cr.COMBINE_UNION) as u:
            s1, got, _ = u.Prune(0, None, want_octdata=True, want_stats=True)
            with s1:
                assert_same_tree(got, *pruned, "combine -> prune(0)")
            s2, got, _ = u.Edit(CARVE, max_depth=7, want_octdata=True, want_stats=True)
            with s2:
                assert_same_tree(got, *edited, "combine -> edit")
        with sa.Edit(CARVE, max_depth=7) as e:
            s3, got = e.Combine(sb_, cr.COMBINE_SUBTRACT, want_octdata=True)
            with s3:
                assert_same_tree(got, *then_cut, "edit -> combine")


def test_errors_are_status_codes(sb):
    L = sb._lib

    def call(a, b, op=cr.COMBINE_UNION, opt=None):
        h = ctypes.c_void_p()
        rc = L.lib.sdfhip_scene_combine(a._h if a is not None else None, b._h if b is not None else None, op,
                                        ctypes.byref(opt) if opt is not None else None, ctypes.byref(h), None, None)
        if h.value:
            L.lib.sdfhip_scene_free(h)
        assert rc == L.OK or not h.value, "*out is not null after a failure"
        return rc

    with upload(sb, "sphere_d4") as sa, upload(sb, "torus_d6") as sb_:
        assert call(sa, sb_) == L.OK
        assert call(sa, sb_, cr.COMBINE_SUBTRACT, sb.CombineOptions(12)) == L.OK
        assert call(sa, None) == L.ERR_ARG and call(None, sb_) == L.ERR_ARG
        assert L.lib.sdfhip_scene_combine(sa._h, sb_._h, 0, None, None, None, None) == L.ERR_ARG
        for op in (-1, 3, 7):
            assert call(sa, sb_, op) == L.ERR_ARG, op
        for max_depth in (13, -2):
            assert call(sa, sb_, opt=sb.CombineOptions(max_depth)) == L.ERR_ARG, max_depth

        class Newer(ctypes.Structure):
            _fields_ = [("size", ctypes.c_uint32), ("max_depth", ctypes.c_int32), ("unknown", ctypes.c_int32)]
        as_options = lambda o: ctypes.cast(ctypes.pointer(o), ctypes.POINTER(sb.CombineOptions)).contents
        assert call(sa, sb_, opt=as_options(Newer(12, -1, 3))) == L.ERR_ARG          # an unknown field that is set
        assert call(sa, sb_, opt=as_options(Newer(12, -1, -1))) == L.OK              # ... and one that says "default"
        small = sb.CombineOptions(None)
        small.size = 4
        assert call(sa, sb_, opt=small) == L.ERR_ARG
        # an inconsistent tree (a child whose parent field points elsewhere) uploads, but cannot be combined, as either operand
        S0, V0 = tree("sphere_d4")
        S = S0.copy()
        S[int(S[0, 1]) + 3, 0] = int(S[0, 1])
        bad_tree = sb.OctData(S, V0)
        assert bad_tree.validate()[1] is False
        with sb.Scene(bad_tree) as bad:
            assert not bad.stack_kernel_ok
            assert call(bad, sb_) == L.ERR_BAD_TREE and call(sa, bad) == L.ERR_BAD_TREE and call(bad, bad) == L.ERR_BAD_TREE


@pytest.fixture(scope="module")
def lab():
    """the laboratory flavour alone: the product reads no SDFHIP_COMBINE_FAIL_ALLOC"""
    import sdfbox_amd.lab
    return sdfbox_amd.lab.load()


def test_an_allocation_that_fails_is_nomem_and_leaves_the_inputs(lab, monkeypatch):
    sb = lab
    L = sb._lib
    assert L.EXPERIMENTS
    W, H = 64, 48
    cam = make_camera("default", W, H)
    S, V, _ = restated("sphere_d4", "torus_d6", cr.COMBINE_INTERSECT)
    with upload(sb, "sphere_d4") as sa, upload(sb, "torus_d6") as sb_:
        before = sa.Draw(cam, W, H), sb_.Draw(cam, W, H)
        failed = 0
        for k in range(64):
            monkeypatch.setenv("SDFHIP_COMBINE_FAIL_ALLOC", str(k))
            h = ctypes.c_void_p()
            rc = L.lib.sdfhip_scene_combine(sa._h, sb_._h, cr.COMBINE_INTERSECT, None, ctypes.byref(h), None, None)
            if rc == L.OK:
                L.lib.sdfhip_scene_free(h)
                break
            assert rc == L.ERR_NOMEM and not h.value, k
            failed += 1
        monkeypatch.delenv("SDFHIP_COMBINE_FAIL_ALLOC")
        assert 0 < failed < 64, "the call has device allocations, and each of them can fail"
        assert_frames_identical(sa.Draw(cam, W, H), before[0], "operand a after failed combinations")
        assert_frames_identical(sb_.Draw(cam, W, H), before[1], "operand b after failed combinations")
        res, got = sa.Combine(sb_, cr.COMBINE_INTERSECT, want_octdata=True)
        with res:
            assert_same_tree(got, S, V, "a plain call after the failed ones")

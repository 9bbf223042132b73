"""The measure on the GPU (sdfhip_scene_measure), both flavours of the library: every double and every count is the CPU restatement's
(tests/measure_restatement.py, held by tests/test_measure.py to the mesh restatement, exact cases and closed forms) byte for byte -- on
one-node trees, analytic trees, a carved tree with cells of two depths, a tree in edit order and one with more than 1024 partial sums,
at levels from the root to deeper than the tree; a level's measure is the pruned tree's; frames in flight are left alone; a measured
scene is fitted and placed; the errors are status codes and a failed allocation leaks nothing."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import edit_restatement as er
import measure_restatement as ms
import mesh_restatement as mr
import prune_restatement as pr
from conftest import REPO, assert_frames_identical, make_camera
from test_gpu_combine import tree as combine_tree

pytestmark = pytest.mark.gpu

ONE = np.array([[-1, -1]], dtype=np.int32)
ONE_NODE = {"empty1": [255] * 8, "full1": [0] * 8, "plane1": [0, 255] * 4}       # nothing inside; everything; the plane x = 0.25
SMALL = ["empty1", "full1", "plane1", "nine", "sphere_d4", "torus_d6", "carved_d7", "torus_edited"]
# more than 1024 partials: the fold runs more than one round.  (The restatement of the 6 M-node gyroid_d8 of test_gpu_combine.py takes
# 15 s here, 4 of them the walk; this depth-9 sphere is the generated tree past 1 048 576 nodes whose restatement stays within seconds.)
BIG = "sphere_d9"


@pytest.fixture(scope="module", params=["product", "lab"])
def sb(request):
    import sdfbox_amd
    if request.param == "product":
        return sdfbox_amd
    import sdfbox_amd.lab
    return sdfbox_amd.lab.load()


_trees, _walked, _restated = {}, {}, {}


def tree(name):
    """(structs, values) of the test trees (the same for both flavours), made once"""
    if name not in _trees:
        if name in ONE_NODE:
            _trees[name] = (ONE, np.array([ONE_NODE[name]], dtype=np.uint8))
        elif name == BIG:
            import sdfbox_amd as base
            od = base.OctData.Generate(base._lib.SHAPE_SPHERE, [0.66, 0.5, 0.42, 0.2], 9)
            _trees[name] = (od.Structs, od.Values)
        elif name == "carved_d7":
            from test_gpu_mesh import tree as mesh_tree
            od = mesh_tree(name)
            _trees[name] = (od.Structs, od.Values)
        else:
            _trees[name] = combine_tree(name)
    return _trees[name]


def levels_of(name):
    """the leaves, the root, one level inside the tree, the tree's own depth, one deeper"""
    depth = er.tree_depth(tree(name)[0])
    return sorted({-1, 0, depth // 2, depth, min(depth + 1, 12)})


def restated(name, level=-1):
    """the restatement's Measured, made once and left unchanged"""
    if (name, level) not in _restated:
        S, V = tree(name)
        if name not in _walked:
            _walked[name] = mr.walk(S)
        _restated[name, level] = ms.measure(S, V, level, walked=_walked[name])
    return _restated[name, level]


def upload(sb, name):
    return sb.Scene(sb.OctData(*tree(name)))


def doubles(m):
    return np.array([m.volume, m.area, *m.moment1, *m.moment2, *m.bounds_min, *m.bounds_max], dtype=np.float64)


def counts(m):
    return np.array([m.cells, m.cells_cut, m.cells_inside, *m.cells_at_depth], dtype=np.int64)


def assert_same_measure(got, want, what):
    g, w = doubles(got), want.doubles()
    bad = np.nonzero(g.view(np.uint64) != w.view(np.uint64))[0]
    names = list(ms.SUMS) + ["min x", "min y", "min z", "max x", "max y", "max z"]
    assert not len(bad), f"{what}: " + "; ".join(f"{names[k]} {g[k]!r} against {w[k]!r}" for k in bad[:6])
    assert np.array_equal(counts(got), want.counts()), (what, counts(got).tolist(), want.counts().tolist())
    assert (got.nodes, got.depth) == (want.nodes, want.depth), what


@pytest.mark.parametrize("name", SMALL)
def test_every_double_and_count_is_the_restatements(sb, name):
    with upload(sb, name) as scene:
        assert scene.stack_kernel_ok
        for level in levels_of(name):
            m = scene.Measure(level)
            assert_same_measure(m, restated(name, level), f"measure({name}, level {level})")
            assert m.kernel_ms > 0 and m.total_ms > 0
        assert_same_measure(scene.Measure(), restated(name), f"measure({name}) again")


def test_the_trees_are_what_they_are_for():
    assert [len(tree(n)[0]) for n in ("empty1", "nine", "torus_d6")] == [1, 9, 38857]
    assert 38857 % 1024 % 64, "the last chunk ends inside a wave"
    S, V = tree("carved_d7")
    depth, _ = mr.walk(S)
    cut = (S[:, 1] < 0) & (V.min(1) <= 63) & (V.max(1) > 63)
    assert set(np.unique(depth[cut])) >= {6, 7}, "cut cells of two depths"
    S = tree("torus_edited")[0]
    depth, _ = mr.walk(S)
    assert (np.diff(depth.astype(np.int64)) < 0).any() and er.tree_depth(S) == 8, "edit order: depth is not monotone in the index"
    assert len(levels_of("torus_edited")) == 5 and levels_of("torus_d6") == [-1, 0, 3, 6, 7]
    full, empty, plane = (restated(n) for n in ("full1", "empty1", "plane1"))
    assert (full.volume, full.cells_inside, empty.volume, empty.cells_inside, plane.cells_cut) == (1.0, 1, 0.0, 0, 1)
    assert np.isposinf(empty.bounds_min).all() and np.isneginf(empty.bounds_max).all()


def test_a_tree_whose_partials_fold_in_more_than_one_round(sb):
    S, V = tree(BIG)
    assert len(S) > 1024 * 1024, "more than 1024 partials of 1024 nodes: the fold runs more than one round"
    want = restated(BIG)
    assert want.cells_cut > 100_000 and want.cells_inside > 100_000
    with upload(sb, BIG) as scene:
        assert_same_measure(scene.Measure(), want, f"measure({BIG})")


# (levels at which a prune at tolerance 0 removes what lies below the level and nothing else: deeper, these analytic trees hold blocks
# whose bytes are exactly their parent's interpolation, the prune collapses them too, and the cell sets differ)
@pytest.mark.parametrize("name, levels", [("sphere_d4", (2, 3)), ("torus_d6", (2, 3))])
def test_a_levels_measure_is_the_pruned_trees(sb, name, levels):
    S, V = tree(name)
    depth, _ = mr.walk(S)
    with upload(sb, name) as scene:
        for L in levels:
            assert len(pr.prune(S, V, 0, L)[0]) == int((depth <= L).sum())
            at_level = scene.Measure(L)
            with scene.Prune(0, L) as pruned:
                leaves = pruned.Measure()
            assert np.array_equal(counts(at_level), counts(leaves)), (name, L)
            a, b = doubles(at_level), doubles(leaves)
            assert np.array_equal(a[11:].view(np.uint64), b[11:].view(np.uint64)), "the bounds are exact, whatever the order"
            assert (np.abs(a[:11] - b[:11]) <= 1e-12 * np.abs(b[:11])).all(), (name, L, a, b)      # the node order differs
            assert at_level.volume > 0


def test_a_measure_beside_frames_in_flight(sb):
    import torch
    W, H = 64, 48
    cam = make_camera("rotated", W, H)
    name = "torus_edited"
    with upload(sb, name) as scene:
        before = scene.Draw(cam, W, H)
        frames = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(6)]
        torch.cuda.synchronize()
        s_frames = torch.cuda.Stream()
        results = []
        for buf in frames:
            scene.DrawDevice(cam, W, H, buf.data_ptr(), stream=s_frames.cuda_stream)
            results.append(scene.Measure())
        torch.cuda.synchronize()
        for buf in frames:
            assert_frames_identical(buf.cpu().numpy(), before, "a frame in flight beside a measure")
        for m in results:
            assert_same_measure(m, restated(name), "a measure beside frames in flight")
        assert_frames_identical(scene.Draw(cam, W, H), before, "the scene after the measures")


def test_measure_fit_place_measure(sb):
    to, size = (0.4, 0.5, 0.55), 0.3
    with upload(sb, "off_d7") as scene:
        m = scene.Measure()
        assert abs(m.centroid[0] - 0.66) < 0.01 and abs(m.centroid[2] - 0.42) < 0.01          # off centre, as built
        R, s, t = sb.placement_fit(m, size=size, to=to)
        with scene.Place(R, s, t) as placed:
            leaf = 2.0 ** -placed.depth
            assert placed.depth == 7
            m2 = placed.Measure()
    lo, hi = np.array(m2.bounds_min[:]), np.array(m2.bounds_max[:])
    assert np.abs((lo + hi) / 2 - np.array(to)).max() <= leaf, ((lo + hi) / 2, to)
    assert abs((hi - lo).max() - size) <= 2 * leaf, ((hi - lo).max(), size)
    assert np.abs(np.array(m2.centroid) - np.array(to)).max() <= leaf


def test_errors_are_status_codes(sb):
    L = sb._lib

    def call(scene, opt, want_out=True):
        out = L.Measure()
        ctypes.memset(ctypes.byref(out), 0xFF, ctypes.sizeof(out))
        rc = L.lib.sdfhip_scene_measure(scene._h if scene is not None else None, ctypes.byref(opt) if opt is not None else None,
                                        ctypes.byref(out) if want_out else None)
        if rc != L.OK and want_out:
            assert bytes(out) == bytes(ctypes.sizeof(out)), "*out is zeroed on failure"
        return rc, out

    with upload(sb, "sphere_d4") as scene:
        rc, out = call(scene, None)                                             # no options: level -1
        assert rc == L.OK
        assert_same_measure(out, restated("sphere_d4"), "opt == NULL")
        assert call(scene, sb.MeasureOptions(12))[0] == L.OK and call(scene, sb.MeasureOptions(0))[0] == L.OK
        assert call(None, sb.MeasureOptions())[0] == L.ERR_ARG and call(scene, sb.MeasureOptions(), want_out=False)[0] == L.ERR_ARG
        assert call(scene, sb.MeasureOptions(13))[0] == L.ERR_ARG and call(scene, sb.MeasureOptions(-2))[0] == L.ERR_ARG
        small = sb.MeasureOptions()
        small.size = 4
        assert call(scene, small)[0] == L.ERR_ARG

        class Newer(ctypes.Structure):
            _fields_ = sb.MeasureOptions._fields_ + [("unknown", ctypes.c_int32)]
        newer = Newer(12, -1, 3)
        as_options = ctypes.cast(ctypes.pointer(newer), ctypes.POINTER(sb.MeasureOptions)).contents
        assert call(scene, as_options)[0] == L.ERR_ARG                          # an unknown field that is set
        newer.unknown = -1
        assert call(scene, as_options)[0] == L.OK                               # ... and one that says "default"
        default = sb.MeasureOptions(5)
        L.lib.sdfhip_measure_options_default(ctypes.byref(default))
        assert (default.size, default.level) == (8, -1)
    # a tree the upload calls inconsistent is refused
    S0, V0 = tree("sphere_d4")
    Sb = S0.copy()
    Sb[int(S0[0, 1]) + 3, 0] = int(S0[0, 1])
    with sb.Scene(sb.OctData(Sb, V0)) as bad:
        assert not bad.stack_kernel_ok
        assert call(bad, sb.MeasureOptions())[0] == L.ERR_BAD_TREE
        with pytest.raises(sb.SdfHipError) as e:
            bad.Measure()
        assert e.value.code == L.ERR_BAD_TREE


def test_an_allocation_that_fails_is_nomem_and_leaks_nothing():
    # in a fresh process of its own, so that neither the variable nor a failed call can reach the tests beside this one: every
    # allocation the call reaches fails once (k = 0, 1, ... until a call gets through), each is SDFHIP_ERR_NOMEM with *out zeroed,
    # and a plain call afterwards gives the restatement's bytes (tests/measure_fault_child.py)
    child = os.path.join(REPO, "tests", "measure_fault_child.py")
    out = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    report = json.loads(out.stdout.strip().splitlines()[-1])
    assert report["codes_ok"] and 1 <= report["failed"] < 8, report
    want = restated("torus_d6")
    assert report["doubles"] == want.doubles().tobytes().hex() and report["counts"] == want.counts().tolist(), report
    assert report["frame_unchanged"] and report["product_reads_no_variable"], report

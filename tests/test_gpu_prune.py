"""Pruning on the GPU (sdfhip_scene_prune), both flavours of the library: the pruned tree is the CPU restatement's
(tests/prune_restatement.py) byte for byte, its frames are the oracle's on the restated arrays, the input handle is untouched, a
prune after an edit and an edit after a prune chain as the restatements do, and the errors are status codes."""
import ctypes

import numpy as np
import pytest

import edit_restatement as er
import prune_restatement as pr
from conftest import CAMERAS, assert_frames_identical, make_camera

pytestmark = pytest.mark.gpu

TOLERANCES = (0, 1, 8, 255)
SMALL = ["leaf", "nine", "sphere_d4", "torus_d6", "torus_edited", "carved_away"]


@pytest.fixture(scope="module", params=["product", "lab"])
def sb(request):
    import sdfbox_amd
    if request.param == "product":
        return sdfbox_amd
    import sdfbox_amd.lab
    return sdfbox_amd.lab.load()


_trees, _restated = {}, {}


def tree(name):
    """(structs, values) of the test trees (the same for both flavours), made once"""
    if name not in _trees:
        import sdfbox_amd as base
        arrays = lambda od: (od.Structs, od.Values)
        root = (np.array([[-1, -1]], dtype=np.int32), np.full((1, 8), 255, dtype=np.uint8))
        if name == "leaf":
            _trees[name] = root
        elif name == "nine":                  # the root split once, its children's bytes the inherited ones: collapses to one node
            _trees[name] = pr.split_leaves(np.array([[-1, -1]], dtype=np.int32), np.array([[60, 80, 90, 120, 70, 200, 40, 255]], dtype=np.uint8))
        elif name == "sphere_d4":
            _trees[name] = arrays(base.sphere_d4())
        elif name == "torus_d6":
            _trees[name] = arrays(base.torus_d6())
        elif name == "gyroid_d8":             # the analytic builder's order; past the scan's chunk and the workgroup
            _trees[name] = arrays(base.dragon_standin(8, nthreads=16))
        elif name == "torus_edited":          # edit order: blocks appended breadth-first behind the original nodes
            edits = [(er.EDIT_CARVE, er.BRUSH_SPHERE, (0.84, 0.5, 0.5, 0.07)), (er.EDIT_ADD, er.BRUSH_BOX, (0.5, 0.6, 0.2, 0.1, 0.04, 0.08)),
                     (er.EDIT_CARVE, er.BRUSH_BOX, (0.3, 0.5, 0.5, 0.05, 0.2, 0.05))]
            _trees[name] = er.edit(*tree("torus_d6"), edits, 8)
        elif name == "carved_away":           # a four-level cascade: 13 385 nodes -> 9
            T = er.edit(*root, [(er.EDIT_ADD, er.BRUSH_SPHERE, (0.5, 0.5, 0.5, 0.3))], 5)
            _trees[name] = er.edit(*T, [(er.EDIT_CARVE, er.BRUSH_SPHERE, (0.5, 0.5, 0.5, 1.2))], 5)
        elif name == "builder_d10":           # as tests/test_gpu_edit.py builds it, after one carve at the surface
            od = base.OctData.SdfGen(base.knot_point_cloud(100_000, seed=3), 10)
            c, _ = er.deepest_leaf_centres(od.Structs)
            _trees[name] = er.edit(od.Structs, od.Values, [(er.EDIT_CARVE, er.BRUSH_SPHERE, (*c[len(c) // 2], 0.06))], -1, region=True)
    return _trees[name]


def restated(name, tolerance, max_depth):
    key = (name, tolerance, max_depth)
    if key not in _restated:
        _restated[key] = pr.prune(*tree(name), tolerance, max_depth)
    return _restated[key]


def upload(sb, name):
    return sb.Scene(sb.OctData(*tree(name)))


def gpu_prune(scene, tolerance=0, max_depth=None):
    return scene.Prune(tolerance, max_depth, want_octdata=True, want_stats=True)


def assert_same_tree(od, S, V, what):
    assert od.Length == len(S), f"{what}: {od.Length} nodes, the restatement {len(S)}"
    bad_s = np.nonzero((od.Structs != S).any(1))[0]
    bad_v = np.nonzero((od.Values != V).any(1))[0]
    assert not len(bad_s) and not len(bad_v), (what, bad_s[:5].tolist(), bad_v[:5].tolist(),
                                                [(od.Structs[i].tolist(), S[i].tolist()) for i in bad_s[:3]])


def check_case(scene, name, tolerance, max_depth):
    n_in = len(tree(name)[0])
    S, V = restated(name, tolerance, max_depth)
    res, got, st = gpu_prune(scene, tolerance, None if max_depth < 0 else max_depth)
    with res:
        what = f"{name} tolerance={tolerance} max_depth={max_depth}"
        assert_same_tree(got, S, V, what)
        assert (st.nodes_in, st.nodes_out, st.blocks_removed) == (n_in, len(S), (n_in - len(S)) // 8), what
        assert st.depth_out == er.tree_depth(S), what
        assert res.Length == len(S) and res.depth == st.depth_out and res.stack_kernel_ok, what


@pytest.mark.parametrize("name", SMALL)
def test_pruned_bytes_are_the_restatements(sb, name):
    depth = er.tree_depth(tree(name)[0])
    with upload(sb, name) as scene:
        for tolerance in TOLERANCES:
            for max_depth in sorted({-1, 0, max(depth - 1, 0)}):
                check_case(scene, name, tolerance, max_depth)


def test_the_small_trees_are_what_they_are_for():
    assert len(tree("nine")[0]) == 9 and len(restated("nine", 0, -1)[0]) == 1
    assert len(tree("carved_away")[0]) == 13385 and len(restated("carved_away", 0, -1)[0]) == 9
    S = tree("torus_edited")[0]
    assert len(S) > len(tree("torus_d6")[0]) and er.tree_depth(S) == 8
    blocks = [int((S[level, 1] >= 0).sum()) for level in pr.levels(S)]
    assert sum(1 for b in blocks if b > 8 and b % 8) >= 3, "level lists that end inside a wave's eight blocks"


@pytest.mark.parametrize("tolerance", TOLERANCES)
def test_pruned_bytes_on_a_tree_past_the_scans_chunk(sb, tolerance):
    S0 = tree("gyroid_d8")[0]
    depth = er.tree_depth(S0)
    blocks = [int((S0[level, 1] >= 0).sum()) for level in pr.levels(S0)]
    assert len(S0) > 4 * 32768 and any(b > 32 and b % 32 for b in blocks), "past the scan's chunk, a level list that ends inside a workgroup"
    with upload(sb, "gyroid_d8") as scene:
        for max_depth in (-1, 0, depth - 1):
            check_case(scene, "gyroid_d8", tolerance, max_depth)


@pytest.mark.parametrize("tolerance", [0, 1])
def test_a_tree_in_the_millions_of_nodes(sb, tolerance):
    assert len(tree("builder_d10")[0]) > 1_000_000
    with upload(sb, "builder_d10") as scene:
        check_case(scene, "builder_d10", tolerance, -1)


@pytest.mark.parametrize("name", ["sphere_d4", "torus_edited"])
def test_pruned_frames_are_the_oracles(sb, oracle_mod, name):
    W = H = 256
    S, V = restated(name, 1, -1)
    assert len(S) < len(tree(name)[0])
    with upload(sb, name) as scene:
        res, got, _ = gpu_prune(scene, 1)
        with res, sb.Scene(got) as fresh:
            assert_same_tree(got, S, V, name)
            for cam_name in CAMERAS:
                cam = make_camera(cam_name, W, H)
                ref, cnt = oracle_mod.render(S, V, cam.State, W, H)
                for flags in (sb.KERNEL_AUTO, sb.KERNEL_GENERIC):
                    img, st = res.Draw(cam, W, H, flags | sb.FLAG_COUNT, want_stats=True)
                    assert_frames_identical(img, ref, f"{name} {cam_name} flags {flags}")
                    assert (st.n_nodes, st.n_samples, st.n_steps, st.n_shadow_rays) == tuple(int(c) for c in cnt)
                    assert_frames_identical(fresh.Draw(cam, W, H, flags), img, f"{name} {cam_name}: the uploaded host_out")


def test_the_input_handle_is_untouched(sb):
    import torch
    W = H = 128
    cam = make_camera("rotated", W, H)
    scene = upload(sb, "torus_edited")
    before = scene.Draw(cam, W, H)
    # a prune issued while frames of the input are enqueued on another stream
    frames = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(6)]
    torch.cuda.synchronize()
    s_frames = torch.cuda.Stream()
    results = []
    for b in frames:
        scene.DrawDevice(cam, W, H, b.data_ptr(), stream=s_frames.cuda_stream)
        results.append(scene.Prune(8, 5))
    torch.cuda.synchronize()
    for b in frames:
        assert_frames_identical(b.cpu().numpy(), before, "a frame in flight beside a prune")
    pruned = results[0].Draw(cam, W, H)
    assert not np.array_equal(pruned, before)
    for r in results[1:]:
        assert_frames_identical(r.Draw(cam, W, H), pruned, "two prunes of one input")
        r.close()
    res = results[0]
    assert_frames_identical(scene.Draw(cam, W, H), before, "the input after a prune")
    scene.close()                                   # either handle may go first
    assert_frames_identical(res.Draw(cam, W, H), pruned, "the result after the input was freed")
    res2 = res.Prune(8, 5)
    res.close()
    assert_frames_identical(res2.Draw(cam, W, H), pruned, "a prune of the result after its input was freed")
    res2.close()


def test_edit_prune_edit_is_the_restatements_chained(sb):
    carve = [(er.EDIT_CARVE, er.BRUSH_SPHERE, (0.5, 0.5, 0.5, 0.45))]
    add = [(er.EDIT_ADD, er.BRUSH_SPHERE, (0.6, 0.5, 0.5, 0.2)), (er.EDIT_CARVE, er.BRUSH_BOX, (0.6, 0.5, 0.5, 0.05, 0.3, 0.05))]
    a = er.edit(*tree("torus_d6"), carve, 7)
    b = pr.prune(*a, 0)
    c = er.edit(*b, add, 7)
    d = pr.prune(*c, 1, 6)
    assert len(b[0]) < len(a[0]) and len(c[0]) > len(b[0]) and len(d[0]) < len(c[0])
    with upload(sb, "torus_d6") as scene, scene.Edit(carve, max_depth=7) as s1:
        s2, got_b, _ = gpu_prune(s1, 0)
        with s2:
            assert_same_tree(got_b, *b, "edit -> prune")
            s3, got_c, _ = s2.Edit(add, max_depth=7, want_octdata=True, want_stats=True)
            with s3:
                assert_same_tree(got_c, *c, "edit -> prune -> edit")
                s4, got_d, _ = gpu_prune(s3, 1, 6)
                with s4:
                    assert_same_tree(got_d, *d, "edit -> prune -> edit -> prune")


@pytest.mark.parametrize("name", ["torus_edited", "gyroid_d8"])
def test_prune_is_idempotent_and_deterministic(sb, name):
    with upload(sb, name) as scene:
        r1, a, _ = gpu_prune(scene, 1)
        r2, b, _ = gpu_prune(scene, 1)
        with r1, r2:
            assert np.array_equal(a.Structs, b.Structs) and np.array_equal(a.Values, b.Values), "two runs differ"
            r3, c, st = gpu_prune(r1, 1)
            with r3:
                assert np.array_equal(a.Structs, c.Structs) and np.array_equal(a.Values, c.Values), "prune of prune is not prune"
                assert st.blocks_removed == 0 and st.nodes_out == st.nodes_in == a.Length


def test_errors_are_status_codes(sb, monkeypatch):
    L = sb._lib

    def call(scene, opt, out=True):
        h = ctypes.c_void_p()
        rc = L.lib.sdfhip_scene_prune(scene._h if scene is not None else None, ctypes.byref(opt) if opt is not None else None,
                                      ctypes.byref(h) if out else None, None, None)
        if h.value:
            L.lib.sdfhip_scene_free(h)
        assert rc == L.OK or not h.value
        return rc

    with upload(sb, "sphere_d4") as scene:
        assert call(scene, None) == L.OK
        assert call(scene, sb.PruneOptions(0, None)) == L.OK
        assert call(scene, sb.PruneOptions(255, 12)) == L.OK
        assert call(None, None) == L.ERR_ARG
        assert call(scene, None, out=False) == L.ERR_ARG
        for tolerance, max_depth in ((256, None), (-2, None), (0, 13), (0, -2)):
            assert call(scene, sb.PruneOptions(tolerance, max_depth)) == L.ERR_ARG, (tolerance, max_depth)

        class Newer(ctypes.Structure):
            _fields_ = [("size", ctypes.c_uint32), ("tolerance", ctypes.c_int32), ("max_depth", ctypes.c_int32), ("unknown", ctypes.c_int32)]
        as_options = lambda o: ctypes.cast(ctypes.pointer(o), ctypes.POINTER(sb.PruneOptions)).contents
        assert call(scene, as_options(Newer(16, 0, -1, 3))) == L.ERR_ARG       # an unknown field that is set
        assert call(scene, as_options(Newer(16, 0, -1, -1))) == L.OK           # ... and one that says "default"
        small = sb.PruneOptions(0, None)
        small.size = 8
        assert call(scene, small) == L.ERR_ARG
        if L.EXPERIMENTS:                               # a device allocation that fails: NOMEM, the input untouched, nothing kept
            cam = make_camera("default", 64, 64)
            before = scene.Draw(cam, 64, 64)
            for k in (0, 2, 5, 6):
                monkeypatch.setenv("SDFHIP_PRUNE_FAIL_ALLOC", str(k))
                assert call(scene, None) == L.ERR_NOMEM
            monkeypatch.delenv("SDFHIP_PRUNE_FAIL_ALLOC")
            assert_frames_identical(scene.Draw(cam, 64, 64), before, "the input after a failed prune")
            assert call(scene, None) == L.OK
    # an inconsistent tree (a child whose parent field points elsewhere) uploads, but cannot be pruned
    S0, V0 = tree("sphere_d4")
    S = S0.copy()
    S[int(S[0, 1]) + 3, 0] = int(S[0, 1])
    bad_tree = sb.OctData(S, V0)
    assert bad_tree.validate()[1] is False
    with sb.Scene(bad_tree) as scene:
        assert not scene.stack_kernel_ok
        assert call(scene, None) == L.ERR_BAD_TREE

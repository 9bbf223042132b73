"""Space carving on the GPU (sdfhip_scene_edit), both flavours of the library: the edited tree is the CPU restatement's
(tests/edit_restatement.py) byte for byte, its frames are the oracle's on the restated arrays, the input handle is untouched, and
the errors are status codes."""
import ctypes

import numpy as np
import pytest

import edit_restatement as er
from conftest import CAMERAS, assert_frames_identical, make_camera

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["product", "lab"])
def sb(request):
    import sdfbox_amd
    if request.param == "product":
        return sdfbox_amd
    import sdfbox_amd.lab
    return sdfbox_amd.lab.load()


_trees = {}


def tree(name):
    """host arrays of the test scenes (the same for both flavours)"""
    if name not in _trees:
        import sdfbox_amd as base
        if name == "sphere_d4":
            _trees[name] = base.sphere_d4()
        elif name == "torus_d6":
            _trees[name] = base.torus_d6()
        elif name == "gyroid_d8":
            _trees[name] = base.dragon_standin(8, nthreads=16)
        elif name == "builder_d10":
            _trees[name] = base.OctData.SdfGen(base.knot_point_cloud(100_000, seed=3), 10)
        elif name == "dragon_d9":
            _trees[name] = base.dragon_standin(9, nthreads=16)
    return _trees[name]


def placements(od, small):
    """brush centres and sizes: through the surface, wholly inside the solid, far away, covering the root box, straddling its faces"""
    c, scale = er.deepest_leaf_centres(od.Structs)
    surf = tuple(c[len(c) // 2])
    out = {"surface": (surf, 0.06), "face": ((0.02, 0.5, 0.97), 0.1)}
    if small:
        out.update({"inside": ((0.5, 0.5, 0.5), 0.05), "far": ((2.5, -1.0, 0.5), 0.3), "cover": ((0.5, 0.5, 0.5), 1.2)})
    return out


def brushes(od, small):
    for where, (c, r) in placements(od, small).items():
        for op in (er.EDIT_CARVE, er.EDIT_ADD):
            yield where, op, er.BRUSH_SPHERE, (*c, r)
            yield where, op, er.BRUSH_BOX, (*c, r, 0.6 * r, 1.3 * r)


def gpu_edit(sb, scene, edits, max_depth=None):
    res, od, st = scene.Edit(edits, max_depth=max_depth, want_octdata=True, want_stats=True)
    return res, od, st


def assert_same_tree(od, S, V, what):
    assert od.Length == len(S), f"{what}: {od.Length} nodes, the restatement {len(S)}"
    bad_s = np.nonzero((od.Structs != S).any(1))[0]
    bad_v = np.nonzero((od.Values != V).any(1))[0]
    assert not len(bad_s) and not len(bad_v), (what, bad_s[:5].tolist(), bad_v[:5].tolist(),
                                                [(od.Values[i].tolist(), V[i].tolist()) for i in bad_v[:3]])


def split_windows(S, nodes_in):
    """{depth: (lowest, highest)} over the parents of an edit's new blocks (the nodes whose children link is >= nodes_in): per
    level, the span of the split bitmap that the edit ranks"""
    parents = np.nonzero(S[:, 1] >= nodes_in)[0]
    depth, up = np.zeros(len(parents), dtype=np.int64), S[parents, 0].astype(np.int64)
    while (up >= 0).any():
        depth[up >= 0] += 1
        up = np.where(up >= 0, S[np.maximum(up, 0), 0], -1)
    return {int(d): (int(parents[depth == d].min()), int(parents[depth == d].max())) for d in np.unique(depth)}


@pytest.mark.parametrize("name", ["sphere_d4", "torus_d6", "gyroid_d8", "builder_d10"])
def test_edited_bytes_are_the_restatements(sb, name):
    od = tree(name)
    d0 = er.tree_depth(od.Structs)
    small = od.Length < 1_000_000
    with sb.Scene(od) as scene:
        for where, op, brush, params in brushes(od, small):
            for md in ((-1, d0 + 1) if d0 < 12 else (-1,)):
                S, V = er.edit(od.Structs, od.Values, [(op, brush, params)], md, region=not small)
                if name == "gyroid_d8" and where == "surface" and md == d0 + 1:
                    # the window form of the shared word scan (k_rank_scan_words): the deepest level's splits are ranked over a
                    # window of the bitmap that does not start at word 0 and spans more than one chunk of 1024 words
                    lowest, highest = split_windows(S, od.Length)[d0]
                    assert lowest >> 5 > 0 and (highest >> 5) - (lowest >> 5) >= 1024, (op, brush, lowest, highest)
                res, got, st = gpu_edit(sb, scene, [(op, brush, params)], None if md < 0 else md)
                with res:
                    what = f"{name} {where} op={op} brush={brush} max_depth={md}"
                    assert_same_tree(got, S, V, what)
                    assert (st.nodes_in, st.nodes_out) == (od.Length, len(S)), what
                    assert st.blocks_added == (len(S) - od.Length) // 8 and st.depth_out == er.tree_depth(S), what
                    assert res.Length == len(S) and res.depth == st.depth_out and res.stack_kernel_ok
                    if where == "far":
                        assert st.nodes_visited <= 8 * (d0 + 2) and st.nodes_changed == 0, (what, st.nodes_visited)


def test_an_edit_list_equals_chained_calls_and_no_edit_is_a_clone(sb):
    od = tree("torus_d6")
    edits = [(er.EDIT_CARVE, er.BRUSH_SPHERE, (0.84, 0.5, 0.5, 0.05)), (er.EDIT_ADD, er.BRUSH_BOX, (0.5, 0.6, 0.2, 0.1, 0.04, 0.08)),
             (er.EDIT_CARVE, er.BRUSH_BOX, (0.3, 0.5, 0.5, 0.05, 0.2, 0.05))]
    with sb.Scene(od) as scene:
        whole, got, _ = gpu_edit(sb, scene, edits, 8)
        with whole:
            chain = scene
            for e in edits:
                nxt, part, _ = gpu_edit(sb, chain, [e], 8)
                if chain is not scene:
                    chain.close()
                chain = nxt
            chain.close()
            assert np.array_equal(got.Structs, part.Structs) and np.array_equal(got.Values, part.Values)
            S, V = er.edit(od.Structs, od.Values, edits, 8)
            assert_same_tree(got, S, V, "3-edit list")
        clone, c, st = gpu_edit(sb, scene, [])
        with clone:
            assert np.array_equal(c.Structs, od.Structs) and np.array_equal(c.Values, od.Values)
            assert (st.nodes_visited, st.blocks_added, clone.depth) == (0, 0, scene.depth)


@pytest.mark.parametrize("name", ["sphere_d4", "torus_d6"])
def test_edited_frames_are_the_oracles(sb, oracle_mod, name):
    od = tree(name)
    W = H = 256
    surf = placements(od, True)["surface"][0]
    edits = [(er.EDIT_CARVE, er.BRUSH_SPHERE, (*surf, 0.08)), (er.EDIT_ADD, er.BRUSH_BOX, (0.5, 0.5, 0.15, 0.12, 0.05, 0.05))]
    d0 = er.tree_depth(od.Structs)
    S, V = er.edit(od.Structs, od.Values, edits, d0 + 1)
    with sb.Scene(od) as scene:
        res, got, _ = gpu_edit(sb, scene, edits, d0 + 1)
        with res, sb.Scene(got) as fresh:
            assert_same_tree(got, S, V, name)
            for cam_name in CAMERAS:
                cam = make_camera(cam_name, W, H)
                ref, cnt = oracle_mod.render(S, V, cam.State, W, H)
                for flags in (sb.KERNEL_AUTO, sb.KERNEL_GENERIC):
                    img, st = res.Draw(cam, W, H, flags | sb.FLAG_COUNT, want_stats=True)
                    assert_frames_identical(img, ref, f"{name} {cam_name} flags {flags}")
                    assert (st.n_nodes, st.n_samples, st.n_steps, st.n_shadow_rays) == tuple(int(c) for c in cnt)
                    img2, st2 = fresh.Draw(cam, W, H, flags | sb.FLAG_COUNT, want_stats=True)
                    assert_frames_identical(img2, img, f"{name} {cam_name}: the uploaded host_out")
                    assert (st2.n_nodes, st2.n_samples, st2.n_steps, st2.n_shadow_rays, st2.n_loads) == \
                        (st.n_nodes, st.n_samples, st.n_steps, st.n_shadow_rays, st.n_loads)


def test_the_input_handle_is_untouched(sb):
    od = tree("torus_d6")
    W = H = 128
    cam = make_camera("rotated", W, H)
    scene = sb.Scene(od)
    before = scene.Draw(cam, W, H)
    res = scene.Edit([(er.EDIT_CARVE, er.BRUSH_SPHERE, (0.5, 0.5, 0.5, 0.45))], max_depth=7)
    edited = res.Draw(cam, W, H)
    assert not np.array_equal(edited, before)
    assert_frames_identical(scene.Draw(cam, W, H), before, "the input after an edit")
    scene.close()                                   # either handle may go first
    assert_frames_identical(res.Draw(cam, W, H), edited, "the result after the input was freed")
    res2 = res.Edit([])
    res.close()
    assert_frames_identical(res2.Draw(cam, W, H), edited, "a clone after its input was freed")
    res2.close()


def test_one_carve_on_the_28m_node_scene(sb, oracle_mod):
    od = tree("dragon_d9")
    W, H = 1920, 1080
    cam = sb.Logic(W, H)
    cam.Position = (0.5, 0.5, -0.35); cam.Heading = (-0.2, 0.35)        # cfg-2's camera
    c = er.surface_point_under(od.Structs, cam.Position, [list(r) for r in cam.State.heading])
    edit = (er.EDIT_CARVE, er.BRUSH_SPHERE, (*c, 0.05))
    S, V = er.edit(od.Structs, od.Values, [edit], -1, region=True)
    with sb.Scene(od) as scene:
        res, got, st = gpu_edit(sb, scene, [edit])
        with res:
            assert_same_tree(got, S, V, "dragon_d9 r=0.05")
            assert st.nodes_changed > 1000 and st.nodes_visited < od.Length // 4, (st.nodes_changed, st.nodes_visited)
            a, b = scene.Draw(cam, W, H), res.Draw(cam, W, H)
            rows = np.nonzero((a != b).any(axis=(1, 2)))[0]
            assert len(rows) > 10, "the brush is not in view"
            for y in rows[np.linspace(0, len(rows) - 1, 4).astype(int)]:
                ref, _ = oracle_mod.render(S, V, cam.State, W, H, row0=int(y), nrows=1, nthreads=16)
                assert_frames_identical(b[y:y + 1], ref.reshape(1, W, 4), f"1080p row {y}")


def test_errors_are_status_codes(sb, monkeypatch):
    L = sb._lib
    od = tree("sphere_d4")
    ok = sb.Edit(sb.EDIT_CARVE, sb.BRUSH_SPHERE, (0.5, 0.5, 0.5, 0.1))

    def call(scene, edits, n=None, max_depth=-1, out=True):
        arr = (sb.Edit * max(1, len(edits)))(*edits)
        h = ctypes.c_void_p()
        rc = L.lib.sdfhip_scene_edit(scene._h if scene is not None else None, arr if edits else None, len(edits) if n is None else n,
                                     max_depth, ctypes.byref(h) if out else None, None, None)
        if h.value:
            L.lib.sdfhip_scene_free(h)
        assert rc == L.OK or not h.value
        return rc

    with sb.Scene(od) as scene:
        assert call(scene, [ok]) == L.OK
        assert call(None, [ok]) == L.ERR_ARG
        assert call(scene, [ok], out=False) == L.ERR_ARG
        assert call(scene, [], n=1) == L.ERR_ARG
        bad = [sb.Edit(2, 0, (0.5, 0.5, 0.5, 0.1)), sb.Edit(0, 2, (0.5, 0.5, 0.5, 0.1)), sb.Edit(0, 0, (0.5, float("nan"), 0.5, 0.1)),
               sb.Edit(1, 1, (0.5, 0.5, float("inf"), 0.1, 0.1, 0.1)), sb.Edit(0, 0, (0.5, 0.5, 0.5, 0.0)),
               sb.Edit(0, 0, (0.5, 0.5, 0.5, -0.1)), sb.Edit(0, 1, (0.5, 0.5, 0.5, 0.1, 0.0, 0.1))]
        for e in bad:
            assert call(scene, [ok, e]) == L.ERR_ARG, (e.op, e.brush, list(e.params))
        for md in (13, -2):
            assert call(scene, [ok], max_depth=md) == L.ERR_ARG
        assert call(scene, [ok], max_depth=12) == L.OK
        if L.EXPERIMENTS:                               # a device allocation that fails: NOMEM, the input untouched, nothing kept
            cam = make_camera("default", 64, 64)
            before = scene.Draw(cam, 64, 64)
            for k in (0, 1, 3):
                monkeypatch.setenv("SDFHIP_EDIT_FAIL_ALLOC", str(k))
                assert call(scene, [ok], max_depth=6) == L.ERR_NOMEM
            monkeypatch.delenv("SDFHIP_EDIT_FAIL_ALLOC")
            assert_frames_identical(scene.Draw(cam, 64, 64), before, "the input after a failed edit")
            assert call(scene, [ok], max_depth=6) == L.OK
    # an inconsistent tree (a child whose parent field points elsewhere) uploads, but cannot be edited
    S = od.Structs.copy()
    S[int(S[0, 1]) + 3, 0] = int(S[0, 1])
    bad_tree = sb.OctData(S, od.Values)
    assert bad_tree.validate()[1] is False
    with sb.Scene(bad_tree) as scene:
        assert not scene.stack_kernel_ok
        assert call(scene, [ok]) == L.ERR_BAD_TREE

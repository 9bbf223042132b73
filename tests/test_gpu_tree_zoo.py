"""Edit, query and mesh on the tree zoo (tests/tree_zoo.py), both flavours of the library: trees in depth-first order, a 12-deep and a
14-deep chain, a root that is a leaf, node counts one past the mesh passes' wave, row and chunk, all filled with bytes that are no
distance field.  Every vertex, record and node is the numpy restatement's (tests/mesh_restatement.py, query_restatement.py,
edit_restatement.py; tests/test_tree_zoo.py holds those to the frozen oracle and to their invariants on these same trees) byte for
byte, NaN equal to NaN.  Then the consumers composed: mesh, queries and frames on the handle an overlapping chain of edits returned
-- a scene made from device arrays -- against the restated arrays and against the same arrays uploaded from the host."""
import ctypes

import numpy as np
import pytest

import edit_restatement as er
import mesh_restatement as mr
import query_restatement as qr
import tree_zoo as tz
from conftest import CAMERAS, assert_frames_identical, make_camera
from test_gpu_edit import assert_same_tree
from test_gpu_mesh import assert_mesh
from test_gpu_query import SKY, assert_records, frame_pixels, random_rays
from test_query import lattice_points, outside_points

pytestmark = pytest.mark.gpu
f32 = np.float32
want = tz.restated                                             # each restatement answer once, for both flavours


@pytest.fixture(scope="module", params=["product", "lab"])
def sb(request):
    import sdfbox_amd
    if request.param == "product":
        return sdfbox_amd
    import sdfbox_amd.lab
    return sdfbox_amd.lab.load()


def octdata(sb, name):
    s, v = tz.zoo()[name]
    return sb.OctData(s, v)


# ---- mesh ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tz.MESHABLE)
def test_mesh_is_the_restatements_on_the_zoo(sb, name, monkeypatch):
    import torch
    s, v = tz.zoo()[name]
    depth = er.tree_depth(s)
    walked = want(("walk", name), lambda: mr.walk(s))
    with sb.Scene(octdata(sb, name)) as scene:
        assert scene.stack_kernel_ok and scene.depth == depth
        for level in tz.mesh_levels(depth):
            ref, _, (cells, cut) = want(("mesh", name, level), lambda: mr.mesh(s, v, level, want_cells=True, walked=walked))
            n = len(ref)
            got, st = scene.Mesh(level)
            assert (st.nodes, st.cells, st.cells_cut, st.n_triangles) == (len(s), cells, cut, n), (name, level)
            assert_mesh(got, ref, (name, level))
            assert scene.MeshDevice(level=level) == n, (name, level)
            # the _device form into a buffer one triangle longer than needed: the guard triangle stays
            buf = torch.full((n + 1, 3, 6), -7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            assert scene.MeshDevice(buf.data_ptr(), n, level=level) == n
            torch.cuda.synchronize()
            host = buf.cpu().numpy()
            assert_mesh(host[:n], ref, (name, level, "the _device form"))
            assert (host[n] == -7.0).all(), (name, level, "the guard triangle")
        if name == "dfs_d6_a" and sb._lib.EXPERIMENTS:           # the A/B store forms give the same bytes
            ref = want(("mesh", name, -1), None)[0]
            for knob, value in (("SDFHIP_MESH_STORE", "nt"), ("SDFHIP_MESH_VEC", "8")):
                monkeypatch.setenv(knob, value)
                assert_mesh(scene.Mesh(-1, want_stats=False), ref, (name, knob, value))
                monkeypatch.delenv(knob)


def test_a_tree_deeper_than_12_is_not_meshed_or_edited(sb):
    import torch
    L = sb._lib
    out, n = L.CMesh(), ctypes.c_uint32(7)
    with sb.Scene(octdata(sb, "chain14")) as scene:
        assert not scene.stack_kernel_ok and scene.depth == 14
        assert L.lib.sdfhip_scene_mesh(scene._h, None, ctypes.byref(out), None) == L.ERR_BAD_TREE
        assert out.n_triangles == 0 and not out.verts6
        buf = torch.full((64, 3, 6), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert L.lib.sdfhip_scene_mesh_device(scene._h, None, ctypes.c_void_p(buf.data_ptr()), 64, ctypes.byref(n), None) == L.ERR_BAD_TREE
        torch.cuda.synchronize()
        assert n.value == 0 and (buf.cpu().numpy() == -7.0).all()
        with pytest.raises(sb.SdfHipError) as e:
            scene.Edit([(er.EDIT_ADD, er.BRUSH_SPHERE, (*tz.placement("chain12")[0], tz.placement("chain12")[1]))])
        assert e.value.code == L.ERR_BAD_TREE


# ---- queries ---------------------------------------------------------------------------------------------------------------------
def uploads(sb, name, depth):
    """(what, scene, the form its marches take): no grid, a plain grid of a middle level (not as deep as the tree: the queries walk
    the links), a split grid with a middle coarse level, and the upload's own choice"""
    od = octdata(sb, name)
    yield "no grid", sb.Scene(od, top_grid_level=0), "generic"
    if name == "chain14":
        return
    if depth >= 2:
        yield "plain grid of a middle level", sb.Scene(od, top_grid_level=depth // 2), "generic"
        yield "split grid", sb.Scene(od, top_grid_split=max(depth // 2, depth - 6)), "split"
    yield "default", sb.Scene(od), "dense" if 1 <= depth <= 8 else None


def query_inputs(name, depth):
    rng = np.random.default_rng(101)
    pts = {"uniform": rng.random((20_000, 3)).astype(f32), "lattice": lattice_points(rng, depth), "outside": outside_points(rng)}
    return pts, random_rays(7, 20_000), frame_pixels(64, 64)


@pytest.mark.parametrize("name", tz.ALL_TREES)
def test_queries_are_the_restatements_on_the_zoo_in_every_form(sb, name, monkeypatch):
    s, v = tz.zoo()[name]
    depth = er.tree_depth(s)
    pts, (o, d), pixels = query_inputs(name, depth)
    cams = {c: make_camera(c, 64, 64) for c in CAMERAS}
    ref_s = {k: want(("sample", name, k), lambda: qr.sample(s, v, p)) for k, p in pts.items()}
    ref_r = want(("rays", name), lambda: qr.raycast(s, v, o, d, 0.001, 4.0, 100))
    ref_p = {c: want(("pick", name, c), lambda: qr.pick(s, v, cam.State, pixels)) for c, cam in cams.items()}
    forms = set()
    for what, scene, form in uploads(sb, name, depth):
        with scene:
            # which form: from the grid the handle reports
            if name == "chain14":
                assert not scene.stack_kernel_ok and scene.depth == 14
            else:
                assert scene.stack_kernel_ok and scene.depth == depth
            if form == "generic":
                assert scene.top_grid_level < max(depth, 1) or not scene.stack_kernel_ok, (name, what, scene.top_grid_level)
                assert what != "no grid" or scene.top_grid_level == 0
            elif form == "split":
                assert scene.top_grid_level == max(depth // 2, depth - 6) < depth, (name, what, scene.top_grid_level)
                assert scene.top_grid_bytes >= 16 << (3 * scene.top_grid_level)
            elif form == "dense":
                assert scene.top_grid_level == depth, (name, what, scene.top_grid_level)
            forms.add(form)

            def check(tag):
                for k, p in pts.items():
                    got = scene.Sample(p)
                    assert (got["status"] == qr.HIT).all()
                    assert_records(got, ref_s[k], (name, what, tag, "sample", k))
                assert_records(scene.Raycast(o, d, 0.001, 4.0, 100), ref_r, (name, what, tag, "raycast"))
                for c, cam in cams.items():
                    assert_records(scene.Pick(cam, pixels), ref_p[c], (name, what, tag, "pick", c))

            check("the library's choice")
            if sb._lib.EXPERIMENTS:                             # sample walks the links and the march looks the grid up: force both
                for forced in ("grid", "generic"):
                    monkeypatch.setenv("SDFHIP_QUERY_FORM", forced)
                    check(f"SDFHIP_QUERY_FORM={forced}")
                monkeypatch.delenv("SDFHIP_QUERY_FORM")
            if what == "default" or name == "chain14":
                # picks against the GPU's own frame: sky <=> ESCAPED, with steps == alpha there; elsewhere steps <= alpha
                for c, cam in cams.items():
                    frame = scene.Draw(cam, 64, 64).reshape(-1, 4)
                    sky = (frame[:, :3].view(np.uint32) == SKY.view(np.uint32)).all(1)
                    assert ((ref_p[c]["status"] == qr.ESCAPED) == sky).all(), (name, c)
                    assert (ref_p[c]["steps"][sky] == frame[sky, 3]).all() and (ref_p[c]["steps"][~sky] <= frame[~sky, 3]).all(), (name, c)
    if name == "chain14" or depth < 2:
        assert forms <= {"generic", None, "dense"} and "generic" in forms      # the 12-descent cap binds: only the links may be walked
    else:
        assert {"generic", "split"} <= forms and (depth > 8 or "dense" in forms), (name, forms)


# ---- edit ------------------------------------------------------------------------------------------------------------------------
def gpu_edit(scene, edits, md):
    return scene.Edit(edits, max_depth=None if md < 0 else md, want_octdata=True, want_stats=True)


def assert_edit(sb, res, got, st, n_in, S, V, what):
    assert_same_tree(got, S, V, what)
    assert (st.nodes_in, st.nodes_out) == (n_in, len(S)), what
    assert st.blocks_added == (len(S) - n_in) // 8 and st.depth_out == er.tree_depth(S), what
    assert res.Length == len(S) and res.depth == st.depth_out and res.stack_kernel_ok, what


@pytest.mark.parametrize("name", tz.EDITED)
def test_edited_bytes_are_the_restatements_on_the_zoo(sb, name):
    s, v = tz.zoo()[name]
    d0 = er.tree_depth(s)
    grew = 0
    with sb.Scene(octdata(sb, name)) as scene:
        for label, e in tz.single_edits(name):
            for md in tz.max_depths(d0):
                S, V = tz.restated_edit(name, [e], md)
                res, got, st = gpu_edit(scene, [e], md)
                with res:
                    assert_edit(sb, res, got, st, len(s), S, V, f"{name} {label} max_depth={md}")
                    grew += 8 * st.blocks_added > len(s) // 16 + 4096
    if name in ("dfs_d6_a", "blocks_1025", "blocks_4097"):
        assert grew >= 1, "one call that outgrows the arrays' initial capacity (n + n / 16 + 4096)"


def test_a_tie_between_brush_and_field_at_the_centre_does_not_split(sb):
    """The split rule is strict: the brush must WIN at the cell's centre (-s(c) > v(c) for a carve).  A flat leaf holds v(c) = the
    decoded byte exactly (a lerp between equal values returns them), a sphere about the cell's centre has s(c) = -r exactly, so a
    radius equal to the decoded byte is a tie: no split, though the centre lies within the band and max_depth allows one."""
    b = 200
    r = float(er.decode(np.array([b], dtype=np.uint8), f32(1))[0])
    assert 0 < r < 2
    s, v = np.array([[-1, -1]], dtype=np.int32), np.full((1, 8), b, dtype=np.uint8)
    with sb.Scene(sb.OctData(s, v)) as scene:
        for radius, splits in ((r, False), (float(np.nextafter(f32(r), f32(2))), True)):
            e = (er.EDIT_CARVE, er.BRUSH_SPHERE, (0.5, 0.5, 0.5, radius))
            S, V = er.edit(s, v, [e], 1)
            assert (len(S) == 9) == splits
            res, got, st = gpu_edit(scene, [e], 1)
            with res:
                assert_edit(sb, res, got, st, 1, S, V, f"tie at the centre, r = {radius!r}")


def run_chain(sb, scene, name):
    """the overlapping chain as two calls -> (handle, arrays) of B's result; A's handle is closed"""
    s, _ = tz.zoo()[name]
    a, md_a, b, md_b = tz.overlapping_chain(name, er.tree_depth(s))
    (SA, VA), (SB, VB), _ = tz.restated_chain(name)
    res_a, got_a, st_a = gpu_edit(scene, [a], md_a)
    with res_a:
        assert_edit(sb, res_a, got_a, st_a, len(s), SA, VA, f"{name}: A")
        res_b, got_b, st_b = gpu_edit(res_a, [b], md_b)
    assert_edit(sb, res_b, got_b, st_b, len(SA), SB, VB, f"{name}: B on A's handle")
    return res_b, got_b


@pytest.mark.parametrize("name", tz.EDITED)
def test_an_overlapping_chain_as_two_calls_and_as_a_list(sb, name):
    s, v = tz.zoo()[name]
    a, md_a, b, md_b = tz.overlapping_chain(name, er.tree_depth(s))
    SL, VL = tz.restated_chain(name)[2]
    with sb.Scene(octdata(sb, name)) as scene:
        res_b, _ = run_chain(sb, scene, name)
        res_b.close()
        # the list [A, B] at B's depth: the restatement's, and the same two edits as two calls at that depth
        whole, got, st = gpu_edit(scene, [a, b], md_b)
        with whole:
            assert_edit(sb, whole, got, st, len(s), SL, VL, f"{name}: the list [A, B]")
        first, _, _ = gpu_edit(scene, [a], md_b)
        with first:
            second, part, _ = gpu_edit(first, [b], md_b)
            second.close()
        assert np.array_equal(got.Structs, part.Structs) and np.array_equal(got.Values, part.Values), name


# ---- composition -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dfs_d6_a", "chain12"])
def test_mesh_queries_and_frames_on_an_edited_handle(sb, oracle_mod, name):
    s, _ = tz.zoo()[name]
    d0 = er.tree_depth(s)
    S, V = tz.restated_chain(name)[1]
    key = ("edited", name)
    rng = np.random.default_rng(103)
    pts = rng.random((20_000, 3)).astype(f32)
    o, d = random_rays(11, 20_000)
    pixels = frame_pixels(64, 64)
    cams = {c: make_camera(c, 64, 64) for c in CAMERAS}
    walked = want((key, "walk"), lambda: mr.walk(S))
    ref_m = {lv: want((key, "mesh", lv), lambda: mr.mesh(S, V, lv, walked=walked)) for lv in (-1, d0)}
    ref_s = want((key, "sample"), lambda: qr.sample(S, V, pts))
    ref_r = want((key, "rays"), lambda: qr.raycast(S, V, o, d, 0.001, 4.0, 100))
    ref_p = want((key, "pick"), lambda: qr.pick(S, V, cams["rotated"].State, pixels))
    ref_f = {c: want((key, "frame", c), lambda: oracle_mod.render(S, V, cam.State, 64, 64)[0]) for c, cam in cams.items()}
    with sb.Scene(octdata(sb, name)) as scene:
        edited, got = run_chain(sb, scene, name)
    with edited, sb.Scene(got) as fresh:                        # (the input handle is gone: the result stands alone)
        assert (fresh.Length, fresh.depth, fresh.top_grid_level) == (edited.Length, edited.depth, edited.top_grid_level)
        for what, sc in (("the edit's handle", edited), ("its arrays uploaded", fresh)):
            for lv, ref in ref_m.items():
                assert_mesh(sc.Mesh(lv, want_stats=False), ref, (name, what, lv))
            assert len(ref_m[-1]) > 0
            assert_records(sc.Sample(pts), ref_s, (name, what, "sample"))
            assert_records(sc.Raycast(o, d, 0.001, 4.0, 100), ref_r, (name, what, "raycast"))
            assert_records(sc.Pick(cams["rotated"], pixels), ref_p, (name, what, "pick"))
            for c, cam in cams.items():
                assert_frames_identical(sc.Draw(cam, 64, 64), ref_f[c], f"{name}: {what}, camera {c}")

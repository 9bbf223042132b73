"""Prune, combine, place and measure on the tree zoo (tests/tree_zoo.py), both flavours of the library: the four calls that take any
uploaded handle, on trees no builder of the project lays out -- depth-first order, blocks appended under random leaves, a 12-deep
chain, one node, node counts one past a wave, a row and a scan chunk, bytes that are no distance field.  Every node, byte, double and
count is the numpy restatement's (tests/prune_restatement.py, combine_restatement.py, place_restatement.py, measure_restatement.py;
tests/test_zoo_builders.py holds those to things they did not come from on these same cases), with no tolerance anywhere.  Then the
14-deep chain, which only a placement with a depth given accepts, and the calls chained on the handles they return -- scenes made from
device arrays -- against the restatements chained and the oracle's frames."""
import ctypes

import numpy as np
import pytest

import combine_restatement as cr
import edit_restatement as er
import measure_restatement as ms
import prune_restatement as pr
import tree_zoo as tz
from conftest import assert_frames_identical, make_camera
from test_gpu_measure import assert_same_measure
from test_gpu_prune import assert_same_tree

pytestmark = pytest.mark.gpu
OP_NAMES = {cr.COMBINE_UNION: "union", cr.COMBINE_INTERSECT: "intersect", cr.COMBINE_SUBTRACT: "subtract"}
UNIFORM = ("chain12", "dfs_d6_a", "blocks_65", "blocks_1025", "blocks_4097")         # the trees filled with fill_uniform
W, H = 64, 48


@pytest.fixture(scope="module", params=["product", "lab"])
def sb(request):
    import sdfbox_amd
    if request.param == "product":
        return sdfbox_amd
    import sdfbox_amd.lab
    return sdfbox_amd.lab.load()


def upload(sb, name, **kw):
    s, v = tz.zoo()[name]
    return sb.Scene(sb.OctData(s, v), **kw)


def opt_depth(max_depth):
    return None if max_depth < 0 else max_depth


# ---- prune -----------------------------------------------------------------------------------------------------------------------
def assert_prune(res, got, st, n_in, S, V, what):
    assert_same_tree(got, S, V, what)
    assert (st.nodes_in, st.nodes_out, st.blocks_removed) == (n_in, len(S), (n_in - len(S)) // 8), what
    assert st.depth_out == er.tree_depth(S), what
    assert res.Length == len(S) and res.depth == st.depth_out and res.stack_kernel_ok, what


@pytest.mark.parametrize("name", tz.MESHABLE)
def test_pruned_bytes_are_the_restatements_on_the_zoo(sb, name):
    s, v = tz.zoo()[name]
    depth = er.tree_depth(s)
    with upload(sb, name) as scene:
        assert scene.stack_kernel_ok and scene.depth == depth
        for tolerance in tz.PRUNE_TOLERANCES:
            for max_depth in tz.prune_depths(depth):
                S, V = tz.restated_prune(name, tolerance, max_depth)
                res, got, st = scene.Prune(tolerance, opt_depth(max_depth), want_octdata=True, want_stats=True)
                with res:
                    assert_prune(res, got, st, len(s), S, V, f"prune({name}) tolerance={tolerance} max_depth={max_depth}")
                    if tolerance == 0 and max_depth < 0 and name in UNIFORM:
                        # nothing is removed: the source's arrays in the source's own order, depth first or in order of appending
                        assert st.blocks_removed == 0
                        assert_same_tree(got, s, v, f"prune({name}) at tolerance 0 against the source")


# ---- combine ---------------------------------------------------------------------------------------------------------------------
def check_combine(sa, sb_, a, b, op, max_depth):
    S, V, counts = tz.restated_combine(a, b, op, max_depth)
    res, got, st = sa.Combine(sb_, op, opt_depth(max_depth), want_octdata=True, want_stats=True)
    with res:
        what = f"{OP_NAMES[op]}({a}, {b}) max_depth={max_depth}"
        assert_same_tree(got, S, V, what)
        assert (st.nodes_a, st.nodes_b, st.nodes_out) == (len(tz.zoo()[a][0]), len(tz.zoo()[b][0]), len(S)), what
        assert (st.nodes_shared, st.depth_out) == (counts["nodes_shared"], counts["depth_out"]) and st.depth_out == er.tree_depth(S), what
        assert res.Length == len(S) and res.depth == st.depth_out and res.stack_kernel_ok, what


_PAIRS = tz.COMBINE_PAIRS + tz.COMBINE_REVERSED


@pytest.mark.parametrize("a, b", _PAIRS, ids=["-".join(p) for p in _PAIRS])
def test_combined_bytes_are_the_restatements_on_the_zoo(sb, a, b):
    cases = [c for c in tz.combine_cases() if c[:2] == (a, b)]
    assert len(cases) == (2 if (a, b) in tz.COMBINE_REVERSED else 6)
    with upload(sb, a) as sa:
        if a == b:                                                  # ONE handle as both operands
            for _, _, op, max_depth in cases:
                check_combine(sa, sa, a, b, op, max_depth)
        else:
            with upload(sb, b) as sb_:
                for _, _, op, max_depth in cases:
                    check_combine(sa, sb_, a, b, op, max_depth)


# ---- place -----------------------------------------------------------------------------------------------------------------------
def check_place(scene, src, name, depth, n_in=None):
    S, V, counts = tz.restated_place(src, name, depth)
    res, got, st = scene.Place(*tz.place_args(name), depth, want_octdata=True, want_stats=True)
    with res:
        what = f"place({src}, {name}) depth={depth}, top grid level {scene.top_grid_level}"
        assert_same_tree(got, S, V, what)
        assert (st.nodes_in, st.nodes_out, st.depth_out, st.levels) == (len(tz.zoo()[src][0]), len(S), counts["depth_out"], counts["levels"]), what
        assert st.samples == counts["samples"] and st.depth_out == er.tree_depth(S), what
        assert res.Length == len(S) and res.depth == st.depth_out and res.stack_kernel_ok, what


@pytest.mark.parametrize("src", list(tz.PLACE_DEPTHS))
def test_placed_bytes_are_the_restatements_on_the_zoo(sb, src):
    with upload(sb, src) as scene:
        assert scene.stack_kernel_ok
        for _, name, depth in tz.place_cases(src):
            check_place(scene, src, name, depth)


@pytest.mark.parametrize("src", ["dfs_d6_a", "chain12"])
def test_every_cursor_form_places_the_same_bytes_on_the_zoo(sb, src):
    """the look-up through a split grid and the walk along the links alone (test_placed_bytes_... takes the upload's own choice)"""
    depth = er.tree_depth(tz.zoo()[src][0])
    with upload(sb, src, top_grid_split=max(depth // 2, depth - 6)) as split, upload(sb, src, top_grid_level=0) as without:
        assert split.top_grid_level == max(depth // 2, depth - 6) < depth and without.top_grid_level == 0
        for scene in (split, without):
            for _, name, d in tz.place_cases(src):
                check_place(scene, src, name, d)


# ---- measure ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tz.MESHABLE)
def test_every_double_and_count_is_the_restatements_on_the_zoo(sb, name):
    depth = er.tree_depth(tz.zoo()[name][0])
    with upload(sb, name) as scene:
        assert scene.stack_kernel_ok
        for level in tz.mesh_levels(depth):
            want = tz.restated_measure(name, level)
            first = scene.Measure(level)
            assert_same_measure(first, want, f"measure({name}, level {level})")
            assert_same_measure(scene.Measure(level), want, f"measure({name}, level {level}) again")


# ---- the 14-deep chain -----------------------------------------------------------------------------------------------------------
def test_a_tree_deeper_than_12_is_refused_or_placed_by_the_walk(sb):
    L = sb._lib

    def handle_call(fn, *args):
        h = ctypes.c_void_p()
        rc = fn(*args, ctypes.byref(h), None, None)
        if h.value:
            L.lib.sdfhip_scene_free(h)
        assert rc == L.OK or not h.value, "*out is not null after a failure"
        return rc

    with upload(sb, "chain14") as deep, upload(sb, "chain12") as other:
        assert not deep.stack_kernel_ok and deep.depth == 14 and other.stack_kernel_ok
        assert handle_call(L.lib.sdfhip_scene_prune, deep._h, None) == L.ERR_BAD_TREE
        assert handle_call(L.lib.sdfhip_scene_prune, deep._h, ctypes.byref(sb.PruneOptions(255, 3))) == L.ERR_BAD_TREE
        for a, b in ((deep, other), (other, deep), (deep, deep)):
            for op in cr.OPS:
                assert handle_call(L.lib.sdfhip_scene_combine, a._h, b._h, op, None) == L.ERR_BAD_TREE
        out = L.Measure()
        ctypes.memset(ctypes.byref(out), 0xFF, ctypes.sizeof(out))
        assert L.lib.sdfhip_scene_measure(deep._h, None, ctypes.byref(out)) == L.ERR_BAD_TREE
        assert bytes(out) == bytes(ctypes.sizeof(out)), "*out is zeroed on failure"
        with pytest.raises(sb.SdfHipError) as e:
            deep.Measure(4)
        assert e.value.code == L.ERR_BAD_TREE
        # no depth given: the source's own is none the library can use.  With one, the look-ups walk the links of all 14 levels
        for name in tz.PLACE_NAMES:
            R, s, t = tz.place_args(name)
            pl = sb.Placement(np.asarray(R).tolist(), float(s), [float(x) for x in t])
            assert handle_call(L.lib.sdfhip_scene_place, deep._h, ctypes.byref(pl)) == L.ERR_BAD_TREE
            check_place(deep, "chain14", name, 4)
        # the refused calls left both handles as they were
        check_place(other, "chain12", "identity", 4)


# ---- chains on returned handles --------------------------------------------------------------------------------------------------
def frames_of(scenes, cam):
    return [sc.Draw(cam, W, H) for sc in scenes]


def test_combine_prune_measure_on_returned_handles(sb, oracle_mod):
    a, b = "dfs_d6_a", "dfs_d6_b"
    US, UV, _ = tz.restated_combine(a, b, cr.COMBINE_UNION, -1)
    PS, PV = tz.restated(("chain 1", "pruned"), lambda: pr.prune(US, UV, 8, 5))
    want = tz.restated(("chain 1", "measured"), lambda: ms.measure(PS, PV))
    assert 1 < len(PS) < len(US) and er.tree_depth(PS) == 5 and want.cells_cut > 100
    cam = make_camera("rotated", W, H)
    ref = tz.restated(("chain 1", "frame"), lambda: oracle_mod.render(PS, PV, cam.State, W, H)[0])
    with upload(sb, a) as sa, upload(sb, b) as sb_:
        before = frames_of((sa, sb_), cam)
        united, got_u = sa.Combine(sb_, cr.COMBINE_UNION, want_octdata=True)
        with united:
            assert_same_tree(got_u, US, UV, "union")
            pruned, got_p, st = united.Prune(8, 5, want_octdata=True, want_stats=True)
        with pruned:                                                # (the union's handle is gone: the result stands alone)
            assert_prune(pruned, got_p, st, len(US), PS, PV, "union -> prune(8, 5)")
            assert_same_measure(pruned.Measure(), want, "union -> prune(8, 5) -> measure")
            assert_frames_identical(pruned.Draw(cam, W, H), ref, "union -> prune(8, 5)")
            assert_frames_identical(pruned.Draw(cam, W, H, sb.KERNEL_GENERIC), ref, "union -> prune(8, 5), the generic kernel")
        for sc, frame, which in zip((sa, sb_), before, "ab"):
            assert_frames_identical(sc.Draw(cam, W, H), frame, f"operand {which} after the chain")


def test_place_combine_prune_on_returned_handles(sb, oracle_mod):
    src, name, depth = "blocks_1025", "dyadic_075", 4
    S1, V1, _ = tz.restated_place(src, name, depth)
    S2, V2 = tz.restated(("chain 2", "cut"), lambda: cr.combine((S1, V1), tz.zoo()["leaf"], cr.COMBINE_SUBTRACT))
    S3, V3 = tz.restated(("chain 2", "pruned"), lambda: pr.prune(S2, V2, 0))
    assert len(S2) == len(S1) > 1000 and 1 < len(S3) < len(S2)
    cam = make_camera("rotated", W, H)
    ref = tz.restated(("chain 2", "frame"), lambda: oracle_mod.render(S3, V3, cam.State, W, H)[0])
    with upload(sb, src) as source, upload(sb, "leaf") as leaf:
        before = frames_of((source, leaf), cam)
        with source.Place(*tz.place_args(name), depth) as placed:
            cut, got_c = placed.Combine(leaf, cr.COMBINE_SUBTRACT, want_octdata=True)
        with cut:
            assert_same_tree(got_c, S2, V2, "place -> subtract")
            pruned, got_p, st = cut.Prune(0, None, want_octdata=True, want_stats=True)
        with pruned:
            assert_prune(pruned, got_p, st, len(S2), S3, V3, "place -> subtract -> prune(0)")
            assert_frames_identical(pruned.Draw(cam, W, H), ref, "place -> subtract -> prune(0)")
            assert_frames_identical(pruned.Draw(cam, W, H, sb.KERNEL_GENERIC), ref, "place -> subtract -> prune(0), the generic kernel")
        for sc, frame, which in zip((source, leaf), before, ("the source", "the leaf")):
            assert_frames_identical(sc.Draw(cam, W, H), frame, f"{which} after the chain")

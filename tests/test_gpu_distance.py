"""Exact distance, offset and shell on the GPU (sdfhip_scene_distance / _distance_device / sdfhip_scene_offset), both flavours of the
library: every Offset, Shell and Distance result below is the brute-force restatement's (tests/distance_restatement.py: every point
against every triangle of the restated mesh, no search, no pruning) byte for byte -- a sphere, a torus, a sphere with a concave
crease carved into it, the hostile trees of tests/tree_zoo.py that the mesh accepts; results coarser than, as deep as and deeper than
the source; delta of both signs and zero; a level-of-detail surface -- the same call twice gives the same bytes and the same
`visited` (the search order depends on the point and the scene alone), the result chains with the render, the prune, the combination
and the measure, and the errors are status codes."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import combine_restatement as cr
import distance_restatement as dr
import edit_restatement as er
import measure_restatement as msr
import prune_restatement as pr
import tree_zoo
from conftest import REPO, assert_frames_identical, make_camera
from test_gpu_prune import assert_same_tree
from test_gpu_prune import tree as prune_tree

pytestmark = pytest.mark.gpu
f32 = np.float32
G, SH = dr.GROW, dr.SHELL


@pytest.fixture(scope="module", params=["product", "lab"])
def sb(request):
    import sdfbox_amd
    if request.param == "product":
        return sdfbox_amd
    import sdfbox_amd.lab
    return sdfbox_amd.lab.load()


_trees = {}


def tree(name):
    """(structs, values) of the sources (the same for both flavours), made once"""
    if name not in _trees:
        import sdfbox_amd as base
        if name == "torus_d4":
            od = base.OctData.Generate(base._lib.SHAPE_TORUS, [0.5, 0.5, 0.5, 0.25, 0.1], 4)
            _trees[name] = (od.Structs, od.Values)
        elif name == "carved":           # one sphere brush out of the sphere's side: a concave crease, and an edge between two sheets
            _trees[name] = er.edit(*prune_tree("sphere_d4"), [(er.EDIT_CARVE, er.BRUSH_SPHERE, (0.74, 0.6, 0.56, 0.17))], -1)
        elif name == "empty":
            _trees[name] = (np.array([[-1, -1]], dtype=np.int32), np.full((1, 8), 255, dtype=np.uint8))
        elif name in tree_zoo.ALL_TREES:
            _trees[name] = tree_zoo.zoo()[name]
        else:
            _trees[name] = prune_tree(name)
    return _trees[name]


_surfaces = {}


def surface(name, level=-1):
    if (name, level) not in _surfaces:
        _surfaces[(name, level)] = dr.Surface(*tree(name), level)
    return _surfaces[(name, level)]


# (mode, amount, depth, level) per source: depth 3, 4 and 5 against sources four levels deep, delta of both signs and zero, the shell,
# and the level-2 surface.  The brute force costs points x triangles, so the depth-5 cases shrink the solid until little is left to
# refine -- which also puts every evaluated point far outside the stored field's band.
CASES = {
    "sphere_d4": [(G, 0.03, 3, -1), (G, -0.03, 3, -1), (G, 0.0, 3, -1), (SH, 0.05, 3, -1), (G, 0.03, 4, -1), (G, 0.03, 4, 2), (G, -0.25, 5, -1)],
    "torus_d4": [(G, 0.02, 4, -1), (G, -0.02, 3, -1), (SH, 0.04, 3, -1), (G, 0.0, 3, 2), (G, -0.07, 5, -1)],
    "carved": [(G, -0.03, 4, -1), (G, 0.03, 3, -1), (SH, 0.05, 3, -1), (G, 0.0, 4, 2), (G, -0.2, 5, -1)],
}
# The zoo's trees: random bytes cut nearly every leaf, so a result is nearly the full tree of its depth and the surface has up to
# 59 266 triangles.  The four small ones run depth 3, 4 and 5 at full detail (depth 5 shrunk, as above; blocks_257, 1 734 triangles,
# shrunk at depth 4 too) and at level 2.  On the six large ones every depth runs against the level-2 surface (some hundred
# triangles); against the full surface blocks_1017, _1025 and _2049 run depth 3, and dfs_d6_a (42 026 triangles), dfs_d6_b (59 266)
# and blocks_4097 (18 872) run depth 2 -- depth 3 is 5 500 points against every triangle, 20 to 65 s of numpy each -- with the finer
# entries into their searches left to the point queries of test_distance_bits_are_the_restatements (DESIGN.md N13 says so).
_LOD = [(G, 0.02, 3, 2), (G, 0.0, 4, 2), (G, -0.2, 5, 2)]
_D3 = [(G, 0.02, 3, -1), (G, -0.02, 3, -1), (SH, 0.03, 3, -1), (G, 0.0, 3, -1)]
_D2 = [(G, 0.02, 2, -1), (G, -0.02, 2, -1), (SH, 0.03, 2, -1), (G, 0.0, 2, -1)]
CASES["leaf"] = _D3 + _LOD + [(G, 0.02, 4, -1), (SH, 0.03, 4, -1), (G, -0.02, 5, -1), (G, 0.02, 6, -1)]
CASES["chain12"] = _D3 + _LOD + [(G, 0.02, 4, -1), (G, -0.15, 5, -1)]
CASES["blocks_65"] = _D3 + _LOD + [(G, -0.02, 4, -1), (G, -0.15, 5, -1)]
CASES["blocks_257"] = _D3 + _LOD + [(G, -0.1, 4, -1), (G, -0.25, 5, -1)]
for _name in ("blocks_1017", "blocks_1025", "blocks_2049"):
    CASES[_name] = _D3[:3] + _LOD
for _name in ("dfs_d6_a", "dfs_d6_b", "blocks_4097"):
    CASES[_name] = _D2 + _LOD
assert set(tree_zoo.MESHABLE) <= set(CASES)
BIG = ("leaf", (G, 0.02, 7, -1))


def restated(src, mode, amount, depth, level):
    """(structs, values, counts) of the restatement, made once per process and left unchanged"""
    return tree_zoo.restated(("offset", src, mode, float(amount), depth, level),
                             lambda: dr.offset(tree(src), mode, amount, depth, level, want_counts=True, surf=surface(src, level)))


def upload(sb, name, **kw):
    return sb.Scene(sb.OctData(*tree(name)), **kw)


def gpu_offset(scene, mode, amount, depth, level, **kw):
    return (scene.Shell if mode == SH else scene.Offset)(amount, depth, level, **kw)


@pytest.mark.parametrize("src", list(CASES))
def test_offset_and_shell_bytes_are_the_restatements(sb, src):
    with upload(sb, src) as scene:
        for mode, amount, depth, level in CASES[src]:
            S, V, counts = restated(src, mode, amount, depth, level)
            res, got, st = gpu_offset(scene, mode, amount, depth, level, want_octdata=True, want_stats=True)
            with res:
                what = f"{'shell' if mode == SH else 'offset'}({src}, {amount}) depth={depth} level={level}"
                assert_same_tree(got, S, V, what)
                assert (st.nodes_in, st.nodes_out, st.depth_out, st.levels) == (len(tree(src)[0]), len(S), counts["depth_out"], counts["levels"]), what
                assert st.points == counts["points"] and res.Length == len(S) and res.depth == st.depth_out and res.stack_kernel_ok, what
                assert st.visited >= 0 and (len(surface(src, level)) == 0 or st.visited >= st.points), what


def test_the_cases_are_what_they_are_for():
    assert [er.tree_depth(tree(s)[0]) for s in ("sphere_d4", "torus_d4", "carved")] == [4, 4, 4]
    for src in ("sphere_d4", "torus_d4", "carved"):
        deep = [c for c in CASES[src] if c[2] == 5]
        assert deep and all(restated(src, *c)[2]["depth_out"] == 5 for c in deep), "finer than the source"
        assert any(restated(src, *c)[2]["depth_out"] == 3 for c in CASES[src]) and any(c[3] == 2 for c in CASES[src])
        assert len(surface(src, 2)) and len(surface(src, 2)) < len(surface(src)) // 4
    # the carve took a bite out of the sphere: the solid is smaller, and its surface has the brush's concave sheet and a crease
    assert msr.measure(*tree("carved")).volume < 0.95 * msr.measure(*tree("sphere_d4")).volume
    # a grown solid has more inside corners than a shrunk one; a shell's centre is outside the wall
    grown, shrunk = restated("sphere_d4", G, 0.03, 3, -1), restated("sphere_d4", G, -0.03, 3, -1)
    assert (grown[1] <= 63).sum() > (shrunk[1] <= 63).sum() > 0
    # the zoo's trees keep their surfaces (random bytes: thousands of triangles in every direction)
    assert len(surface("dfs_d6_a")) > 10_000 and len(surface("chain12")) > 0 and len(surface("leaf")) > 0
    # every zoo tree runs depth 3, 4 and 5 and the level-2 surface; the small ones reach depth 4 and 5 against the full surface too
    for src in tree_zoo.MESHABLE:
        assert {3, 4, 5} <= {c[2] for c in CASES[src]} and any(c[3] == 2 for c in CASES[src])
        if len(surface(src, 2)) and src != "leaf":          # (the leaf's eight triangles leave most of the cube far away: it stops at 4)
            assert {restated(src, *c)[2]["depth_out"] for c in _LOD} == {3, 4, 5}, src
    for src in ("leaf", "chain12", "blocks_65", "blocks_257"):
        assert {restated(src, *c)[2]["depth_out"] for c in CASES[src] if c[3] < 0} >= {3, 4, 5}, src
    # the result's arrays start at max(1.5 x the source, 4096) nodes: the leaf's finer results make them grow
    assert len(restated("leaf", G, -0.02, 5, -1)[0]) > 4096 and len(restated("leaf", G, 0.02, 6, -1)[0]) > 4 * 4096


def test_offset_bytes_on_a_result_whose_arrays_grow(sb):
    src, case = BIG
    S, V, counts = restated(src, *case)
    level_sizes = [len(level) for level in pr.levels(S)]
    # the level loop under the offset's first pass where a small case does not reach: arrays that had to grow six times (they start at
    # 4096 nodes), a level that the first pass takes in more than one sweep of its grid (65 536 nodes), level lists that end inside
    # a workgroup (32 nodes).  (No level that is SCANNED is past the scan's chunk of 32 768 nodes: the last level is not scanned, and
    # a level behind such a level costs the brute force 20 s.  DESIGN.md N13 says so.)
    assert 32 * 4096 < len(S) < 200_000 and max(level_sizes) > 65536 and max(level_sizes[:-1]) < 32768, level_sizes
    assert any(m > 32 and m % 32 for m in level_sizes), level_sizes
    with upload(sb, src) as scene:
        res, got, st = gpu_offset(scene, *case, want_octdata=True, want_stats=True)
        with res:
            assert_same_tree(got, S, V, "offset(leaf) to depth 7")
            assert (st.nodes_out, st.depth_out, st.points) == (len(S), 7, counts["points"])


# ---- Distance --------------------------------------------------------------------------------------------------------------------
def lattice():
    """cell corners, face centres and cell centres of the depth-4 lattice on a coarse stride, and points outside the cube"""
    k = np.arange(0, 33, 4, dtype=np.float64) / 32                 # corners (multiples of 1/8) ...
    c = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
    faces = c[(c < 1).all(1)][::7] + [1 / 32, 1 / 32, 0]             # ... face centres of depth-4 cells
    centres = c[(c < 1).all(1)][::5] + 1 / 32
    outside = np.array([[-0.25, 0.5, 0.5], [1.5, 1.5, 1.5], [0.5, -3.0, 0.25], [2.0, 0.5, 0.5], [0.3, 0.3, 1.0001], [-1e-3, -1e-3, -1e-3],
                        [1e6, 0.5, 0.5], [1e30, 0.0, 0.0]])
    return np.concatenate([c, faces, centres, outside]).astype(f32)


def random_points(n=4096):
    p = np.random.default_rng(20260).random((n, 3)) * 1.2 - 0.1
    return p.astype(f32)


def records_differ(got, want):
    """indices where distance, node, nearest or status differ bit for bit (`visited` is not restated)"""
    bad = (got["distance"].view(np.uint32) != want["distance"].view(np.uint32)) | (got["node"] != want["node"]) | (got["status"] != want["status"])
    bad |= (got["nearest"].view(np.uint32) != want["nearest"].view(np.uint32)).any(1)
    bad |= got["pad_"] != 0
    return np.nonzero(bad)[0]


def restated_distance(src, which, level):
    pts = {"lattice": lattice, "random": random_points, "random400": lambda: random_points(400), "random1000": lambda: random_points(1000)}[which]()
    return pts, tree_zoo.restated(("distance", src, which, level), lambda: dr.distance(*tree(src), pts, surf=surface(src, level)))


@pytest.mark.parametrize("src, which, level", [("sphere_d4", "lattice", -1), ("sphere_d4", "random", -1), ("carved", "lattice", -1),
                                               ("carved", "random", 2), ("torus_d4", "lattice", 2), ("chain12", "lattice", -1),
                                               ("blocks_257", "lattice", -1), ("blocks_257", "random", -1), ("dfs_d6_a", "random400", -1),
                                               ("dfs_d6_b", "random400", 2), ("blocks_4097", "random1000", -1)])
def test_distance_bits_are_the_restatements(sb, src, which, level):
    pts, want = restated_distance(src, which, level)
    with upload(sb, src) as scene:
        got = scene.Distance(pts, level)
        bad = records_differ(got, want)
        assert not len(bad), (src, which, len(bad), [(pts[i].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:3]])
        assert (got["visited"][np.isfinite(got["distance"])] >= 1).all()
        # determinism: the same call again, bytes and the work measure alike
        again = scene.Distance(pts, level)
        assert got.tobytes() == again.tobytes()


def test_distance_device_form_bad_elements_and_an_empty_batch(sb):
    import torch
    pts, want = restated_distance("sphere_d4", "lattice", -1)
    pts = pts.copy()
    pts[3, 1], pts[10, 0], pts[11, 2] = np.nan, np.inf, -np.inf
    want = dr.distance(*tree("sphere_d4"), pts, surf=surface("sphere_d4"))
    assert (want["status"][[3, 10, 11]] == dr.INVALID).all() and (want["status"] == dr.HIT).sum() == len(pts) - 3
    with upload(sb, "sphere_d4") as scene:
        host = scene.Distance(pts)
        assert not len(records_differ(host, want))
        assert (host["visited"][[3, 10, 11]] == 0).all() and (host["nearest"][[3, 10, 11]] == 0).all()
        d_in = torch.from_numpy(pts).cuda()
        d_out = torch.zeros(len(pts) * 8, dtype=torch.int32, device="cuda")
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            scene.DistanceDevice(d_in.data_ptr(), len(pts), d_out.data_ptr(), stream=stream.cuda_stream)
            scene.DistanceDevice(d_in.data_ptr(), len(pts), d_out.data_ptr(), stream=stream.cuda_stream)     # (the bitmap is written again behind the first query)
        stream.synchronize()
        dev = d_out.cpu().numpy().view(dr.CLEARANCE)
        assert dev.tobytes() == host.tobytes()
        # n = 0: nothing is read or written, whatever the pointers
        assert scene.Distance(np.zeros((0, 3), f32)).shape == (0,)
        L = sb._lib
        assert L.lib.sdfhip_scene_distance(scene._h, None, 0, -1, None) == L.OK
        assert L.lib.sdfhip_scene_distance_device(scene._h, None, 0, -1, None, None) == L.OK


# ---- edges -----------------------------------------------------------------------------------------------------------------------
def test_an_empty_surface_and_a_surface_moved_out_of_the_cube(sb):
    L = sb._lib
    with upload(sb, "empty") as scene:
        got = scene.Distance([[0.5, 0.5, 0.5], [2.0, 0.0, 0.0]])
        assert (got["distance"] == np.inf).all() and (got["status"] == L.QUERY_HIT).all() and (got["node"] == 0).all() and (got["visited"] == 0).all()
        res, od = scene.Offset(0.1, 4, want_octdata=True)
        with res:
            assert_same_tree(od, *dr.grow(tree("empty"), 0.1, 4), "offset of an empty surface")
            assert od.Length == 1 and (od.Values == 255).all()
    with upload(sb, "sphere_d4") as scene:
        for delta in (2.0, -3.0):
            res, od = scene.Offset(delta, want_octdata=True)
            with res:
                assert od.Length == 1 and ((od.Values <= 63).all() if delta > 0 else (od.Values > 63).all())
                assert_same_tree(od, *dr.grow(tree("sphere_d4"), delta, 4, surf=surface("sphere_d4")), f"offset by {delta}")
        # host_out alone is an output; neither is refused
        raw = L.COctData()
        opt = sb.OffsetOptions(L.OFFSET_GROW, 0.03, 3)
        assert L.lib.sdfhip_scene_offset(scene._h, ctypes.byref(opt), None, ctypes.byref(raw), None) == L.OK
        assert raw.length == len(restated("sphere_d4", G, 0.03, 3, -1)[0])
        L.lib.sdfhip_octdata_free(ctypes.byref(raw))
        assert L.lib.sdfhip_scene_offset(scene._h, ctypes.byref(opt), None, None, None) == L.ERR_ARG


def test_the_same_offset_twice_gives_the_same_bytes_and_the_same_work(sb):
    with upload(sb, "carved") as scene:
        a = scene.Shell(0.05, 3, want_octdata=True, want_stats=True)
        b = scene.Shell(0.05, 3, want_octdata=True, want_stats=True)
        with a[0], b[0]:
            assert a[1].Structs.tobytes() == b[1].Structs.tobytes() and a[1].Values.tobytes() == b[1].Values.tobytes()
            assert a[2].visited == b[2].visited > 0 and a[2].points == b[2].points


def test_offset_chains_with_render_prune_combine_and_measure(sb, oracle_mod):
    W, H = 64, 48
    S, V, _ = restated("sphere_d4", G, 0.03, 4, -1)
    pruned = pr.prune(S, V, 0)
    cam = make_camera("rotated", W, H)
    with upload(sb, "sphere_d4") as scene:
        before = scene.Draw(cam, W, H)
        with scene.Offset(0.03, 4) as grown:
            assert_frames_identical(scene.Draw(cam, W, H), before, "the source after the call")
            ref, _ = oracle_mod.render(S, V, cam.State, W, H)
            assert_frames_identical(grown.Draw(cam, W, H), ref, "the grown sphere")
            m, want = grown.Measure(), msr.measure(S, V)
            assert msr.same_bits(np.array(m.volume), np.array(want.volume)) and msr.same_bits(np.array(m.area), np.array(want.area))
            assert msr.same_bits(np.array(list(m.moment1)), np.array(want.moment1)) and m.volume > scene.Measure().volume
            res, got = grown.Prune(0, None, want_octdata=True)
            with res:
                assert_same_tree(got, *pruned, "offset -> prune(0)")
            res, got = grown.Combine(scene, cr.COMBINE_SUBTRACT, want_octdata=True)
            with res:
                assert_same_tree(got, *cr.combine((S, V), tree("sphere_d4"), cr.COMBINE_SUBTRACT), "offset -> subtract the source")


def test_errors_are_status_codes(sb):
    L = sb._lib

    def call(scene, opt, want_out=True):
        h = ctypes.c_void_p()
        rc = L.lib.sdfhip_scene_offset(scene._h if scene is not None else None, ctypes.byref(opt) if opt is not None else None,
                                       ctypes.byref(h) if want_out else None, None, None)
        if h.value:
            L.lib.sdfhip_scene_free(h)
        assert rc == L.OK or not h.value, "*out is not null after a failure"
        return rc

    good = lambda **kw: sb.OffsetOptions(**dict(dict(mode=L.OFFSET_GROW, amount=0.03, depth=3, level=-1), **kw))
    W, H = 32, 24
    cam = make_camera("default", W, H)
    with upload(sb, "sphere_d4") as scene:
        before = scene.Draw(cam, W, H)
        assert call(scene, good()) == L.OK and call(scene, good(depth=0)) == L.OK and call(scene, good(mode=L.OFFSET_SHELL, level=12)) == L.OK
        assert call(None, good()) == L.ERR_ARG and call(scene, None) == L.ERR_ARG and call(scene, good(), want_out=False) == L.ERR_ARG
        for bad in (good(amount=float("nan")), good(amount=float("inf")), good(mode=L.OFFSET_SHELL, amount=0.0), good(mode=L.OFFSET_SHELL, amount=-0.1),
                    good(mode=2), good(mode=-1), good(depth=13), good(depth=-2), good(level=13), good(level=-2)):
            assert call(scene, bad) == L.ERR_ARG, (bad.mode, bad.amount, bad.depth, bad.level)
        small = good()
        small.size = 16
        assert call(scene, small) == L.ERR_ARG

        class Newer(ctypes.Structure):
            _fields_ = sb.OffsetOptions._fields_ + [("unknown", ctypes.c_int32)]
        newer = Newer()
        ctypes.memmove(ctypes.byref(newer), ctypes.byref(good()), 20)
        as_options = ctypes.cast(ctypes.pointer(newer), ctypes.POINTER(sb.OffsetOptions)).contents
        newer.size, newer.unknown = 24, 3
        assert call(scene, as_options) == L.ERR_ARG                     # an unknown field that is set
        newer.unknown = -1
        assert call(scene, as_options) == L.OK                          # ... and one that says "default"
        # the query's own refusals
        p = np.zeros((4, 3), f32)
        out = np.zeros(4, dr.CLEARANCE)
        D = L.lib.sdfhip_scene_distance
        assert D(None, p.ctypes.data, 4, -1, out.ctypes.data) == L.ERR_ARG and D(scene._h, None, 4, -1, out.ctypes.data) == L.ERR_ARG
        assert D(scene._h, p.ctypes.data, 4, -1, None) == L.ERR_ARG and D(scene._h, p.ctypes.data, 4, 13, out.ctypes.data) == L.ERR_ARG
        assert D(scene._h, p.ctypes.data, 4, -2, out.ctypes.data) == L.ERR_ARG
        assert L.lib.sdfhip_scene_distance_device(scene._h, None, 4, -1, None, None) == L.ERR_ARG
        assert_frames_identical(scene.Draw(cam, W, H), before, "the source after the refusals")
    # a source the mesh refuses: an inconsistent tree, and one deeper than twelve levels
    S0, V0 = tree("sphere_d4")
    Sb = S0.copy()
    Sb[int(S0[0, 1]) + 3, 0] = int(S0[0, 1])
    for arrays in ((Sb, V0), tree("chain14")):
        with sb.Scene(sb.OctData(*arrays)) as bad:
            before = bad.Draw(cam, W, H, sb.KERNEL_GENERIC)
            assert call(bad, good()) == L.ERR_BAD_TREE
            with pytest.raises(sb.SdfHipError) as e:
                bad.Distance(np.zeros((1, 3), f32))
            assert e.value.code == L.ERR_BAD_TREE
            assert_frames_identical(bad.Draw(cam, W, H, sb.KERNEL_GENERIC), before, "the refused source still renders")


def test_an_allocation_that_fails_is_nomem_and_leaves_the_source():
    # in a fresh process of its own, so that neither variable nor a failed call can reach the tests beside this one: every
    # allocation the offset and the host query reach fails once (k = 0, 1, ... until a call gets through), each is SDFHIP_ERR_NOMEM
    # with no handle, and afterwards the source renders as before and plain calls give the restatement's answers
    # (tests/distance_fault_child.py)
    S, V, _ = restated("sphere_d4", G, 0.03, 3, -1)
    pts = (np.random.default_rng(3).random((64, 3)) * 1.2 - 0.1).astype(f32)
    want = dr.distance(*tree("sphere_d4"), pts, surf=surface("sphere_d4"))["distance"]
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    child = os.path.join(REPO, "tests", "distance_fault_child.py")
    out = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    report = json.loads(out.stdout.strip().splitlines()[-1])
    # the bitmap, the counter, the two arrays, the blocks and the three scan buffers at the least; the query's three buffers
    assert report["codes_ok"] and 8 <= report["offset_failed"] < 64 and report["distance_failed"] == 3, report
    assert report["source_frame_unchanged"] and report["nodes_after"] == len(S), report
    assert report["structs_sha"] == sha(S) and report["values_sha"] == sha(V) and report["distance_sha"] == sha(want), report
    assert report["product_reads_no_variable"], report

"""Placement on the GPU (sdfhip_scene_place), both flavours of the library: the placed tree is the CPU restatement's
(tests/place_restatement.py) byte for byte -- every source, placement and depth below -- its statistics are the restatement's counts,
both cursor forms give the same bytes, its frames are the oracle's on the restated arrays, the source is untouched, a placement
chains with the combination and the prune as the restatements do, and the errors are status codes."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import combine_restatement as cr
import edit_restatement as er
import place_restatement as plr
import prune_restatement as pr
from conftest import REPO, assert_frames_identical, make_camera
from test_gpu_combine import tree
from test_gpu_prune import assert_same_tree

pytestmark = pytest.mark.gpu


def _placement(*args, **kw):
    import sdfbox_amd
    return sdfbox_amd.placement(*args, **kw)


# name -> (R, s, t): the identity; a dyadic translation (every look-up lands on the source's own lattice); a generic two-axis rotation
# at half size about the cube's centre; the same rotation at 0.62 (torus_d6 to depth 7: past the scan's chunk); an enlargement that
# pushes part of the source out of the cube, turned about all three axes; the source moved wholly outside; a mirror in x, moved
PLACEMENTS = {
    "identity": lambda: (plr.IDENTITY, 1.0, (0.0, 0.0, 0.0)),
    "dyadic": lambda: (plr.IDENTITY, 1.0, (0.25, 0.0, -0.125)),
    "generic_half": lambda: _placement(30, 20, 0, 0.5),
    "generic_062": lambda: _placement(30, 20, 0, 0.62),
    "enlarged": lambda: _placement(-40, 15, 65, 1.5, to=(0.8, 0.45, 0.6)),
    "outside": lambda: (plr.IDENTITY, 1.0, (3.0, 0.0, 0.0)),
    "mirror": lambda: (np.diag([-1.0, 1.0, 1.0]).astype(np.float32), 0.75, (0.95, 0.1, 0.2)),
}
SOURCES = ["leaf", "nine", "sphere_d4", "torus_edited", "torus_d6", "off_d7"]
# (source, placement, depth): depth -1 = the source's, "less" / "more" = one less / one more than the source's.  torus_edited is eight
# levels deep where it was edited: resampled to that depth everywhere it would have 1.3 M nodes, so it is placed to depth 6 and 7
CASES = ([(src, name, -1) for src in ("leaf", "nine", "sphere_d4") for name in ("identity", "dyadic", "generic_half")]
         + [("sphere_d4", name, -1) for name in ("enlarged", "outside", "mirror")]
         + [("torus_edited", "identity", 6), ("torus_edited", "generic_half", 7), ("torus_edited", "outside", -1)]
         + [("torus_d6", name, -1) for name in ("generic_half", "outside", "mirror")]
         + [("off_d7", "generic_half", -1), ("off_d7", "mirror", -1)]
         + [(src, "generic_half", depth) for src in ("nine", "sphere_d4", "torus_d6") for depth in (0, "less", "more")])
BIG = ("torus_d6", "generic_062", "more")


@pytest.fixture(scope="module", params=["product", "lab"])
def sb(request):
    import sdfbox_amd
    if request.param == "product":
        return sdfbox_amd
    import sdfbox_amd.lab
    return sdfbox_amd.lab.load()


_restated = {}


def depth_of(src, depth):
    own = er.tree_depth(tree(src)[0])
    return {"less": max(own - 1, 0), "more": own + 1}.get(depth, depth)


def restated(src, name, depth=-1):
    """(structs, values, counts) of the restatement, made once and left unchanged"""
    key = (src, name, depth_of(src, depth))
    if key not in _restated:
        _restated[key] = plr.place(tree(src), *PLACEMENTS[name](), key[2], want_counts=True)
    return _restated[key]


def upload(sb, name, **kw):
    return sb.Scene(sb.OctData(*tree(name)), **kw)


def gpu_place(scene, name, depth=-1, **kw):
    return scene.Place(*PLACEMENTS[name](), None if depth < 0 else depth, **kw)


def check_case(scene, src, name, depth):
    S, V, counts = restated(src, name, depth)
    d = depth_of(src, depth)
    res, got, st = gpu_place(scene, name, d, want_octdata=True, want_stats=True)
    with res:
        what = f"place({src}, {name}) depth={d}"
        assert_same_tree(got, S, V, what)
        assert (st.nodes_in, st.nodes_out, st.depth_out, st.levels) == (len(tree(src)[0]), len(S), counts["depth_out"], counts["levels"]), what
        assert st.samples == counts["samples"] and st.depth_out == er.tree_depth(S), what
        assert res.Length == len(S) and res.depth == st.depth_out and res.stack_kernel_ok, what


@pytest.mark.parametrize("src", SOURCES)
def test_placed_bytes_are_the_restatements(sb, src):
    with upload(sb, src) as scene:
        for s, name, depth in CASES:
            if s == src:
                check_case(scene, src, name, depth)


def test_the_cases_are_what_they_are_for():
    assert len(tree("nine")[0]) == 9 and len(tree("leaf")[0]) == 1
    assert [er.tree_depth(tree(s)[0]) for s in ("sphere_d4", "torus_d6", "off_d7", "torus_edited")] == [4, 6, 7, 8]
    for src in ("sphere_d4", "torus_d6", "torus_edited"):
        assert len(restated(src, "outside")[0]) == 1, "wholly outside: the root alone"
    for src in ("nine", "sphere_d4", "torus_d6"):
        assert len(restated(src, "generic_half", 0)[0]) == 1, "depth 0: the root alone"
    for src in ("sphere_d4", "torus_d6"):
        less, same, more = (restated(src, "generic_half", d) for d in ("less", -1, "more"))
        assert len(less[0]) < len(same[0]) < len(more[0])
        own = er.tree_depth(tree(src)[0])
        assert [x[2]["depth_out"] for x in (less, same, more)] == [own - 1, own, own + 1]
    # part of the enlarged source is outside the cube, part inside: some corner of the result is inside the solid, and the tree is
    # smaller than the same enlargement would be with room for all of it
    for src in ("sphere_d4",):
        S, V, _ = restated(src, "enlarged")
        assert len(S) > 1000 and (V <= 63).any()
        R, s, t = plr.as_placement(*PLACEMENTS["enlarged"]())
        corners = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.float64)
        where = float(s) * corners @ R.astype(np.float64).T + t
        assert (where < 0).any() or (where > 1).any(), "a corner of the source's cube lands outside"
    R = PLACEMENTS["mirror"]()[0]
    assert np.linalg.det(R) < 0
    # edit order in, breadth first out
    S_in = tree("torus_edited")[0]
    inner = np.nonzero(S_in[:, 1] >= 0)[0]
    assert not (S_in[inner, 1] == 1 + 8 * np.arange(len(inner))).all()
    S_out = restated("torus_edited", "identity", 6)[0]
    inner = np.nonzero(S_out[:, 1] >= 0)[0]
    assert (S_out[inner, 1] == 1 + 8 * np.arange(len(inner))).all()
    # level lists that end inside a workgroup of either pass: four blocks of eight siblings, 32 nodes (a wave of the first pass holds
    # one block, and no level but the root's ends inside one; eight lanes a node: a wave of the second holds eight nodes)
    blocks = [len(level) // 8 for level in pr.levels(restated("torus_d6", "generic_half")[0])]
    assert any(b > 4 and b % 4 for b in blocks), blocks


def test_placed_bytes_on_a_result_past_the_scans_chunk(sb):
    src, name, depth = BIG
    S, V, _ = restated(src, name, depth)
    level_sizes = [len(level) for level in pr.levels(S)]
    # past the scan's chunk (1024 words of 32 nodes) in two levels, a level that both passes take in more than one sweep of their
    # grids (65 536 nodes), a level list that ends inside a workgroup (32 nodes), and arrays that had to grow (they start at 1.5
    # times the source)
    assert 4 * 32768 < len(S) < 200_000 and sum(m > 32768 for m in level_sizes) >= 2 and max(level_sizes) > 65536, level_sizes
    assert any(m > 32 and m % 32 for m in level_sizes) and len(S) > 2 * (len(tree(src)[0]) * 3 // 2), level_sizes
    with upload(sb, src) as scene:
        check_case(scene, src, name, depth)


@pytest.mark.parametrize("src, name", [("torus_d6", "generic_half"), ("off_d7", "mirror"), ("sphere_d4", "enlarged")],
                         ids=["torus_d6-generic_half", "off_d7-mirror", "sphere_d4-enlarged"])
def test_both_cursor_forms_give_the_same_bytes(sb, src, name):
    S, V, _ = restated(src, name)
    with upload(sb, src) as with_grid, upload(sb, src, top_grid_level=0) as without:
        assert with_grid.stack_kernel_ok and with_grid.top_grid_level >= with_grid.depth and without.top_grid_level == 0
        for scene in (with_grid, without):
            res, got = gpu_place(scene, name, want_octdata=True)
            with res:
                assert_same_tree(got, S, V, f"place({src}, {name}), top grid level {scene.top_grid_level}")
    # a tree the upload calls inconsistent has no grid and no depth of its own: placed with a depth given, by the walk along the links
    S0, V0 = tree("sphere_d4")
    Sb = S0.copy()
    Sb[int(S0[0, 1]) + 3, 0] = int(S0[0, 1])
    want = plr.place((Sb, V0), *PLACEMENTS[name](), 4)
    with sb.Scene(sb.OctData(Sb, V0)) as bad:
        assert not bad.stack_kernel_ok
        res, got = gpu_place(bad, name, 4, want_octdata=True)
        with res:
            assert_same_tree(got, *want, "an inconsistent source with a depth given")
        with pytest.raises(sb.SdfHipError) as e:
            gpu_place(bad, name)
        assert e.value.code == sb._lib.ERR_BAD_TREE


def test_placed_frames_are_the_oracles_and_the_source_is_untouched(sb, oracle_mod):
    W, H = 64, 48
    src, name, depth = "torus_edited", "generic_half", 7
    S, V, _ = restated(src, name, depth)
    cams = [make_camera(cam, W, H) for cam in ("default", "rotated")]
    with upload(sb, src) as scene:
        before = [scene.Draw(cam, W, H) for cam in cams]
        res = gpu_place(scene, name, depth)
        for cam, frame in zip(cams, before):
            assert_frames_identical(scene.Draw(cam, W, H), frame, "the source after the call")
    # (the source is freed: the result stands alone)
    with res:
        for cam in cams:
            ref, _ = oracle_mod.render(S, V, cam.State, W, H)
            for flags in (sb.KERNEL_AUTO, sb.KERNEL_GENERIC):
                assert_frames_identical(res.Draw(cam, W, H, flags), ref, f"placed, flags {flags}")


def test_place_then_combine_then_prune(sb, oracle_mod):
    # the workflow the call exists for: a model placed at half size into a corner, united with another, the result tidied
    W, H = 64, 48
    corner = _placement(25, -35, 10, 0.5, to=(0.27, 0.27, 0.3))
    placed = plr.place(tree("torus_d6"), *corner)
    united = cr.combine(placed, tree("sphere_d4"), cr.COMBINE_UNION)
    pruned = pr.prune(*united, 0)
    assert len(placed[0]) > 1000 and len(united[0]) > len(placed[0]) and len(pruned[0]) < len(united[0])
    cam = make_camera("rotated", W, H)
    with upload(sb, "torus_d6") as torus, upload(sb, "sphere_d4") as sphere:
        with torus.Place(*corner) as p, p.Combine(sphere, cr.COMBINE_UNION) as u:
            res, got = u.Prune(0, None, want_octdata=True)
            with res:
                assert_same_tree(got, *pruned, "place -> combine -> prune(0)")
                ref, _ = oracle_mod.render(*pruned, cam.State, W, H)
                assert_frames_identical(res.Draw(cam, W, H), ref, "place -> combine -> prune(0)")


def test_a_placement_beside_frames_in_flight(sb):
    import torch
    W, H = 64, 48
    cam = make_camera("rotated", W, H)
    src, name, depth = "torus_edited", "generic_half", 7
    S, V, _ = restated(src, name, depth)
    with upload(sb, src) as scene:
        before = scene.Draw(cam, W, H)
        frames = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(6)]
        torch.cuda.synchronize()
        s_frames = torch.cuda.Stream()
        results = []
        for buf in frames:
            scene.DrawDevice(cam, W, H, buf.data_ptr(), stream=s_frames.cuda_stream)
            results.append(gpu_place(scene, name, depth, want_octdata=True))
        torch.cuda.synchronize()
        for buf in frames:
            assert_frames_identical(buf.cpu().numpy(), before, "a frame in flight beside a placement")
        for res, got in results:
            assert_same_tree(got, S, V, "one of several placements of the same source")
            res.close()


def test_errors_are_status_codes(sb):
    L = sb._lib

    def call(scene, pl, want_out=True):
        h = ctypes.c_void_p()
        rc = L.lib.sdfhip_scene_place(scene._h if scene is not None else None, ctypes.byref(pl) if pl is not None else None,
                                      ctypes.byref(h) if want_out else None, None, None)
        if h.value:
            L.lib.sdfhip_scene_free(h)
        assert rc == L.OK or not h.value, "*out is not null after a failure"
        return rc

    R, s, t = PLACEMENTS["generic_half"]()
    good = lambda **kw: sb.Placement(**dict(dict(rotation=R.tolist(), scale=s, translation=t.tolist()), **kw))
    with upload(sb, "sphere_d4") as scene:
        assert call(scene, good()) == L.OK and call(scene, good(depth=12)) == L.OK and call(scene, good(depth=0)) == L.OK
        assert call(None, good()) == L.ERR_ARG and call(scene, None) == L.ERR_ARG and call(scene, good(), want_out=False) == L.ERR_ARG
        for bad in (good(scale=0.0), good(scale=-1.0), good(scale=float("nan")), good(translation=(0.0, float("inf"), 0.0)),
                    good(rotation=((1, 0, 0), (0, 1, 0), (0, 0, 1.001))), good(rotation=((1, 2e-4, 0), (0, 1, 0), (0, 0, 1))),
                    good(depth=13), good(depth=-2)):
            assert call(scene, bad) == L.ERR_ARG, (bad.scale, list(bad.translation), bad.depth)
        small = good()
        small.size = 56
        assert call(scene, small) == L.ERR_ARG

        class Newer(ctypes.Structure):
            _fields_ = sb.Placement._fields_ + [("unknown", ctypes.c_int32)]
        newer = Newer()
        ctypes.memmove(ctypes.byref(newer), ctypes.byref(good()), 60)
        as_placement = ctypes.cast(ctypes.pointer(newer), ctypes.POINTER(sb.Placement)).contents
        newer.size, newer.unknown = 64, 3
        assert call(scene, as_placement) == L.ERR_ARG                   # an unknown field that is set
        newer.unknown = -1
        assert call(scene, as_placement) == L.OK                        # ... and one that says "default"
        # host_out alone is an output
        raw = L.COctData()
        assert L.lib.sdfhip_scene_place(scene._h, ctypes.byref(good()), None, ctypes.byref(raw), None) == L.OK
        assert raw.length == len(restated("sphere_d4", "generic_half")[0])
        L.lib.sdfhip_octdata_free(ctypes.byref(raw))


def test_an_allocation_that_fails_is_nomem_and_leaves_the_source():
    # in a fresh process of its own, so that neither the variable nor a failed call can reach the tests beside this one: every
    # allocation the call reaches fails once (k = 0, 1, ... until a call gets through), each is SDFHIP_ERR_NOMEM with no handle, and
    # afterwards the source renders as before and a plain call gives the restatement's tree (tests/place_fault_child.py)
    S, V, _ = restated("torus_d6", "generic_062", "more")
    child = os.path.join(REPO, "tests", "place_fault_child.py")
    out = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    report = json.loads(out.stdout.strip().splitlines()[-1])
    # the arrays start at 1.5 times the source and this result is four times the source: the growth's allocations are among them
    assert report["codes_ok"] and 9 <= report["failed"] < 64, report
    assert report["source_frame_unchanged"] and report["nodes_after"] == len(S), report
    assert report["structs_sha"] == plr_sha(S) and report["values_sha"] == plr_sha(V), report
    assert report["product_reads_no_variable"], report


def plr_sha(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()

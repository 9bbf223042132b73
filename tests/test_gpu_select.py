"""Selection on the GPU (sdfhip_scene_select), both flavours of the library: the selected tree is the CPU restatement's
(tests/select_restatement.py) byte for byte and the stats' integer fields are its counts -- every rule on the cases of
tests/select_cases.py; the lattices that are one bit, part of a word, exactly one word and eight words of the bitmaps; a changed zone
that crosses a word of them; a box that leaves the unit cube; result depths above and below the lattice's; every cursor form.  With no
rule the handle is Scene.Place's at the identity; Components of the result gives the pinned counts; two calls give the same bytes;
the source is untouched and may be freed; every refusal is a status code with its word and leaves `out` alone; Split gives the solids
one by one; the C++ mirror gives the same bytes.  Every tree is uploaded from arrays made on the CPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import components_cases as cs
import place_restatement as plr
import select_cases as sc
import select_restatement as sr
from conftest import REPO, assert_frames_identical, make_camera
from test_gpu_prune import assert_same_tree

pytestmark = pytest.mark.gpu

LATTICE = 5
INTEGERS = ("components", "solids", "flipped_solids", "flipped_voids", "points_flipped", "nodes_in", "nodes_out", "depth_out", "levels", "samples")


@pytest.fixture(scope="module", params=["product", "lab"])
def sb(request):
    import sdfbox_amd
    if request.param == "product":
        return sdfbox_amd
    import sdfbox_amd.lab
    return sdfbox_amd.lab.load()


def upload(sb, name, **kw):
    return sb.Scene(sb.OctData(*sc.tree(name)), **kw)


def arguments(name, rule_name, lattice_depth, box=sc.UNIT):
    flags, min_points, listed = sc.rule(name, rule_name, lattice_depth, box)
    return dict(keep_largest=bool(flags & sr.KEEP_LARGEST), drop_below=min_points if flags & sr.DROP_SMALL else 0,
                fill_enclosed=bool(flags & sr.FILL_ENCLOSED), flip=listed if flags & sr.FLIP_LISTED else None,
                keep=listed if flags & sr.KEEP_LISTED else None, lattice_depth=lattice_depth, origin=box[0], side=box[1])


def check_case(scene, name, rule_name, lattice_depth, depth, box=sc.UNIT):
    S, V, counts = sc.restated(name, rule_name, lattice_depth, depth, box)
    res, got, st = scene.Select(depth=depth, want_octdata=True, want_stats=True, **arguments(name, rule_name, lattice_depth, box))
    with res:
        what = f"select({name}, {rule_name}) lattice={lattice_depth} depth={depth}"
        assert_same_tree(got, S, V, what)
        assert {k: getattr(st, k) for k in INTEGERS} == {k: counts[k] for k in INTEGERS}, what
        assert res.Length == len(S) and res.depth == st.depth_out and res.stack_kernel_ok, what
        assert st.label_ms > 0 and st.kernel_ms > 0 and st.total_ms >= st.kernel_ms, what
    return counts


def phases(scene, lattice_depth, box=sc.UNIT):
    return cs.points_by_phase(scene.Components(depth=lattice_depth, origin=box[0], side=box[1])[0])


@pytest.mark.parametrize("name", ["crumbs", "hollow", "eight", "csg"])
def test_every_rule_is_the_restatements(sb, name):
    flipped = 0
    with upload(sb, name) as scene:
        for rule_name in ("keep_largest", "drop_small", "fill_enclosed", "flip_listed", "keep_listed", "keep_largest_and_fill"):
            flipped += check_case(scene, name, rule_name, LATTICE, sc.result_depth(name))["points_flipped"]
    assert flipped > 0


# (the eight points of the unit cube's depth-1 lattice all lie outside the sphere: that lattice is laid on a box that has the centre)
SMALL_LATTICES = [(0, sc.UNIT), (1, ((0.3, 0.3, 0.3), 0.8)), (2, sc.UNIT), (3, sc.UNIT)]


@pytest.mark.parametrize("lattice_depth, box", SMALL_LATTICES, ids=[str(d) for d, _ in SMALL_LATTICES])
def test_the_bitmaps_of_one_bit_part_of_a_word_one_word_and_eight(sb, lattice_depth, box):
    with upload(sb, "sphere_d4") as scene:
        assert len(phases(scene, lattice_depth, box)[0]) == 1
        counts = check_case(scene, "sphere_d4", "flip_the_one_solid", lattice_depth, 4, box)
        assert counts["flipped_solids"] == 1
        with scene.Select(**arguments("sphere_d4", "flip_the_one_solid", lattice_depth, box)) as res:
            assert phases(res, lattice_depth, box) == ([], [8 ** lattice_depth])


def test_a_changed_zone_across_a_word_of_the_bitmaps(sb):
    small = sc.straddle_small()             # (asserts that the small solid has points at x = 63 and x = 64 of the depth-7 lattice)
    with upload(sb, "straddle") as scene:
        counts = check_case(scene, "straddle", "keep_largest", sc.STRADDLE_DEPTH, 5)
        assert counts["points_flipped"] == small["points"]


def test_a_box_that_leaves_the_unit_cube(sb):
    with upload(sb, "eight") as scene:
        for rule_name in ("keep_largest", "flip_listed"):
            assert check_case(scene, "eight", rule_name, cs.OFF_CUBE_DEPTH, 5, sc.OFF_CUBE)["points_flipped"] > 0


@pytest.mark.parametrize("depth", [3, 6])
def test_a_result_depth_below_and_above_the_lattices(sb, depth):
    with upload(sb, "crumbs") as scene:
        check_case(scene, "crumbs", "keep_largest", LATTICE, depth)


def test_every_cursor_form_gives_the_same_bytes(sb):
    name, rule_name = "hollow", "fill_enclosed"
    S, V, _ = sc.restated(name, rule_name, LATTICE, 5)
    with upload(sb, name) as with_grid, upload(sb, name, top_grid_level=0) as without:
        assert with_grid.stack_kernel_ok and with_grid.top_grid_level >= with_grid.depth and without.top_grid_level == 0
        for scene in (with_grid, without):
            check_case(scene, name, rule_name, LATTICE, 5)
    # a tree the upload calls inconsistent has no grid and no depth of its own: selected with a depth given, by the walk along the links
    S0, V0 = sc.tree("sphere_d4")
    Sb = S0.copy()
    Sb[int(S0[0, 1]) + 3, 0] = int(S0[0, 1])
    want = sr.select((Sb, V0), sr.KEEP_LARGEST, (), 3, depth=4)
    with sb.Scene(sb.OctData(Sb, V0)) as bad:
        assert not bad.stack_kernel_ok
        res, got = bad.Select(keep_largest=True, lattice_depth=3, depth=4, want_octdata=True)
        with res:
            assert_same_tree(got, *want, "an inconsistent source with a depth given")
        with pytest.raises(sb.SdfHipError, match="no depth") as e:
            bad.Select(keep_largest=True, lattice_depth=3)
        assert e.value.code == sb._lib.ERR_BAD_TREE


def test_no_rule_is_place_at_the_identity_and_components_of_the_results_are_the_pinned_counts(sb):
    with upload(sb, "crumbs") as scene:
        placed, want = scene.Place(plr.IDENTITY, 1.0, (0.0, 0.0, 0.0), want_octdata=True)
        res, got = scene.Select(lattice_depth=LATTICE, want_octdata=True)
        with placed, res:
            assert_same_tree(got, want.Structs, want.Values, "no rule against Place at the identity")
            assert phases(res, LATTICE) == ([735, 17, 1], [32015])
        with scene.KeepLargest(lattice_depth=LATTICE) as res:
            assert phases(res, LATTICE) == ([735], [32033])
    with upload(sb, "hollow") as scene, scene.FillCavities(lattice_depth=LATTICE) as res:
        assert phases(scene, LATTICE) == ([3064], [29272, 432]) and phases(res, LATTICE) == ([3496], [29272])
    with upload(sb, "eight") as scene, scene.KeepLargest(lattice_depth=LATTICE) as res:
        assert phases(res, LATTICE) == ([202], [32566])
    with upload(sb, "csg") as scene, scene.KeepLargest(lattice_depth=LATTICE, depth=6) as res:
        assert phases(scene, LATTICE) == ([794, 2, 2], [31970]) and phases(res, LATTICE) == ([794], [31974])


def test_two_calls_give_the_same_bytes_and_the_source_is_untouched_and_may_be_freed(sb):
    W, H = 64, 48
    cam = make_camera("default", W, H)
    S, V, _ = sc.restated("crumbs", "keep_largest", LATTICE, 5)
    scene = upload(sb, "crumbs")
    before = scene.Draw(cam, W, H)
    first, first_od = scene.KeepLargest(lattice_depth=LATTICE, want_octdata=True)
    second, second_od = scene.KeepLargest(lattice_depth=LATTICE, want_octdata=True)
    assert_frames_identical(scene.Draw(cam, W, H), before, "crumbs after the calls")
    scene.close()
    # the source is freed: the results stand alone
    with first, second:
        assert_same_tree(first_od, S, V, "the first call")
        assert_same_tree(second_od, S, V, "the second call")
        assert_frames_identical(first.Draw(cam, W, H), second.Draw(cam, W, H), "the two results")


def test_every_refusal_is_a_status_code_with_its_word_and_leaves_out_alone(sb):
    L = sb._lib
    sentinel = 0x5EED

    def call(scene, opt, labels=None, n=None, want_out=True, want_host=False):
        h = ctypes.c_void_p(sentinel)
        raw = L.COctData()
        arr = None if labels is None else np.asarray(labels, dtype=np.uint32)
        rc = L.lib.sdfhip_scene_select(scene._h if scene is not None else None, ctypes.byref(opt) if opt is not None else None,
                                       arr.ctypes.data if arr is not None and len(arr) else None, (0 if arr is None else len(arr)) if n is None else n,
                                       ctypes.byref(h) if want_out else None, ctypes.byref(raw) if want_host else None, None)
        message = L.lib.sdfhip_last_error().decode("utf-8", "replace")
        if rc == L.OK:
            assert h.value != sentinel
            L.lib.sdfhip_scene_free(h)
        else:
            assert h.value == sentinel and not raw.length, "an output was touched by a refused call"
        return rc, message

    def refused(word, *args, code=None, **kw):
        rc, message = call(*args, **kw)
        assert rc == (L.ERR_ARG if code is None else code) and word in message, (rc, message, word)

    good = lambda **kw: sb.SelectOptions(**dict(dict(lattice_depth=LATTICE), **kw))
    rec, lab = sc.labelled("hollow", LATTICE)
    solid, void = int(sc.solids(rec)[0]["label"]), int(sc.enclosed_voids(rec, LATTICE)[0]["label"])
    other = int(np.nonzero(lab.reshape(-1) == solid)[0][1])              # a point of the solid that is not its label
    with upload(sb, "hollow") as scene:
        assert call(scene, good())[0] == L.OK and call(scene, None)[0] == L.OK and call(scene, good(depth=7, flags=sr.FILL_ENCLOSED))[0] == L.OK
        assert call(scene, good(flags=sr.FLIP_LISTED), [void, solid, void])[0] == L.OK and call(scene, good(flags=sr.KEEP_LISTED), [solid])[0] == L.OK
        refused("null scene", None, good())
        refused("both outputs", scene, good(), want_out=False)
        refused("unknown flags", scene, good(flags=32))
        refused("both FLIP_LISTED and KEEP_LISTED", scene, good(flags=sr.FLIP_LISTED | sr.KEEP_LISTED), [solid])
        refused("no labels", scene, good(flags=sr.FLIP_LISTED))
        refused("no labels", scene, good(flags=sr.KEEP_LISTED), [], n=3)            # a count and a null list
        refused("without a listed rule", scene, good(flags=sr.KEEP_LARGEST), [solid])
        refused("lattice_depth", scene, good(lattice_depth=10))
        refused("origin", scene, good(origin=(0.0, float("nan"), 0.0)))
        refused("side", scene, good(side=0.0))
        refused("side", scene, good(side=float("inf")))
        refused("far corner", scene, good(origin=(3e38, 0.0, 0.0), side=3e38))
        refused("depth", scene, good(depth=13))
        refused("depth", scene, good(depth=-2))
        small = good()
        small.size = 32
        refused("options of 32 bytes", scene, small)
        # after the labelling pass: nothing is built, and the label is named
        refused(f"label {other} is not the label", scene, good(flags=sr.FLIP_LISTED), [solid, other])
        refused(f"label {8 ** LATTICE} is not the label", scene, good(flags=sr.KEEP_LISTED), [8 ** LATTICE, solid])
        refused(f"label {void} is a void", scene, good(flags=sr.KEEP_LISTED), [solid, void])
        # host_out alone is an output
        raw = L.COctData()
        assert L.lib.sdfhip_scene_select(scene._h, ctypes.byref(good(flags=sr.FILL_ENCLOSED)), None, 0, None, ctypes.byref(raw), None) == L.OK
        assert raw.length == len(sc.restated("hollow", "fill_enclosed", LATTICE, 5)[0])
        L.lib.sdfhip_octdata_free(ctypes.byref(raw))
        with pytest.raises(ValueError):
            scene.Select(flip=[solid], keep=[solid])


def test_split_gives_the_solids_of_eight_one_by_one(sb):
    rec, _ = sc.labelled("eight", LATTICE)
    labels = [int(r["label"]) for r in rec if r["flags"] == sb.COMPONENT_SOLID]
    with upload(sb, "eight") as scene:
        parts = scene.Split(lattice_depth=LATTICE)
        try:
            assert len(parts) == 8
            for label, part in zip(labels, parts):
                got, _, lab = part.Components(depth=LATTICE, labels=True)
                assert cs.points_by_phase(got) == ([202], [8 ** LATTICE - 202])
                assert int(got[got["flags"] == sb.COMPONENT_SOLID][0]["label"]) == label, "the parts come in label order"
        finally:
            for part in parts:
                part.close()
        with pytest.raises(ValueError, match="max_parts"):
            scene.Split(lattice_depth=LATTICE, max_parts=7)


def test_the_cpp_mirror_gives_the_same_bytes(tmp_path):
    # Program::Select (include/sdfbox.hpp) on the depth-4 sphere: its one solid flipped, the restatement's bytes (tests/cpp_select.cpp)
    import shutil
    from conftest import GOLDEN
    lattice_depth = 3
    exe, libdir = str(tmp_path / "cpp_select"), os.path.join(REPO, "sdfbox_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "cpp_select.cpp"),
                           "-o", exe, "-L", libdir, "-lsdfhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    shutil.copy(os.path.join(GOLDEN, "sphere_d4.asdf"), tmp_path / "sphere.asdf")
    out = subprocess.run([exe, str(tmp_path / "sphere.asdf"), str(lattice_depth), str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "argument checks ok" in out.stderr, (out.returncode, out.stderr)
    S, V, _ = sc.restated("sphere_d4", "flip_the_one_solid", lattice_depth, 4)
    assert np.fromfile(tmp_path / "out.structs", dtype=np.int32).tobytes() == S.tobytes()
    assert np.fromfile(tmp_path / "out.values", dtype=np.uint8).tobytes() == V.tobytes()

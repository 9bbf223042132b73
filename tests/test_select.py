"""tests/select_restatement.py held to things it did not come from: the counts pinned from a prototype of the rule, the identity
placement, the invariance of the links, the agreement of two rules that name the same component, and what the call refuses after its
labelling pass; and the library itself to what it refuses before any device call, with `out` left alone, and tests/cpp_select.cpp to
its argument checks.  No GPU is needed.  Everything is an integer or a byte: every comparison is exact."""
import numpy as np
import pytest

import components_cases as cs
import components_restatement as cpr
import place_restatement as plr
import select_cases as sc
import select_restatement as sr
from trimesh_restatement import CORNER, from_float

LATTICE = 5

# case, rule -> (solids, voids) before and after, descending: pinned from a numpy prototype of the rule
PINNED = [
    ("crumbs", "keep_largest", ([735, 17, 1], [32015]), ([735], [32033])),
    ("hollow", "fill_enclosed", ([3064], [29272, 432]), ([3496], [29272])),
    ("eight", "keep_largest", ([202] * 8, [31152]), ([202], [32566])),
    ("csg", "keep_largest", ([794, 2, 2], [31970]), ([794], [31974])),
]


def targets(name, rule_name):
    flags, min_points, listed = sc.rule(name, rule_name, LATTICE)
    return sr.targets(sc.tree(name), flags, LATTICE, min_points=min_points, listed=listed, labelled=sc.labelled(name, LATTICE))


def identity(name):
    return plr.place(sc.tree(name), plr.IDENTITY, 1.0, (0.0, 0.0, 0.0), sc.result_depth(name))


def node_corners(structs):
    """(n, 8, 3) integer corner coordinates of every node in units of its own edge, and (n,) its depth: from the links alone"""
    n = len(structs)
    coords, depth = np.zeros((n, 3), np.int64), np.zeros(n, np.int64)
    for k in np.nonzero(structs[:, 1] >= 0)[0]:                       # breadth first: a parent comes before its children
        c = int(structs[k, 1])
        coords[c:c + 8] = 2 * coords[k] + CORNER
        depth[c:c + 8] = depth[k] + 1
    return coords[:, None, :] + CORNER[None], depth


@pytest.mark.parametrize("name, rule_name, before, after", PINNED, ids=[p[0] for p in PINNED])
def test_the_pinned_counts_and_the_result_has_the_target_phase_at_every_lattice_point(name, rule_name, before, after):
    # (csg is a depth-6 tree: the identity placement at depth 5 already moves 166 lattice phases on its own, so it is built to 6,
    # where it has mixed near-contact points and still ends with no mismatch)
    assert cs.points_by_phase(sc.labelled(name, LATTICE)[0]) == before
    S, V, counts = sc.restated(name, rule_name, LATTICE, sc.result_depth(name))
    _, T, lattice_counts = targets(name, rule_name)
    got = cpr.inside((S, V), LATTICE)
    assert int((got != T).sum()) == 0
    assert cs.points_by_phase(cpr.records(got, cpr.label(got))) == after
    assert counts["solids"] == len(before[0]) and counts["components"] == len(before[0]) + len(before[1])
    assert counts["flipped_solids"] + counts["flipped_voids"] == counts["components"] - len(after[0]) - len(after[1])
    assert counts["points_flipped"] == abs(sum(before[0]) - sum(after[0])) and {k: counts[k] for k in lattice_counts} == lattice_counts


@pytest.mark.parametrize("name, rule_name", [("crumbs", "none"), ("hollow", "drop_small"), ("eight", "fill_enclosed")])
def test_a_call_that_flips_nothing_is_the_identity_placement_byte_for_byte(name, rule_name):
    S, V, counts = sc.restated(name, rule_name, LATTICE, sc.result_depth(name))
    want_S, want_V, want = plr.place(sc.tree(name), plr.IDENTITY, 1.0, (0.0, 0.0, 0.0), sc.result_depth(name), want_counts=True)
    assert counts["flipped_solids"] == counts["flipped_voids"] == counts["points_flipped"] == 0
    assert S.tobytes() == want_S.tobytes() and V.tobytes() == want_V.tobytes()
    assert {k: counts[k] for k in want} == want


@pytest.mark.parametrize("name, rule_name", [("crumbs", "keep_largest"), ("hollow", "fill_enclosed"), ("eight", "keep_listed"), ("csg", "drop_small")])
def test_the_links_are_the_identity_placements_and_bytes_differ_only_in_changed_zones(name, rule_name):
    S, V, counts = sc.restated(name, rule_name, LATTICE, sc.result_depth(name))
    want_S, want_V = identity(name)
    assert counts["points_flipped"] > 0 and S.tobytes() == want_S.tobytes()
    differs = (V != want_V).any(1)
    assert differs.any()
    # a node's corner is in a changed zone iff some lattice point with non-zero trilinear weight there flips
    F, _, _ = targets(name, rule_name)
    corners, depth = node_corners(S)
    p = (corners[differs].reshape(-1, 3) * (2.0 ** -depth[differs]).repeat(8)[:, None]).astype(np.float32)
    (x0, x1), (y0, y1), (z0, z1) = sr.neighbours(p, LATTICE, *sc.UNIT)
    near = np.zeros(len(p), bool)
    for z in (z0, z1):
        for y in (y0, y1):
            for x in (x0, x1):
                near |= F[z, y, x]
    assert near.reshape(-1, 8).any(1).all()


def test_keep_listed_on_each_solid_of_eight_gives_eight_scenes_of_one_solid():
    rec, _ = sc.labelled("eight", LATTICE)
    labels = [int(r["label"]) for r in rec if r["flags"] == cpr.SOLID]
    assert len(labels) == 8
    memo, total = {}, 0
    for label in labels:
        S, V, counts = sr.select(sc.tree("eight"), sr.KEEP_LISTED, [label], LATTICE, depth=5, want_counts=True, labelled=(rec, sc.labelled("eight", LATTICE)[1]),
                                 memo=memo)
        assert (counts["flipped_solids"], counts["flipped_voids"]) == (7, 0)
        got = cpr.inside((S, V), LATTICE)
        solids, voids = cs.points_by_phase(cpr.records(got, cpr.label(got)))
        assert len(solids) == 1 and len(voids) == 1
        assert got.reshape(-1)[label], "the kept solid is where its label is"
        total += solids[0]
    assert total == int(rec["points"][rec["flags"] == cpr.SOLID].sum()) == 8 * 202


def test_flip_listed_of_a_crumb_is_drop_small_with_a_threshold_that_selects_it():
    rec, lab = sc.labelled("crumbs", LATTICE)
    crumb = sc.solids(rec)[-1]
    assert crumb["points"] == 1 and sorted(sc.solids(rec)["points"]) == [1, 17, 735]
    memo = {}
    listed = sr.select(sc.tree("crumbs"), sr.FLIP_LISTED, [int(crumb["label"])] * 3, LATTICE, depth=5, want_counts=True, labelled=(rec, lab), memo=memo)
    dropped = sr.select(sc.tree("crumbs"), sr.DROP_SMALL, (), LATTICE, depth=5, min_points=2, want_counts=True, labelled=(rec, lab), memo=memo)
    assert listed[0].tobytes() == dropped[0].tobytes() and listed[1].tobytes() == dropped[1].tobytes() and listed[2] == dropped[2]
    assert listed[2]["points_flipped"] == 1 and listed[1].tobytes() != identity("crumbs")[1].tobytes()
    # ... and the rule bits are OR-ed: both crumbs by either route
    both = sr.select(sc.tree("crumbs"), sr.FLIP_LISTED | sr.DROP_SMALL, [int(crumb["label"])], LATTICE, depth=5, min_points=18, labelled=(rec, lab), memo=memo)
    largest = sc.restated("crumbs", "keep_largest", LATTICE, 5)
    assert both[0].tobytes() == largest[0].tobytes() and both[1].tobytes() == largest[1].tobytes()


def test_what_the_call_refuses_after_its_labelling_pass():
    rec, lab = sc.labelled("hollow", LATTICE)
    void = int(sc.enclosed_voids(rec, LATTICE)[0]["label"])
    solid = int(sc.solids(rec)[0]["label"])
    other = int(np.nonzero(lab.reshape(-1) == solid)[0][1])              # a point of the solid that is not its label
    for flags, listed, word in ((sr.FLIP_LISTED, [other], "not the label"), (sr.KEEP_LISTED, [8 ** LATTICE], "not the label"),
                                (sr.KEEP_LISTED, [solid, void], "void")):
        with pytest.raises(ValueError, match=word):
            sr.decide(rec, flags, LATTICE, 0, listed)
    assert sr.decide(rec, sr.FLIP_LISTED, LATTICE, 0, [void, solid]).tolist() == [(r["label"] in (void, solid)) for r in rec]


def test_h_reads_as_outside_at_every_level_and_leaves_the_split_rule_alone_down_to_level_eight():
    for d in range(13):
        S = np.float32(2.0 ** -d)
        assert int(from_float(np.array([sr.H], np.float32), S)[0]) >= 64 and int(from_float(np.array([-sr.H], np.float32), S)[0]) <= 63
    assert all(sr.H < np.float32(2.0) * np.float32(2.0 ** -d) for d in range(9)) and not sr.H < np.float32(2.0) * np.float32(2.0 ** -9)


def test_the_library_refuses_before_any_device_call_and_leaves_out_alone():
    # (no GPU is needed: the null scene is the last thing the call looks at)
    import ctypes
    import sdfbox_amd as sb
    L = sb._lib
    opt = sb.SelectOptions()
    ctypes.memset(ctypes.byref(opt), 0xEE, ctypes.sizeof(opt))
    L.lib.sdfhip_select_options_default(ctypes.byref(opt))
    assert (opt.size, opt.flags, opt.lattice_depth, list(opt.origin), opt.side, opt.depth, opt.min_points) == (36, 0, 6, [0.0, 0.0, 0.0], 1.0, -1, 0)
    assert (sb.SELECT_KEEP_LARGEST_SOLID, sb.SELECT_DROP_SMALL_SOLIDS, sb.SELECT_FILL_ENCLOSED_VOIDS, sb.SELECT_FLIP_LISTED, sb.SELECT_KEEP_LISTED) == \
        (sr.KEEP_LARGEST, sr.DROP_SMALL, sr.FILL_ENCLOSED, sr.FLIP_LISTED, sr.KEEP_LISTED)
    labels = np.array([3, 1, 3], np.uint32)
    for word, kw, listed, want_out in (("both outputs", {}, None, False), ("unknown flags", dict(flags=64), None, True),
                                       ("both FLIP_LISTED and KEEP_LISTED", dict(flags=24), labels, True), ("no labels", dict(flags=8), None, True),
                                       ("without a listed rule", dict(flags=1), labels, True), ("lattice_depth", dict(lattice_depth=10), None, True),
                                       ("side", dict(side=-1.0), None, True), ("origin", dict(origin=(float("inf"), 0, 0)), None, True),
                                       ("depth", dict(depth=13), None, True), ("null scene", dict(flags=16), labels, True)):
        h = ctypes.c_void_p(0x5EED)
        rc = L.lib.sdfhip_scene_select(None, ctypes.byref(sb.SelectOptions(**kw)), None if listed is None else listed.ctypes.data,
                                       0 if listed is None else len(listed), ctypes.byref(h) if want_out else None, None, None)
        assert rc == L.ERR_ARG and word in L.lib.sdfhip_last_error().decode() and h.value == 0x5EED, (word, rc, L.lib.sdfhip_last_error())


def test_the_cpp_mirror_checks_its_arguments_and_fails_loudly_without_a_gpu(tmp_path):
    # Program::Select (include/sdfbox.hpp) through tests/cpp_select.cpp: what it refuses needs no GPU; with one the bytes are
    # tests/test_gpu_select.py's
    import os
    import shutil
    import subprocess
    import torch
    from conftest import GOLDEN, REPO
    exe, libdir = str(tmp_path / "cpp_select"), os.path.join(REPO, "sdfbox_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "cpp_select.cpp"),
                           "-o", exe, "-L", libdir, "-lsdfhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    shutil.copy(os.path.join(GOLDEN, "sphere_d4.asdf"), tmp_path / "sphere.asdf")
    out = subprocess.run([exe, str(tmp_path / "sphere.asdf"), "3", str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert "argument checks ok" in out.stderr, (out.returncode, out.stderr)
    if torch.cuda.is_available():
        assert out.returncode == 0, out.stderr
    else:
        assert out.returncode == 3 and "sdfhip:" in out.stderr, (out.returncode, out.stderr)

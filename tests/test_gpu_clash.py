"""The clash check on the GPU (sdfhip_instances_clash), both flavours of the library: every case of tests/clash_cases.py gives the
CPU restatement's records (tests/clash_restatement.py) byte for byte -- they are integers throughout -- with the exact skip on and
off, at the depths where the lattice is less than, exactly and more than one 4 x 4 x 4 block, on a box that leaves the unit cube, at
every capacity; the stats count what they say; a path that exists already (Scene.SampleParts of the pair's intersection) counts the
same points; the sources are untouched and may be freed; two calls give the same bytes; an allocation that fails is
SDFHIP_ERR_NOMEM; the C++ mirror gives the same bytes."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import clash_cases as ca
import clash_restatement as clr
import compose_cases as cc
import compose_restatement as cr
from conftest import REPO, assert_frames_identical, make_camera
from test_gpu_compose import Uploaded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["product", "lab"])
def sb(request):
    import sdfbox_amd
    if request.param == "product":
        return sdfbox_amd
    import sdfbox_amd.lab
    return sdfbox_amd.lab.load()


def same_bytes(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def check_stats(st, depth, K, skip):
    points = 8 ** depth
    assert st.points == points and st.blocks == 8 ** max(depth - 2, 0) and st.blocks_looked <= st.blocks, (depth, K, skip)
    if skip:
        assert st.lookups <= points * K
    else:
        assert st.lookups == points * K and st.blocks_looked == st.blocks


@pytest.mark.parametrize("name, depth", ca.RUNS)
def test_every_case_is_the_restatements(sb, name, depth):
    parts = ca.parts(name)
    want = ca.restated(name, depth)
    with Uploaded(sb, parts) as up:
        for skip in (True, False):
            got, st = sb.Scene.ClashParts(up.parts(parts), depth=depth, skip=skip)
            assert same_bytes(got, want), (name, depth, skip, got, want)
            check_stats(st, depth, len(parts), skip)


@pytest.mark.parametrize("depth", [0, 1, 2, 3])
def test_less_than_one_block_exactly_one_and_eight(sb, depth):
    # depth 0: one lane; depth 1: eight lanes; depth 2: exactly one block; depth 3: eight blocks in two workgroups.  The source's own
    # sphere (radius 0.3 round the cube's centre) three times over: every point inside it is in all three pairs -- the cube's centre
    # at depth 0, none of the eight points at depth 1, the inner eight at depth 2
    parts = [("sphere_d4", cc.ONE_PLACEMENTS["identity"](), cr.COMBINE_UNION)] * 3
    want = clr.clash(cr.as_instances(cc.with_trees(parts)), depth)
    assert len(want) == (0 if depth == 1 else 3) and (depth != 2 or (want["points"] == 8).all())
    with Uploaded(sb, parts) as up:
        for skip in (True, False):
            got, st = sb.Scene.ClashParts(up.parts(parts), depth=depth, skip=skip)
            assert same_bytes(got, want), (depth, skip, got, want)
            check_stats(st, depth, 3, skip)


def test_a_box_that_leaves_the_unit_cube(sb):
    parts = ca.parts("csg")
    origin, side = ca.OFF_CUBE
    want = ca.restated("csg", ca.OFF_CUBE_DEPTH, ca.OFF_CUBE)
    assert len(want) >= 1
    with Uploaded(sb, parts) as up:
        for skip in (True, False):
            got, _ = sb.Scene.ClashParts(up.parts(parts), depth=ca.OFF_CUBE_DEPTH, origin=origin, side=side, skip=skip)
            assert same_bytes(got, want), (skip, got, want)


def test_capacity_zero_one_and_exact(sb):
    L = sb._lib
    parts, depth = ca.parts("csg"), 5
    want = ca.restated("csg", depth)
    assert len(want) == 3
    with Uploaded(sb, parts) as up:
        _, arr = sb.Scene._instances("test", up.parts(parts))
        opt = sb.ClashOptions(depth=depth)
        n = ctypes.c_uint32(77)
        assert L.lib.sdfhip_instances_clash(arr, 3, ctypes.byref(opt), None, 0, ctypes.byref(n), None) == L.OK and n.value == 3
        for capacity in (1, 3, 5):
            out = np.frombuffer(bytes([0xEE]) * (5 * 64), dtype=clr.CLASH).copy()
            n = ctypes.c_uint32(77)
            assert L.lib.sdfhip_instances_clash(arr, 3, ctypes.byref(opt), out.ctypes.data, capacity, ctypes.byref(n), None) == L.OK
            k = min(capacity, 3)
            assert n.value == 3 and same_bytes(out[:k], want[:k]) and (out[k:].view(np.uint8) == 0xEE).all(), capacity
        # one instance: a success with no pair; NULL options are the defaults
        n = ctypes.c_uint32(77)
        assert L.lib.sdfhip_instances_clash(arr, 1, None, None, 0, ctypes.byref(n), None) == L.OK and n.value == 0
        st = sb.ClashStats()
        assert L.lib.sdfhip_instances_clash(arr, 3, None, None, 0, ctypes.byref(n), ctypes.byref(st)) == L.OK
        assert n.value == len(ca.restated("csg", 6)) and st.points == 8 ** 6


def test_the_stats_count_what_they_say(sb):
    for name, depth in (("far", 5), ("csg", 5), ("two_spheres", 5), ("one", 3)):
        parts = ca.parts(name)
        with Uploaded(sb, parts) as up:
            _, on = sb.Scene.ClashParts(up.parts(parts), depth=depth)
            _, off = sb.Scene.ClashParts(up.parts(parts), depth=depth, skip=False)
        check_stats(on, depth, len(parts), True)
        check_stats(off, depth, len(parts), False)
        if name in ("far", "one"):
            # nothing but the torus reaches the cube, or there is one part only: no block has two candidates, nothing is looked up
            assert on.lookups == 0 and on.blocks_looked == 0, name
        elif name == "csg":
            # the half-size sphere's cube begins at x = 0.47 and its bound turns positive 0.5625 * 0.5 before it: the points with
            # x < 0.18 do not look it up.  (The torus and the large sphere are candidates everywhere: every block looks something up.)
            assert 0 < on.lookups < off.lookups
        else:
            # the first sphere's cube ends at x = 0.55, its bound turns positive at 0.55 + 0.5625 * 0.5 < 0.875: the blocks of the
            # last x layer have one candidate and look nothing up; the blocks between the two cubes have two
            assert 0 < on.lookups < off.lookups and 0 < on.blocks_looked <= on.blocks - 64


def test_the_pairs_intersection_sampled_counts_the_same_points(sb):
    # a path that exists already: Scene.SampleParts of [a, (b, INTERSECT)] on the same lattice
    depth = 5
    parts = ca.parts("csg")
    p = clr.lattice(depth)[0]
    want = ca.as_dict(ca.restated("csg", depth))
    with Uploaded(sb, parts) as up:
        h = up.parts(parts)
        got = ca.as_dict(sb.Scene.ClashParts(h, depth=depth)[0])
        assert got == want
        for a in range(3):
            for b in range(a + 1, 3):
                probes = sb.Scene.SampleParts([(h[a][0], h[a][1], cr.COMBINE_UNION), (h[b][0], h[b][1], cr.COMBINE_INTERSECT)], p)
                assert int((probes["value"] < 0).sum()) == got.get((a, b), 0), (a, b)


def test_the_sources_are_untouched_and_two_calls_give_the_same_bytes(sb):
    W, H, depth = 64, 48, 5
    parts = ca.parts("csg")
    cam = make_camera("default", W, H)
    up = Uploaded(sb, parts)
    before = {src: scene.Draw(cam, W, H) for src, scene in up.scenes.items()}
    first, _ = sb.Scene.ClashParts(up.parts(parts), depth=depth)
    second, _ = sb.Scene.ClashParts(up.parts(parts), depth=depth)
    for src, scene in up.scenes.items():
        assert_frames_identical(scene.Draw(cam, W, H), before[src], f"{src} after the calls")
    up.__exit__()
    # the sources are freed: the answers stand alone
    assert same_bytes(first, second) and same_bytes(first, ca.restated("csg", depth))
    with Uploaded(sb, parts) as again:
        assert same_bytes(sb.Scene.ClashParts(again.parts(parts), depth=depth)[0], first)


def test_a_list_of_65_is_refused_and_names_the_limit(sb):
    parts = ca.parts(ca.REFUSED)
    with Uploaded(sb, parts) as up:
        with pytest.raises(sb.SdfHipError) as e:
            sb.Scene.ClashParts(up.parts(parts), depth=3)
        assert e.value.code == sb._lib.ERR_ARG and "1..64" in str(e.value) and "SDFHIP_CLASH_MAX_INSTANCES" in str(e.value)
        got, _ = sb.Scene.ClashParts(up.parts(parts)[:64], depth=3)            # the first 64 are taken
        assert same_bytes(got, clr.clash(cr.as_instances(cc.with_trees(parts[:64])), 3))


def test_an_allocation_that_fails_is_nomem_and_a_plain_call_follows():
    # in a fresh process of its own, so that neither the variable nor a failed call can reach the tests beside this one: every
    # allocation the call reaches fails once through the library's own host-side allocation hook (nothing on the device is
    # provoked), each is SDFHIP_ERR_NOMEM, and afterwards a plain call gives the restatement's bytes (tests/clash_fault_child.py)
    child = os.path.join(REPO, "tests", "clash_fault_child.py")
    out = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    report = json.loads(out.stdout.strip().splitlines()[-1])
    assert report["failed"] == 3, report              # the instance table, the pair table, the counters
    assert report["codes_ok"] and report["outputs_untouched"] and report["source_frame_unchanged"], report
    assert report["plain_call_is_the_restatement"] and report["product_reads_no_variable"], report


def test_the_cpp_mirror_gives_the_same_bytes(tmp_path):
    # Program::ClashParts (include/sdfbox.hpp) on "lens": the restatement's bytes (tests/cpp_clash.cpp)
    import shutil
    from conftest import GOLDEN
    depth = 5
    exe, libdir = str(tmp_path / "cpp_clash"), os.path.join(REPO, "sdfbox_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "cpp_clash.cpp"),
                           "-o", exe, "-L", libdir, "-lsdfhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    shutil.copy(os.path.join(GOLDEN, "sphere_d4.asdf"), tmp_path / "sphere.asdf")
    out = subprocess.run([exe, str(tmp_path / "sphere.asdf"), str(depth), str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr)
    assert same_bytes(np.fromfile(tmp_path / "out.clash", dtype=clr.CLASH), ca.restated("lens", depth))

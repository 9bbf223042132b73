"""The penetration depth on the GPU (sdfhip_instances_penetration), both flavours of the library: the cases of tests/clash_cases.py
give the CPU restatement's records (tests/penetration_restatement.py, brute force) byte for byte -- floats included -- with the exact
skip on and off: two sources of different sizes, a box that leaves the unit cube, 64 parts in a chain (ties decided by the lowest
index) and 64 times one part (the fold's worst contention), every cursor form, a lattice of less than, exactly and more than one
4 x 4 x 4 block, one part, no overlap at all; the stats count what they say; every capacity; two calls give the same bytes; the
sources are untouched and may be freed; an allocation that fails is SDFHIP_ERR_NOMEM; the C++ mirror gives the same bytes."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import clash_cases as ca
import penetration_cases as pc
import penetration_restatement as pr
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


def check_stats(st, depth, K, skip, searches):
    points = 8 ** depth
    assert st.points == points and st.blocks == 8 ** max(depth - 2, 0) and st.blocks_looked <= st.blocks, (depth, K, skip)
    if skip:
        assert st.lookups <= points * K
    else:
        assert st.lookups == points * K and st.blocks_looked == st.blocks
    assert st.searches == searches
    if searches:
        assert st.visited >= searches                # every search loads the root at least
    else:
        # nothing was marked, emitted, searched, folded or recorded
        assert st.visited == 0 and not any(st.pass_ms[1:])


def check_case(sb, parts, depth, box, want, searches):
    origin, side = box
    with Uploaded(sb, parts) as up:
        for skip in (True, False):
            got, st = sb.Scene.PenetrationParts(up.parts(parts), depth=depth, origin=origin, side=side, skip=skip)
            assert same_bytes(got, want), (depth, skip, got, want)
            check_stats(st, depth, len(parts), skip, searches)
            # lookups, blocks_looked: as the clash check counts them on the same lattice
            _, cst = sb.Scene.ClashParts(up.parts(parts), depth=depth, origin=origin, side=side, skip=skip)
            assert (st.lookups, st.blocks_looked) == (cst.lookups, cst.blocks_looked)


@pytest.mark.parametrize("name, depth", pc.RUNS)
def test_every_case_is_the_restatements(sb, name, depth):
    want, counts = pc.restated(name, depth)
    assert len(want) == len(ca.restated(name, depth))
    check_case(sb, pc.parts(name), depth, pc.UNIT, want, counts["searches"])


def test_the_cases_are_what_they_are_for():
    # chain64: in most pairs more than one shared point attains the maximum -- the lowest-index rule decides; same64: every contained
    # point is in all 64 parts; lens: 60 and 504 shared points; csg: two distinct sources; eight: no overlap
    inst = pc.instances("chain64")
    import clash_restatement as clr
    p = clr.lattice(5)[0]
    inside = clr.contains(inst, p)
    tied = 0
    rec = pc.restated("chain64", 5)[0]
    assert len(rec) == 480
    for r in rec[::16]:
        both = np.nonzero(inside[r["a"]] & inside[r["b"]])[0]
        m = np.fmin(pr.searched(inst[r["a"]], p[both])[0], pr.searched(inst[r["b"]], p[both])[0])
        tied += int((m == m.max()).sum() > 1)
        assert both[np.nonzero(m == m.max())[0][0]] == r["witness"]
    assert tied >= 10, tied
    same, counts = pc.restated("same64", 3)
    assert len(same) == 2016 and counts["searches"] == 512 and len(set(same["witness"].tolist())) == 1 and len(set(same["depth"].tolist())) == 1
    assert [int(r["points"][0]) for r in (pc.restated("lens", 5)[0], pc.restated("lens", 6)[0])] == [60, 504]
    assert len({src for src, _, _ in pc.parts("csg")}) == 2 and len(pc.restated("csg", 5)[0]) == 3
    assert pc.restated("eight", 5)[1]["searches"] == 0 and pc.restated("one", 3)[1]["searches"] == 0


def test_a_box_that_leaves_the_unit_cube(sb):
    # inverse-mapped points outside a source's cube are searched like any other
    want, counts = pc.restated("csg", pc.OFF_CUBE_DEPTH, pc.OFF_CUBE)
    assert len(want) >= 1
    check_case(sb, pc.parts("csg"), pc.OFF_CUBE_DEPTH, pc.OFF_CUBE, want, counts["searches"])


@pytest.mark.parametrize("depth", [0, 1, 2, 3])
def test_less_than_one_block_exactly_one_and_eight(sb, depth):
    # the source's own sphere three times over.  depth 0: one lane, inside all three; depth 1: eight lanes and no pair; depth 2:
    # exactly one block; depth 3: eight blocks in two workgroups
    want, counts = pc.restated("own3", depth)
    assert len(want) == (0 if depth == 1 else 3) and counts["searches"] == {0: 3, 1: 0, 2: 24, 3: 168}[depth]
    check_case(sb, pc.parts("own3"), depth, pc.UNIT, want, counts["searches"])


def test_capacity_zero_one_and_exact(sb):
    L = sb._lib
    parts, depth = pc.parts("csg"), 5
    want = pc.restated("csg", depth)[0]
    assert len(want) == 3
    with Uploaded(sb, parts) as up:
        _, arr = sb.Scene._instances("test", up.parts(parts))
        opt = sb.PenetrationOptions(depth=depth)
        n = ctypes.c_uint32(77)
        assert L.lib.sdfhip_instances_penetration(arr, 3, ctypes.byref(opt), None, 0, ctypes.byref(n), None) == L.OK and n.value == 3
        for capacity in (1, 3, 5):
            out = np.frombuffer(bytes([0xEE]) * (5 * 64), dtype=pr.PENETRATION).copy()
            n = ctypes.c_uint32(77)
            assert L.lib.sdfhip_instances_penetration(arr, 3, ctypes.byref(opt), out.ctypes.data, capacity, ctypes.byref(n), None) == L.OK
            k = min(capacity, 3)
            assert n.value == 3 and same_bytes(out[:k], want[:k]) and (out[k:].view(np.uint8) == 0xEE).all(), capacity
        # one instance: a success with no pair; NULL options are the defaults (depth 6 on the unit cube, the skip on)
        n = ctypes.c_uint32(77)
        assert L.lib.sdfhip_instances_penetration(arr, 1, None, None, 0, ctypes.byref(n), None) == L.OK and n.value == 0
        st, dst = sb.PenetrationStats(), sb.PenetrationStats()
        out = np.zeros(3, pr.PENETRATION)
        assert L.lib.sdfhip_instances_penetration(arr, 3, None, out.ctypes.data, 3, ctypes.byref(n), ctypes.byref(st)) == L.OK
        assert n.value == len(ca.restated("csg", 6)) and st.points == 8 ** 6
        defaults, explicit = sb.PenetrationOptions(), np.zeros(3, pr.PENETRATION)
        assert L.lib.sdfhip_instances_penetration(arr, 3, ctypes.byref(defaults), explicit.ctypes.data, 3, ctypes.byref(n), ctypes.byref(dst)) == L.OK
        assert same_bytes(out, explicit) and (st.searches, st.visited, st.lookups) == (dst.searches, dst.visited, dst.lookups)
        assert np.array_equal(out["points"][:n.value], ca.restated("csg", 6)["points"])


def test_the_sources_are_untouched_and_two_calls_give_the_same_bytes(sb):
    W, H, depth = 64, 48, 5
    parts = pc.parts("csg")
    cam = make_camera("default", W, H)
    up = Uploaded(sb, parts)
    before = {src: scene.Draw(cam, W, H) for src, scene in up.scenes.items()}
    first, st1 = sb.Scene.PenetrationParts(up.parts(parts), depth=depth)
    second, st2 = sb.Scene.PenetrationParts(up.parts(parts), depth=depth)
    for src, scene in up.scenes.items():
        assert_frames_identical(scene.Draw(cam, W, H), before[src], f"{src} after the calls")
    up.__exit__()
    # the sources are freed: the answers stand alone
    assert same_bytes(first, second) and same_bytes(first, pc.restated("csg", depth)[0])
    assert (st1.searches, st1.visited, st1.lookups, st1.blocks_looked) == (st2.searches, st2.visited, st2.lookups, st2.blocks_looked) and st1.visited > 0
    with Uploaded(sb, parts) as again:
        third, st3 = sb.Scene.PenetrationParts(again.parts(parts), depth=depth)
        assert same_bytes(third, first) and st3.visited == st1.visited


def test_a_list_of_65_is_refused_and_names_the_limit(sb):
    parts = ca.parts(ca.REFUSED)
    with Uploaded(sb, parts) as up:
        with pytest.raises(sb.SdfHipError) as e:
            sb.Scene.PenetrationParts(up.parts(parts), depth=3)
        assert e.value.code == sb._lib.ERR_ARG and "1..64" in str(e.value) and "SDFHIP_CLASH_MAX_INSTANCES" in str(e.value)


def test_a_source_without_a_mesh_is_refused_only_when_a_search_would_run_on_it(sb):
    # sphere_d4 with one parent link bent (test_gpu_compose.py's inconsistent source): the look-ups follow the child links and read
    # the same values, so the clash check takes it; sdfhip_scene_mesh refuses it, and so does this call -- but only for the lens,
    # where both balls are searched, not where the bent one overlaps nothing
    import compose_cases as cc
    import place_restatement as plr
    S0, V0 = cc.tree("sphere_d4")
    Sb = S0.copy()
    Sb[int(S0[0, 1]) + 3, 0] = int(S0[0, 1])
    lens = pc.parts("lens")
    with sb.Scene(sb.OctData(S0, V0)) as good, sb.Scene(sb.OctData(Sb, V0)) as bad:
        assert not bad.stack_kernel_ok
        both = [(good, lens[0][1]), (bad, lens[1][1])]
        assert same_bytes(sb.Scene.ClashParts(both, depth=5)[0], ca.restated("lens", 5))
        with pytest.raises(sb.SdfHipError) as e:
            sb.Scene.PenetrationParts(both, depth=5)
        assert e.value.code == sb._lib.ERR_BAD_TREE and "instances_penetration: instance 1" in str(e.value)
        # the bent ball 0.45 from the good one's centre (two radii are 0.3), and alone: no search, no refusal
        apart, st = sb.Scene.PenetrationParts([(good, lens[0][1]), (bad, (plr.IDENTITY, 0.5, (0.5, 0.25, 0.25)))], depth=5)
        assert len(apart) == 0 and st.searches == 0
        alone, st = sb.Scene.PenetrationParts([(bad, lens[1][1])], depth=5)
        assert len(alone) == 0 and st.searches == 0
        # ... and the good one twice is the lens again
        assert same_bytes(sb.Scene.PenetrationParts([(good, lens[0][1]), (good, lens[1][1])], depth=5)[0], pc.restated("lens", 5)[0])


def test_an_allocation_that_fails_is_nomem_and_a_plain_call_follows():
    # in a fresh process of its own, so that neither the variable nor a failed call can reach the tests beside this one: every
    # allocation the call reaches fails once through the library's own host-side allocation hook (nothing on the device is
    # provoked), each is SDFHIP_ERR_NOMEM, and afterwards a plain call gives the restatement's bytes (tests/penetration_fault_child.py)
    child = os.path.join(REPO, "tests", "penetration_fault_child.py")
    out = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    report = json.loads(out.stdout.strip().splitlines()[-1])
    assert report["failed"] == 6, report              # the instance table, the pair table, the counters; one bitmap, the items, the records
    assert report["codes_ok"] and report["outputs_untouched"] and report["source_frame_unchanged"], report
    assert report["plain_call_is_the_restatement"] and report["product_reads_no_variable"], report


def test_the_cpp_mirror_gives_the_same_bytes(tmp_path):
    # Program::PenetrationParts (include/sdfbox.hpp) on "lens": the restatement's bytes (tests/cpp_penetration.cpp)
    import shutil
    from conftest import GOLDEN
    depth = 5
    exe, libdir = str(tmp_path / "cpp_penetration"), os.path.join(REPO, "sdfbox_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "cpp_penetration.cpp"),
                           "-o", exe, "-L", libdir, "-lsdfhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    shutil.copy(os.path.join(GOLDEN, "sphere_d4.asdf"), tmp_path / "sphere.asdf")
    out = subprocess.run([exe, str(tmp_path / "sphere.asdf"), str(depth), str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr)
    assert same_bytes(np.fromfile(tmp_path / "out.penetration", dtype=pr.PENETRATION), pc.restated("lens", depth)[0])

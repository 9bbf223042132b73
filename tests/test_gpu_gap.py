"""The clearance on the GPU (sdfhip_instances_gap), both flavours of the library: the cases of tests/gap_cases.py give the CPU
restatement's records (tests/gap_restatement.py, brute force) byte for byte -- floats included -- at limit = +inf, at a limit between
two of row64's gaps and with no pruning; a second call gives the same bytes; the counters say what the header says of them; every
capacity; NULL options; one part; what is refused; a source without a mesh; an allocation that fails is SDFHIP_ERR_NOMEM; the C++
mirror gives the same bytes.  Sources are uploaded directly: no test goes through Scene.Place."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gap_cases as gc
import gap_restatement as gr
from conftest import REPO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["product", "lab"])
def sb(request):
    import sdfbox_amd
    if request.param == "product":
        return sdfbox_amd
    import sdfbox_amd.lab
    return sdfbox_amd.lab.load()


class Uploaded:
    """one handle per distinct source of a list of parts, closed at the end of the `with`"""

    def __init__(self, sb, parts):
        self.scenes = {}
        for src, _, _ in parts:
            if src not in self.scenes:
                self.scenes[src] = sb.Scene(sb.OctData(*gc.tree(src)))

    def parts(self, parts):
        return [(self.scenes[src], pl, op) for src, pl, op in parts]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for s in self.scenes.values():
            s.close()


def same_bytes(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", gc.NAMES)
def test_every_case_is_the_restatements(sb, name):
    want, counts = gc.restated(name)
    parts = gc.parts(name)
    K = len(parts)
    with Uploaded(sb, parts) as up:
        got, st = sb.Scene.GapParts(up.parts(parts))
        assert same_bytes(got, want), (name, got, want)
        again, st2 = sb.Scene.GapParts(up.parts(parts))
        assert same_bytes(again, want), name
        full, fst = sb.Scene.GapParts(up.parts(parts), prune=False)
        assert same_bytes(full, want), (name, full, want)
        # the counters: no pruning runs the closed count; pruning never runs more
        assert fst.searches == counts["searches"] and fst.visited >= fst.searches
        assert 0 < st.searches <= fst.searches and 0 < st2.searches <= fst.searches
        assert st.pairs == fst.pairs == K * (K - 1) // 2 and st.pairs_searched <= st.pairs and st.cells == fst.cells > 0
        # a limit at the largest gap keeps every record, one below the smallest gap none
        if name != "row64":
            top, low = want["gap"].max(), want["gap"].min()
            assert same_bytes(sb.Scene.GapParts(up.parts(parts), limit=float(top))[0], want)
            if low > 0:
                none, nst = sb.Scene.GapParts(up.parts(parts), limit=float(np.nextafter(low, np.float32(0))))
                assert len(none) == 0 and nst.searches <= fst.searches


def test_a_limit_between_two_gaps_and_the_broad_phase(sb):
    parts = gc.parts("row64")
    want = gc.restated("row64", gc.ROW64_LIMIT)[0]
    assert 0 < len(want) < 2016
    with Uploaded(sb, parts) as up:
        got, st = sb.Scene.GapParts(up.parts(parts), limit=gc.ROW64_LIMIT)
        assert same_bytes(got, want)
        assert st.pairs == 2016 and len(want) <= st.pairs_searched < st.pairs
        full, fst = sb.Scene.GapParts(up.parts(parts), limit=gc.ROW64_LIMIT, prune=False)
        assert same_bytes(full, want) and fst.pairs_searched == 2016 and fst.searches == gc.restated("row64")[1]["searches"]
        assert st.searches <= fst.searches
        # limit 0: only the pairs that touch
        zero = sb.Scene.GapParts(up.parts(parts), limit=0.0)[0]
        assert same_bytes(zero, gc.restated("row64", 0.0)[0])


def test_capacity_zero_one_and_exact_null_options_and_one_part(sb):
    L = sb._lib
    parts = gc.parts("generic") + [gc.parts("nested")[1]]
    want = gr.gap(gc.instances("generic") + [gc.instances("nested")[1]])
    assert len(want) == 3
    with Uploaded(sb, parts) as up:
        _, arr = sb.Scene._instances("test", up.parts(parts))
        opt = sb.GapOptions()
        n = ctypes.c_uint32(77)
        assert L.lib.sdfhip_instances_gap(arr, 4, ctypes.byref(opt), None, 0, ctypes.byref(n), None) == L.OK and n.value == 3
        for capacity in (1, 3, 5):
            out = np.frombuffer(bytes([0xEE]) * (5 * 64), dtype=gr.GAP).copy()
            n = ctypes.c_uint32(77)
            assert L.lib.sdfhip_instances_gap(arr, 4, ctypes.byref(opt), out.ctypes.data, capacity, ctypes.byref(n), None) == L.OK
            k = min(capacity, 3)
            assert n.value == 3 and same_bytes(out[:k], want[:k]) and (out[k:].view(np.uint8) == 0xEE).all(), capacity
        # NULL options are the defaults (limit +inf, pruning on)
        out = np.zeros(3, gr.GAP)
        st = sb.GapStats()
        assert L.lib.sdfhip_instances_gap(arr, 4, None, out.ctypes.data, 3, ctypes.byref(n), ctypes.byref(st)) == L.OK
        assert n.value == 3 and same_bytes(out, want) and st.pairs == 6 and st.pairs_searched == 3
        # one instance: a success with no pair, and nothing is searched
        n = ctypes.c_uint32(77)
        st = sb.GapStats()
        assert L.lib.sdfhip_instances_gap(arr, 1, None, None, 0, ctypes.byref(n), ctypes.byref(st)) == L.OK and n.value == 0
        assert (st.pairs, st.pairs_searched, st.cells, st.searches, st.visited) == (0, 0, 0, 0, 0)


def test_what_is_refused(sb):
    import compose_cases as cc
    parts = [("nine", pl, op) for _, pl, op in cc.case("many")[0]]
    assert len(parts) == 65
    with Uploaded(sb, parts) as up:
        with pytest.raises(sb.SdfHipError) as e:
            sb.Scene.GapParts(up.parts(parts))
        assert e.value.code == sb._lib.ERR_ARG and "1..64" in str(e.value) and "SDFHIP_CLASH_MAX_INSTANCES" in str(e.value)
        for bad in (float("nan"), -1.0):
            with pytest.raises(sb.SdfHipError) as e:
                sb.Scene.GapParts(up.parts(parts[:2]), limit=bad)
            assert e.value.code == sb._lib.ERR_ARG and "limit" in str(e.value)


def test_a_source_without_a_mesh_is_refused_only_when_a_search_would_run_on_it(sb):
    # sphere_d4 with one parent link bent (test_gpu_compose.py's inconsistent source): sdfhip_scene_mesh refuses it, and so does this
    # call, naming the instance, whatever the limit -- but not where it stands alone
    import place_restatement as plr
    S0, V0 = gc.tree("sphere_d4")
    Sb = S0.copy()
    Sb[int(S0[0, 1]) + 3, 0] = int(S0[0, 1])
    apart = gc.parts("apart")
    with sb.Scene(sb.OctData(S0, V0)) as good, sb.Scene(sb.OctData(Sb, V0)) as bad:
        assert not bad.stack_kernel_ok
        with pytest.raises(sb.SdfHipError) as e:
            sb.Scene.GapParts([(good, apart[0][1]), (bad, apart[1][1])])
        assert e.value.code == sb._lib.ERR_BAD_TREE and "instances_gap: instance 1" in str(e.value)
        # a source without a mesh has no box to trust: 0.7 between the centres and a limit of 0.01 still keep its pair, and the call
        # refuses it by name, where the same arrangement of the good source is dropped before any search
        far = (plr.IDENTITY, 0.5, (0.75, 0.25, 0.25))
        with pytest.raises(sb.SdfHipError) as e:
            sb.Scene.GapParts([(good, apart[0][1]), (bad, far)], limit=0.01)
        assert e.value.code == sb._lib.ERR_BAD_TREE and "instances_gap: instance 1" in str(e.value)
        none, st = sb.Scene.GapParts([(good, apart[0][1]), (good, far)], limit=0.01)
        assert len(none) == 0 and st.pairs_searched == 0 and st.searches == 0
        alone, st = sb.Scene.GapParts([(bad, apart[1][1])])
        assert len(alone) == 0 and st.searches == 0
        # ... and the good one twice is the case again
        assert same_bytes(sb.Scene.GapParts([(good, apart[0][1]), (good, apart[1][1])])[0], gc.restated("apart")[0])


def test_the_sources_may_be_freed_and_the_answers_stand_alone(sb):
    parts = gc.parts("generic")
    up = Uploaded(sb, parts)
    first, _ = sb.Scene.GapParts(up.parts(parts))
    up.__exit__()
    assert same_bytes(first, gc.restated("generic")[0])
    v = sb.gap_vector(first[0])
    assert abs(float(np.linalg.norm(v)) - float(first[0]["gap"])) < 1e-6
    with Uploaded(sb, parts) as again:
        assert same_bytes(sb.Scene.GapParts(again.parts(parts))[0], first)


def test_an_allocation_that_fails_is_nomem_and_a_plain_call_follows():
    # in a fresh process of its own, so that neither the variable nor a failed call can reach the tests beside this one: every
    # allocation the call reaches fails once through the library's own host-side allocation hook (nothing on the device is
    # provoked), each is SDFHIP_ERR_NOMEM, and afterwards a plain call gives the restatement's bytes (tests/gap_fault_child.py)
    child = os.path.join(REPO, "tests", "gap_fault_child.py")
    out = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    report = json.loads(out.stdout.strip().splitlines()[-1])
    # the instance table, the keys, the counters, the sources' heads; one source's counts, cells and bitmap; the ordered pairs, the
    # work table, the records
    assert report["failed"] == 10, report
    assert report["codes_ok"] and report["outputs_untouched"] and report["source_frame_unchanged"], report
    assert report["plain_call_is_the_restatement"] and report["product_reads_no_variable"], report


def test_the_cpp_mirror_gives_the_same_bytes(tmp_path):
    # Program::GapParts (include/sdfbox.hpp) on "apart": the restatement's bytes (tests/cpp_gap.cpp)
    import shutil
    from conftest import GOLDEN
    exe, libdir = str(tmp_path / "cpp_gap"), os.path.join(REPO, "sdfbox_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "cpp_gap.cpp"),
                           "-o", exe, "-L", libdir, "-lsdfhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    shutil.copy(os.path.join(GOLDEN, "sphere_d4.asdf"), tmp_path / "sphere.asdf")
    out = subprocess.run([exe, str(tmp_path / "sphere.asdf"), str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr)
    assert same_bytes(np.fromfile(tmp_path / "out.gap", dtype=gr.GAP), gc.restated("apart")[0])

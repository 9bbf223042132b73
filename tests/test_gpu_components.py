"""The components of a scene on the GPU (sdfhip_scene_components[_device]), both flavours of the library: every case of
tests/components_cases.py gives the CPU restatement's records AND labels (tests/components_restatement.py) byte for byte -- they are
integers throughout -- at the depths where the lattice is one lane, eight lanes, one 4 x 4 x 4 block and eight, on a box that
leaves the unit cube, at every capacity, with and without labels, into device memory with guard words; two calls give the same
bytes; the stats count what they say; the source is untouched and may be freed; an allocation that fails is SDFHIP_ERR_NOMEM; the
C++ mirror gives the same bytes.  Every tree is uploaded from arrays made on the CPU."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import components_cases as cs
import components_restatement as cpr
from conftest import REPO, assert_frames_identical, make_camera

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


def upload(sb, name):
    return sb.Scene(sb.OctData(*cs.tree(name)))


def check_stats(st, rec, depth):
    solid = rec["flags"] == cpr.SOLID
    assert (st.points, st.components, st.solids) == (8 ** depth, len(rec), int(solid.sum())), depth
    assert st.inside == int(rec["points"][solid].sum()) and st.kernel_ms > 0 and st.total_ms >= st.kernel_ms


@pytest.mark.parametrize("name, depth, box", cs.RUNS)
def test_every_case_is_the_restatements(sb, name, depth, box):
    # (sphere_d4 at depths 0, 1, 2 and 3: one lane, eight lanes, exactly one block, eight blocks in two workgroups; "eight" on the
    # box that leaves the unit cube; checker: a record table as long as the lattice; snake: one body through every tile)
    want, want_labels = cs.restated(name, depth, box)
    with upload(sb, name) as scene:
        got, st, labels = scene.Components(depth=depth, origin=box[0], side=box[1], labels=True)
        assert same_bytes(got, want), (name, depth, got[:4], want[:4])
        assert same_bytes(labels, want_labels), (name, depth, int((labels != want_labels).sum()))
        check_stats(st, want, depth)
        bare, st = scene.Components(depth=depth, origin=box[0], side=box[1])                 # labels=None gives the same records
        assert same_bytes(bare, want)
        check_stats(st, want, depth)


def test_capacity_zero_one_exact_and_larger(sb):
    L = sb._lib
    name, depth = "csg", 5
    want, want_labels = cs.restated(name, depth)
    total = len(want)
    assert total == 4
    with upload(sb, name) as scene:
        opt = sb.ComponentsOptions(depth=depth)
        n = ctypes.c_uint32(77)
        assert L.lib.sdfhip_scene_components(scene._h, ctypes.byref(opt), None, 0, ctypes.byref(n), None, None) == L.OK and n.value == total
        for capacity in (1, total, total + 2):
            out = np.frombuffer(bytes([0xEE]) * ((total + 2) * 64), dtype=cpr.COMPONENT).copy()
            labels = np.zeros(8 ** depth, np.uint32)
            n = ctypes.c_uint32(77)
            assert L.lib.sdfhip_scene_components(scene._h, ctypes.byref(opt), out.ctypes.data, capacity, ctypes.byref(n), labels.ctypes.data, None) == L.OK
            k = min(capacity, total)
            assert n.value == total and same_bytes(out[:k], want[:k]) and (out[k:].view(np.uint8) == 0xEE).all(), capacity
            assert labels.tobytes() == want_labels.tobytes()
        # NULL options are the defaults: depth 6 on the unit cube
        st = sb.ComponentsStats()
        assert L.lib.sdfhip_scene_components(scene._h, None, None, 0, ctypes.byref(n), None, ctypes.byref(st)) == L.OK
        assert st.points == 8 ** 6 and n.value == st.components >= 2


def test_the_device_form_writes_into_a_tensor_with_guard_words(sb):
    import torch
    name, depth = "hollow", 5
    want, want_labels = cs.restated(name, depth)
    guard, words = 0xA5A5A5A5 - (1 << 32), 8 ** depth
    with upload(sb, name) as scene:
        buf = torch.full((64 + words + 64,), guard, dtype=torch.int32, device=f"cuda:{scene.device}")
        torch.cuda.synchronize(scene.device)
        got, st = scene.ComponentsDevice(depth=depth, labels_ptr=buf.data_ptr() + 64 * 4)
        host = buf.cpu().numpy().view(np.uint32)
        assert same_bytes(got, want) and host[64:64 + words].tobytes() == want_labels.tobytes()
        assert (host[:64] == 0xA5A5A5A5).all() and (host[64 + words:] == 0xA5A5A5A5).all()
        check_stats(st, want, depth)
        none, _ = scene.ComponentsDevice(depth=depth)
        assert same_bytes(none, want)


def test_two_calls_give_the_same_bytes_and_the_source_is_untouched_and_may_be_freed(sb):
    W, H, depth = 64, 48, 6
    cam = make_camera("default", W, H)
    want, want_labels = cs.restated("snake", depth)
    scene = upload(sb, "snake")
    before = scene.Draw(cam, W, H)
    first, _, first_labels = scene.Components(depth=depth, labels=True)
    second, _, second_labels = scene.Components(depth=depth, labels=True)
    assert_frames_identical(scene.Draw(cam, W, H), before, "snake after the calls")
    scene.close()
    # the source is freed: the answers stand alone
    assert same_bytes(first, second) and same_bytes(first_labels, second_labels)
    assert same_bytes(first, want) and same_bytes(first_labels, want_labels)
    with upload(sb, "snake") as again:
        assert same_bytes(again.Components(depth=depth)[0], first)


def test_an_allocation_that_fails_is_nomem_and_a_plain_call_follows():
    # in a fresh process of its own, so that neither the variable nor a failed call can reach the tests beside this one: every
    # allocation the call reaches fails once through the library's own host-side allocation hook (nothing on the device is
    # provoked), each is SDFHIP_ERR_NOMEM, and afterwards a plain call gives the restatement's bytes (tests/components_fault_child.py)
    child = os.path.join(REPO, "tests", "components_fault_child.py")
    out = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    report = json.loads(out.stdout.strip().splitlines()[-1])
    assert report["failed"] == 7, report              # the parents, the sign words, the root bitmap, its two scans, the counters, the records
    assert report["codes_ok"] and report["outputs_untouched"] and report["source_frame_unchanged"], report
    assert report["plain_call_is_the_restatement"] and report["product_reads_no_variable"], report


def test_the_cpp_mirror_gives_the_same_bytes(tmp_path):
    # Program::Components (include/sdfbox.hpp) on the depth-4 sphere: the restatement's bytes (tests/cpp_components.cpp)
    import shutil
    from conftest import GOLDEN
    depth = 5
    exe, libdir = str(tmp_path / "cpp_components"), os.path.join(REPO, "sdfbox_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "cpp_components.cpp"),
                           "-o", exe, "-L", libdir, "-lsdfhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    shutil.copy(os.path.join(GOLDEN, "sphere_d4.asdf"), tmp_path / "sphere.asdf")
    out = subprocess.run([exe, str(tmp_path / "sphere.asdf"), str(depth), str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr)
    want, want_labels = cs.restated("sphere_d4", depth)
    assert same_bytes(np.fromfile(tmp_path / "out.components", dtype=cpr.COMPONENT), want)
    assert np.fromfile(tmp_path / "out.labels", dtype=np.uint32).tobytes() == want_labels.tobytes()

"""ASan + UBSan, then TSan, over the host half of the library (builders incl. the threaded
subtree build, .asdf I/O, validation, camera)."""
import os
import platform
import shutil
import subprocess

from conftest import REPO


def test_host_code_under_asan_ubsan(tmp_path):
    src = os.path.join(REPO, "sdfbox_amd", "csrc")
    exe = str(tmp_path / "host_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-I", os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "host_sanitize.cpp")] +
                          [os.path.join(src, f) for f in ("errors.cpp", "asdf_io.cpp", "camera.cpp", "scene_gen.cpp")] +
                          ["-o", exe, "-lpthread"])
    out = subprocess.run([exe, str(tmp_path / "x.asdf")], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "host sanitizer run ok" in out.stdout


def test_threaded_builder_under_tsan(tmp_path):
    src = os.path.join(REPO, "sdfbox_amd", "csrc")
    exe = str(tmp_path / "host_tsan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-ffp-contract=off",
                           "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "host_sanitize.cpp")] +
                          [os.path.join(src, f) for f in ("errors.cpp", "asdf_io.cpp", "camera.cpp", "scene_gen.cpp")] +
                          ["-o", exe, "-lpthread"])
    # gcc 11's TSan runtime expects the address layout of at most 28 bits of mmap randomisation; on a kernel that randomises
    # more (vm.mmap_rnd_bits above 28) it can stop before main with "unexpected memory mapping".  So the program runs with
    # address randomisation off for its own process (setarch -R), wherever the host lets a process ask for that.
    no_aslr = ["setarch", platform.machine(), "-R"]
    if not shutil.which("setarch") or subprocess.run(no_aslr + ["true"], capture_output=True).returncode != 0:
        no_aslr = []
    out = subprocess.run(no_aslr + [exe, str(tmp_path / "y.asdf")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ThreadSanitizer" not in out.stderr, out.stdout + out.stderr


def test_injected_failures_come_back_as_status_codes(tmp_path):
    """"never throw/abort across the boundary" (the reference does: SdfGen/pch.h:20-26, dllmain.cpp:112-115).  operator
    new fails at every allocation of sdfhip_octdata_validate, sdfhip_load_obj / _ply, sdfhip_generate (serial and threaded) and
    sdfhip_asdf_load in turn, and pthread_create refuses every thread: each call returns SDFHIP_ERR_NOMEM with a message (or
    succeeds where the library copes), never std::terminate (tests/host_fault_injection.cpp; UBSan on)."""
    src = os.path.join(REPO, "sdfbox_amd", "csrc")
    exe = str(tmp_path / "host_fault")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "host_fault_injection.cpp")] +
                          [os.path.join(src, f) for f in ("errors.cpp", "asdf_io.cpp", "camera.cpp", "scene_gen.cpp", "point_readers.cpp")] +
                          ["-o", exe, "-lpthread", "-ldl"])
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "fault injection run ok" in out.stdout
    for entry in ("sdfhip_octdata_validate", "sdfhip_load_obj", "sdfhip_load_ply", "sdfhip_generate (4 threads)", "sdfhip_generate (no threads)"):
        assert entry in out.stdout

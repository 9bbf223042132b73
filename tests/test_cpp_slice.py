"""Program::Slice of the C++ host mirror (include/sdfbox.hpp): compile tests/cpp_slice.cpp, slice the golden sphere with an oblique stack
and compare records and counts with the numpy restatement, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import slice_restatement as sr
from conftest import GOLDEN, REPO


def build(tmp_path):
    exe = str(tmp_path / "cpp_slice")
    libdir = os.path.join(REPO, "sdfbox_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp_slice.cpp"), "-o", exe, "-L", libdir, "-lsdfhip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def run(tmp_path):
    exe = build(tmp_path)
    return subprocess.run([exe, os.path.join(GOLDEN, "sphere_d4.asdf"), str(tmp_path / "s.raw"), str(tmp_path / "c.raw")],
                          capture_output=True, text=True, timeout=120)


def test_cpp_slice_compiles_and_fails_loudly_without_gpu(tmp_path):
    import torch
    out = run(tmp_path)
    if torch.cuda.is_available():
        assert out.returncode == 0, out.stderr
    else:
        assert out.returncode == 3 and "sdfhip:" in out.stderr


@pytest.mark.gpu
def test_cpp_slice_is_the_restatements(tmp_path, scenes):
    out = run(tmp_path)
    assert out.returncode == 0, (out.returncode, out.stderr)
    od = scenes["sphere_d4"]
    rec, counts, _ = sr.slice_scene(od.Structs, od.Values, (0.6, 0.0, 0.8), 0.3, 0.05, 12)
    assert out.stdout.strip() == f"segments {len(rec)}" and len(rec) > 500
    assert np.fromfile(tmp_path / "s.raw", dtype=sr.SEGMENT).tobytes() == rec.tobytes()          # node-major, as the C call returns them
    assert np.fromfile(tmp_path / "c.raw", dtype=np.uint32).tolist() == counts.tolist()

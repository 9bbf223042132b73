"""The components of a scene (sdfhip_scene_components) without a GPU: the numpy restatement (tests/components_restatement.py) held to
counts pinned from labellers written another way -- a breadth-first flood fill written here, and scipy.ndimage.label where it imports
-- and to its own invariants; the Python helpers, the records' layout and the options' defaults; what the library and the mirrors
refuse before any device call.  tests/test_gpu_components.py holds the GPU to the restatement, byte for byte."""
import collections
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import components_cases as cs
import components_restatement as cpr
from conftest import REPO

# (case, depth) -> (the solids' points, the voids' points), each in descending order; N x P = N components of P points each.  Counted
# with the existing restatements and a labeller that is not the restatement's, before the kernels were written
PINS = {
    ("sphere_d4", 2): ([8], [56]), ("sphere_d4", 3): ([56], [456]), ("sphere_d4", 5): ([3568], [29200]),
    ("torus_d6", 2): ([], [64]), ("torus_d6", 5): ([1320], [31448]),
    ("eight", 3): ([4] * 8, [480]), ("eight", 5): ([202] * 8, [31152]),
    ("csg", 5): ([794, 2, 2], [31970]),
    ("hollow", 3): ([48], [456, 8]), ("hollow", 5): ([3064], [29272, 432]),
    ("checker", 3): ([1] * 256, [1] * 256), ("checker", 5): ([64] * 256, [64] * 256),
    ("snake", 3): ([148], [364]), ("snake", 5): ([9472], [23296]), ("snake", 6): ([9472 * 8], [262144 - 9472 * 8]),
}
OFF_CUBE_PIN = ([612, 554, 549, 485], [30568])          # "eight" on clash_cases.OFF_CUBE at depth 5
ZOO_COUNTS = {"dfs_d6_a": (160, 1), "dfs_d6_b": (38, 2), "blocks_1025": (75, 1), "blocks_2049": (9, 14), "blocks_4097": (141, 1),
              "chain12": (14, 1), "leaf": (2, 1)}      # depth 5: (solids, voids)


def flood_fill(ins):
    """Every point's label by a breadth-first flood fill from each unlabelled point in index order: the first point of a component
    to be met is its lowest index"""
    n = ins.shape[0]
    flat = ins.reshape(-1)
    lab = np.full(n ** 3, -1, np.int64)
    steps = ((1, 0), (n, 1), (n * n, 2))
    for start in range(n ** 3):
        if lab[start] >= 0:
            continue
        lab[start] = start
        queue = collections.deque([start])
        while queue:
            i = queue.popleft()
            c = (i % n, i // n % n, i // (n * n))
            for step, axis in steps:
                for j, ok in ((i - step, c[axis] > 0), (i + step, c[axis] < n - 1)):
                    if ok and lab[j] < 0 and flat[j] == flat[i]:
                        lab[j] = start
                        queue.append(j)
    return lab.reshape(n, n, n)


@pytest.mark.parametrize("name, depth", sorted(PINS))
def test_the_counts_labellers_written_another_way_gave(name, depth):
    rec, _ = cs.restated(name, depth)
    assert cs.points_by_phase(rec) == PINS[(name, depth)]


def test_the_counts_on_a_box_that_leaves_the_unit_cube_and_on_the_zoo():
    rec, _ = cs.restated("eight", cs.OFF_CUBE_DEPTH, cs.OFF_CUBE)
    assert cs.points_by_phase(rec) == OFF_CUBE_PIN
    for name, (solids, voids) in ZOO_COUNTS.items():
        s, v = cs.points_by_phase(cs.restated(name, 5)[0])
        assert (len(s), len(v)) == (solids, voids), name


@pytest.mark.parametrize("name, depth, box", [r for r in cs.RUNS if r[1] <= 5])
def test_a_flood_fill_gives_the_restatements_labels(name, depth, box):
    ins = cpr.inside(cs.tree(name), depth, *box)
    _, lab = cs.restated(name, depth, box)
    assert (flood_fill(ins) == lab).all()


@pytest.mark.parametrize("name, depth, box", cs.RUNS)
def test_scipy_counts_the_same_components(name, depth, box):
    ndi = pytest.importorskip("scipy.ndimage")
    ins = cpr.inside(cs.tree(name), depth, *box)
    rec, lab = cs.restated(name, depth, box)
    for phase, flag in ((ins, cpr.SOLID), (~ins, 0)):
        theirs, count = ndi.label(phase)                        # (the default structure is the six face neighbours)
        mine = rec[rec["flags"] == flag]
        assert count == len(mine)
        if count:
            # the same partition: each of scipy's labels meets exactly one of the restatement's, and their sizes agree
            pairs = np.unique(np.stack([theirs[phase], lab[phase].astype(np.int64)], 1), axis=0)
            assert len(pairs) == count
            assert sorted(np.bincount(theirs[phase])[1:]) == sorted(int(p) for p in mine["points"])


@pytest.mark.parametrize("name, depth, box", cs.RUNS)
def test_the_invariants(name, depth, box):
    rec, lab = cs.restated(name, depth, box)
    ins = cpr.inside(cs.tree(name), depth, *box)
    n = 1 << depth
    assert lab.shape == (n, n, n) and lab.dtype == np.uint32 and rec.dtype == cpr.COMPONENT
    assert int(rec["points"].sum()) == 8 ** depth and (rec["points"] >= 1).all() and not rec["reserved"].any()
    flat = lab.reshape(-1)
    assert (flat[rec["label"]] == rec["label"]).all() and (np.diff(rec["label"].astype(np.int64)) > 0).all()
    assert (flat <= np.arange(8 ** depth)).all() and set(np.unique(flat)) == set(int(v) for v in rec["label"])
    assert int(rec["points"][rec["flags"] == cpr.SOLID].sum()) == int(ins.sum())
    assert set(np.unique(rec["flags"])) <= {0, cpr.SOLID}
    # a record is what its fields say, on its own points
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    for r in rec[:: max(1, len(rec) // 8)]:
        at = lab == r["label"]
        c = np.stack([x[at], y[at], z[at]], 1)
        assert int(r["points"]) == len(c) and (r["lo"] == c.min(0)).all() and (r["hi"] == c.max(0)).all() and (r["sum"] == c.sum(0)).all()
        assert (ins[at] == bool(r["flags"])).all()


def test_the_cases_are_what_they_are_for(sb):
    # hollow: the smaller void is a sealed cavity, the larger is the outside; checker at depth 3: a record per lattice point; snake:
    # one body of 148 of the depth-5 lattice's 4 x 4 x 4 blocks, which visits each of its 64 tiles of 8 x 8 x 8
    for depth in (3, 5):
        rec, _ = cs.restated("hollow", depth)
        voids = rec[rec["flags"] == 0]
        assert [sb.component_enclosed(r, depth) for r in voids[np.argsort(voids["points"])]] == [True, False]
        assert not sb.component_enclosed(rec[0], depth) and rec[0]["label"] == 0
    assert len(cs.restated("checker", 3)[0]) == 8 ** 3
    rec, lab = cs.restated("snake", 5)
    solid = rec[rec["flags"] == cpr.SOLID]
    assert len(solid) == 1 and (solid[0]["lo"] == 0).all() and (solid[0]["hi"][:2] == 31).all()
    body = (lab == solid[0]["label"]).reshape(4, 8, 4, 8, 4, 8)
    assert body.any(axis=(1, 3, 5)).all() and int(body.reshape(8, 4, 8, 4, 8, 4).all(axis=(1, 3, 5)).sum()) == 148


def test_the_python_helpers_read_a_record(sb):
    d, (origin, side) = cs.OFF_CUBE_DEPTH, cs.OFF_CUBE
    r = cs.restated("eight", d, cs.OFF_CUBE)[0][1]
    pitch = side * 2.0 ** -d
    assert sb.component_volume(r, d, side) == pytest.approx(int(r["points"]) * pitch ** 3, rel=1e-12)
    want = np.array(origin) + (r["sum"] / float(r["points"]) + 0.5) * pitch
    assert np.allclose(sb.component_centroid(r, d, origin, side), want, rtol=0, atol=1e-12)
    o, s = sb.component_box(r, d, origin, side)
    lo, hi = np.array(origin) + r["lo"] * pitch, np.array(origin) + (r["hi"] + 1.0) * pitch
    assert s == pytest.approx(float((hi - lo).max()), rel=1e-12)
    assert (np.array(o) <= lo + 1e-12).all() and (np.array(o) + s >= hi - 1e-12).all()
    assert np.allclose(np.array(o) + s / 2, (lo + hi) / 2, rtol=0, atol=1e-12)
    fake = np.zeros(1, cpr.COMPONENT)[0]
    for lo_, hi_, want in (((1, 1, 1), (6, 6, 6), True), ((0, 1, 1), (6, 6, 6), False), ((1, 1, 1), (6, 7, 6), False), ((1, 1, 1), (1, 1, 1), True)):
        fake["lo"], fake["hi"] = lo_, hi_
        assert sb.component_enclosed(fake, 3) is want


def test_the_records_are_the_headers(sb):
    text = open(os.path.join(REPO, "include", "sdfhip.h")).read()
    widths = {"float": 4, "uint32_t": 4, "uint64_t": 8}
    for c_name, cls, dtype, size in (("sdfhip_component", sb.Component, cpr.COMPONENT, 64), ("sdfhip_components_options", sb.ComponentsOptions, None, 28),
                                     ("sdfhip_components_stats", sb.ComponentsStats, None, 32)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (c_name, c_name), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        off = 0
        names = []
        for decl in body.split(";"):
            words = decl.split()
            if not words:
                continue
            for n in " ".join(words[1:]).split(","):
                m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", n)
                name, count = m.group(1), int(m.group(2) or 1)
                assert getattr(cls, name).offset == off, (c_name, name)
                if dtype is not None:
                    assert dtype.fields[name][1] == off and dtype.fields[name][0].base.itemsize == widths[words[0]], (c_name, name)
                names.append(name)
                off += widths[words[0]] * count
        assert off == size == ctypes.sizeof(cls) and names == [f[0] for f in cls._fields_], c_name
    assert np.dtype(sb.Component) == cpr.COMPONENT
    assert sb.COMPONENT_SOLID == int(re.search(r"SDFHIP_COMPONENT_SOLID\s*=\s*(\d+)", text).group(1)) == cpr.SOLID == 1
    assert sb.COMPONENTS_MAX_DEPTH == int(re.search(r"SDFHIP_COMPONENTS_MAX_DEPTH\s*=\s*(\d+)", text).group(1)) == cpr.MAX_DEPTH == 9
    for name in ("sdfhip_components_options_default", "sdfhip_scene_components", "sdfhip_scene_components_device"):
        assert name in sb._lib.EXPORTED_SYMBOLS and hasattr(sb._lib.lib, name)
    assert hasattr(sb.Scene, "Components") and hasattr(sb.Scene, "ComponentsDevice")
    # the defaults, from the library and from the Python class
    opt = sb.ComponentsOptions(flags=7, depth=1, origin=(1, 2, 3), side=9.0)
    sb._lib.lib.sdfhip_components_options_default(ctypes.byref(opt))
    for o in (opt, sb.ComponentsOptions()):
        assert (o.size, o.flags, o.depth, tuple(o.origin), o.side) == (28, 0, 6, (0.0, 0.0, 0.0), 1.0)
    sb._lib.lib.sdfhip_components_options_default(None)            # a null argument is a message, never a crash
    assert b"components_options_default" in sb._lib.lib.sdfhip_last_error()


@pytest.mark.parametrize("entry", ["sdfhip_scene_components", "sdfhip_scene_components_device"])
def test_the_library_refuses_what_needs_no_handle(sb, entry):
    L = sb._lib
    call = getattr(L.lib, entry)
    # (the handle is read last: the address of a zeroed block stands in for it where the refusal comes first)
    block = (ctypes.c_uint8 * 4096)()
    fake = ctypes.c_void_p(ctypes.addressof(block))
    out = np.zeros(4, np.dtype(sb.Component))
    labels = np.zeros(8, np.uint32)
    n = ctypes.c_uint32(77)

    def refused(word, scene=fake, opt=None, out_ptr=out.ctypes.data, capacity=4, n_components=n):
        rc = call(scene, ctypes.byref(opt) if opt is not None else None, out_ptr, capacity,
                  ctypes.byref(n_components) if n_components is not None else None, labels.ctypes.data, None)
        msg = L.lib.sdfhip_last_error()
        assert rc == L.ERR_ARG and word in msg and entry[len("sdfhip_"):].encode() + b":" in msg, (word, rc, msg)
        assert n.value == 77 and not out.view(np.uint8).any() and not labels.any()     # nothing was written

    refused(b"null scene", scene=None)
    refused(b"null scene", scene=None, opt=sb.ComponentsOptions(depth=9))
    refused(b"null n_components", n_components=None)
    refused(b"null out", out_ptr=None)
    refused(b"depth", opt=sb.ComponentsOptions(depth=10))
    refused(b"4 GB", opt=sb.ComponentsOptions(depth=10))               # the refusal says why the cap is 9, not the clash check's 10
    refused(b"flags", opt=sb.ComponentsOptions(flags=1))
    for bad in (float("nan"), float("inf")):
        refused(b"origin", opt=sb.ComponentsOptions(origin=(0.0, bad, 0.0)))
    for bad in (float("nan"), float("inf"), 0.0, -1.0):
        refused(b"side", opt=sb.ComponentsOptions(side=bad))
    refused(b"far corner", opt=sb.ComponentsOptions(origin=(3e38, 0.0, 0.0), side=3e38))
    small = sb.ComponentsOptions()
    small.size = 8
    refused(b"bytes", opt=small)

    class Newer(ctypes.Structure):
        _fields_ = sb.ComponentsOptions._fields_ + [("unknown", ctypes.c_int32)]
    newer = Newer()
    ctypes.memmove(ctypes.byref(newer), ctypes.byref(sb.ComponentsOptions()), 28)
    newer.size, newer.unknown = 32, 3
    as_options = ctypes.cast(ctypes.pointer(newer), ctypes.POINTER(sb.ComponentsOptions)).contents
    refused(b"", opt=as_options)                                       # an unknown field that is set
    newer.unknown = -1
    refused(b"null scene", scene=None, opt=as_options)                 # ... and one that says "default": the call goes on to the handle


def test_the_python_layer_refuses_what_needs_no_handle(sb):
    class Unloaded(sb.Scene):
        def __init__(self):
            self._h = None
    for kw in ({}, {"depth": 10}, {"labels": True}, {"side": 0.0}):
        with pytest.raises(sb.SdfHipError) as e:
            Unloaded().Components(**kw)
        assert e.value.code == sb._lib.ERR_ARG
    with pytest.raises(sb.SdfHipError) as e:
        Unloaded().ComponentsDevice(depth=3, labels_ptr=None)
    assert e.value.code == sb._lib.ERR_ARG


def test_the_cpp_mirror_checks_its_arguments_and_fails_loudly_without_a_gpu(tmp_path):
    # Program::Components (include/sdfbox.hpp) through tests/cpp_components.cpp: what it refuses needs no GPU; with one the bytes are
    # tests/test_gpu_components.py's
    import shutil
    import torch
    from conftest import GOLDEN
    exe, libdir = str(tmp_path / "cpp_components"), os.path.join(REPO, "sdfbox_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "cpp_components.cpp"),
                           "-o", exe, "-L", libdir, "-lsdfhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    shutil.copy(os.path.join(GOLDEN, "sphere_d4.asdf"), tmp_path / "sphere.asdf")
    out = subprocess.run([exe, str(tmp_path / "sphere.asdf"), "5", str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert "argument checks ok" in out.stderr, (out.returncode, out.stderr)
    if torch.cuda.is_available():
        assert out.returncode == 0, out.stderr
    else:
        assert out.returncode == 3 and "sdfhip:" in out.stderr, (out.returncode, out.stderr)

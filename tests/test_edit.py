"""Space carving (sdfhip_scene_edit) without a GPU: the CPU restatement's trees (tests/edit_restatement.py) are consistent, in the
pinned node order and carve or add the right solid; the entry point refuses what it must refuse before it touches a device; the
Python mirror's constants are the header's.  tests/test_gpu_edit.py holds the GPU to the restatement byte for byte."""
import ctypes
import os
import re

import numpy as np
import pytest

import edit_restatement as er
from conftest import REPO

SPHERE = (0.5, 0.5, 0.5, 0.3)                  # sphere_d4's shape
TORUS = (0.5, 0.5, 0.5, 0.25, 0.09)            # torus_d6's shape (axis y)

BRUSHES = [
    ("carve", er.EDIT_CARVE, er.BRUSH_SPHERE, (0.5, 0.5, 0.8, 0.12)),
    ("add", er.EDIT_ADD, er.BRUSH_SPHERE, (0.62, 0.55, 0.5, 0.15)),
    ("carve_box", er.EDIT_CARVE, er.BRUSH_BOX, (0.3, 0.5, 0.5, 0.1, 0.07, 0.2)),
    ("add_box", er.EDIT_ADD, er.BRUSH_BOX, (0.5, 0.78, 0.45, 0.2, 0.05, 0.08)),
]


def node_depths(structs):
    depth = np.full(len(structs), -1, dtype=np.int64)
    level, d = np.zeros(1, dtype=np.int64), 0
    while len(level):
        depth[level] = d
        kids = structs[level, 1]
        kids = kids[kids >= 0].astype(np.int64)
        level = (kids[:, None] + np.arange(8)).reshape(-1)
        d += 1
    return depth


def assert_edit_order(before, after):
    """original nodes keep their indices (and structure, bar split leaves); new blocks of 8 follow them, ordered by (depth of the
    block, index of its parent), each parent's children field pointing at its block"""
    n0 = len(before)
    assert (len(after) - n0) % 8 == 0
    assert (after[:n0, 0] == before[:n0, 0]).all()
    changed = np.nonzero(after[:n0, 1] != before[:n0, 1])[0]
    assert (before[changed, 1] == -1).all() and (after[changed, 1] >= n0).all()
    if len(after) == n0:
        return
    starts = np.arange(n0, len(after), 8)
    parents = after[starts, 0].astype(np.int64)
    assert (after[n0:, 0].reshape(-1, 8) == parents[:, None]).all()
    assert (after[parents, 1] == starts).all()
    depth = node_depths(after)
    key = depth[starts] * (1 << 32) + parents
    assert (np.diff(key) > 0).all(), "new blocks out of (depth, parent index) order"


def analytic(shape, p):
    x, y, z = p[:, 0] - 0.5, p[:, 1] - 0.5, p[:, 2] - 0.5
    if shape == "sphere":
        return np.sqrt(x * x + y * y + z * z) - SPHERE[3]
    q = np.sqrt(x * x + z * z) - TORUS[3]
    return np.sqrt(q * q + y * y) - TORUS[4]


def brush_exact(brush, params, p):
    return er.brush_distance(brush, params, p[:, 0].astype(np.float32), p[:, 1].astype(np.float32),
                             p[:, 2].astype(np.float32)).astype(np.float64)


@pytest.fixture(scope="module")
def shapes(sb):
    return {"sphere": sb.sphere_d4(), "torus": sb.torus_d6()}


def test_a_far_brush_changes_nothing(shapes):
    for od in shapes.values():
        for op in (er.EDIT_CARVE, er.EDIT_ADD):
            for brush, params in ((er.BRUSH_SPHERE, (3.0, 0.5, 0.5, 0.5)), (er.BRUSH_BOX, (0.5, -2.0, 0.5, 0.3, 0.5, 0.2))):
                for md in (-1, 7):
                    S, V = er.edit(od.Structs, od.Values, [(op, brush, params)], md)
                    assert np.array_equal(S, od.Structs) and np.array_equal(V, od.Values)


@pytest.mark.parametrize("name", [b[0] for b in BRUSHES])
def test_restated_trees_are_consistent_and_in_order(sb, shapes, name):
    _, op, brush, params = next(b for b in BRUSHES if b[0] == name)
    for od in shapes.values():
        d0 = er.tree_depth(od.Structs)
        for md in (-1, d0 + 1, d0 + 2, 2):
            S, V = er.edit(od.Structs, od.Values, [(op, brush, params)], md)
            depth, consistent = sb.OctData(S, V).validate()
            assert consistent and depth == max(d0, depth) and depth <= max(d0, md)
            assert_edit_order(od.Structs, S)
            if md > d0:
                assert len(S) > len(od.Structs), "a brush through the surface refines past the input's depth"


def test_an_edit_list_is_chained_edits(shapes):
    od = shapes["torus"]
    edits = [(op, brush, params) for _, op, brush, params in BRUSHES[:3]]
    S, V = er.edit(od.Structs, od.Values, edits, 7)
    S1, V1 = od.Structs, od.Values
    for e in edits:
        S1, V1 = er.edit(S1, V1, [e], 7)
    assert np.array_equal(S, S1) and np.array_equal(V, V1)


@pytest.mark.parametrize("shape", ["sphere", "torus"])
def test_the_edited_field_has_the_sign_of_the_csg(oracle_mod, shapes, shape):
    od = shapes[shape]
    rng = np.random.default_rng(7)
    d0 = er.tree_depth(od.Structs)
    for _, op, brush, params in BRUSHES:
        S, V = er.edit(od.Structs, od.Values, [(op, brush, params)], d0 + 2)
        pts = rng.uniform(0.02, 0.98, size=(1500, 3))
        d = analytic(shape, pts)
        s = brush_exact(brush, params, pts)
        want = np.maximum(d, -s) if op == er.EDIT_CARVE else np.minimum(d, s)
        checked = 0
        for p, dd, ss, w in zip(pts, d, s, want):
            got, _, scale = oracle_mod.distance_at(S, V, *p)
            if abs(dd) < 2 * scale or abs(ss) < 2 * scale:
                continue
            checked += 1
            assert np.sign(got) == np.sign(w), (shape, op, brush, p.tolist(), got, w, scale)
        assert checked > 300


def test_edit_refuses_a_null_scene_without_a_gpu(sb):
    out = ctypes.c_void_p()
    e = sb.Edit(sb.EDIT_CARVE, sb.BRUSH_SPHERE, (0.5, 0.5, 0.5, 0.1))
    assert sb._lib.lib.sdfhip_scene_edit(None, ctypes.byref(e), 1, -1, ctypes.byref(out), None, None) == sb._lib.ERR_ARG
    assert b"null" in sb._lib.lib.sdfhip_last_error()
    assert out.value is None


def test_edit_constants_and_structs_match_the_header(sb):
    text = open(os.path.join(REPO, "include", "sdfhip.h")).read()
    enums = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bSDFHIP_((?:EDIT|BRUSH)_[A-Z]+)\s*=\s*(\d+)", text)}
    assert enums == {"EDIT_CARVE": 0, "EDIT_ADD": 1, "BRUSH_SPHERE": 0, "BRUSH_BOX": 1}
    for name, value in enums.items():
        assert getattr(sb, name) == value == getattr(er, name)
    assert ctypes.sizeof(sb.Edit) == 32 and sb.Edit.params.offset == 8
    assert ctypes.sizeof(sb.EditStats) == 36 and sb.EditStats.edit_ms.offset == 24
    assert "sdfhip_scene_edit" in sb._lib.EXPORTED_SYMBOLS

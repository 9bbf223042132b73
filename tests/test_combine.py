"""Combination (sdfhip_scene_combine) without a GPU: the CPU restatement (tests/combine_restatement.py) is held to the rule's
identities, its symmetry, node counts from an independent prototype of the rule and the sign of the analytic CSG; the entry point
refuses what it must refuse before it touches a device; the Python mirror's constants and records are the header's.
tests/test_gpu_combine.py holds the GPU to the restatement byte for byte."""
import ctypes
import os
import re

import numpy as np
import pytest

import combine_restatement as cr
import edit_restatement as er
import prune_restatement as pr
from conftest import REPO

SPHERE = (0.5, 0.5, 0.5, 0.3)                  # sphere_d4's shape
TORUS = (0.5, 0.5, 0.5, 0.25, 0.09)            # torus_d6's shape (axis y)
OFF = (0.66, 0.5, 0.42, 0.17)                  # the off-centre sphere, depth 7
PAIRS = {("torus", "off"): 93273, ("sphere", "torus"): 39497, ("off", "sphere"): 67529}     # nodes, no cut, every op
OP_NAMES = {cr.COMBINE_UNION: "union", cr.COMBINE_INTERSECT: "intersect", cr.COMBINE_SUBTRACT: "subtract"}


@pytest.fixture(scope="module")
def trees(sb):
    arrays = lambda od: (od.Structs, od.Values)
    leaf = np.array([[-1, -1]], dtype=np.int32)
    out = {"sphere": arrays(sb.sphere_d4()), "torus": arrays(sb.torus_d6()),
           "off": arrays(sb.OctData.Generate(sb._lib.SHAPE_SPHERE, list(OFF), 7)),
           "empty": (leaf, np.full((1, 8), 255, dtype=np.uint8)), "full": (leaf.copy(), np.zeros((1, 8), dtype=np.uint8))}
    for S, V in out.values():
        S.setflags(write=False); V.setflags(write=False)
    return out


_combined = {}


def combined(trees, a, b, op, max_depth=-1):
    key = (a, b, op, max_depth)
    if key not in _combined:
        _combined[key] = cr.combine(trees[a], trees[b], op, max_depth)
    return _combined[key]


def same(x, y):
    return np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


def rows(V):
    return np.sort(np.ascontiguousarray(V).view(np.uint64).reshape(-1))


def assert_breadth_first(sb, S, V):
    """sdfhip_octdata_validate accepts the tree; node 0 is the root; the blocks of eight follow one another in ascending index of
    their parents (which is breadth first), child i at block + i, every child's parent pointing back"""
    n = len(S)
    assert S.dtype == np.int32 and V.dtype == np.uint8 and V.shape == (n, 8) and (n - 1) % 8 == 0
    depth, consistent = sb.OctData(S, V).validate()
    assert consistent and depth == er.tree_depth(S)
    assert S[0, 0] == -1
    inner = np.nonzero(S[:, 1] >= 0)[0]
    assert (S[inner, 1] == 1 + 8 * np.arange(len(inner))).all(), "the blocks are not in the order of their parents"
    assert (S[1:, 0].reshape(-1, 8) == inner[:, None]).all(), "a child's parent does not point back"
    return depth


def analytic(name, p):
    if name == "torus":
        x, y, z = p[:, 0] - TORUS[0], p[:, 1] - TORUS[1], p[:, 2] - TORUS[2]
        q = np.sqrt(x * x + z * z) - TORUS[3]
        return np.sqrt(q * q + y * y) - TORUS[4]
    c = SPHERE if name == "sphere" else OFF
    return np.sqrt(((p - np.array(c[:3])) ** 2).sum(1)) - c[3]


@pytest.mark.parametrize("name", ["sphere", "torus", "off", "empty", "full"])
def test_identities(sb, trees, name):
    X = trees[name]
    forms = {"union(X, empty)": combined(trees, name, "empty", cr.COMBINE_UNION), "union(empty, X)": combined(trees, "empty", name, cr.COMBINE_UNION),
             "intersect(X, full)": combined(trees, name, "full", cr.COMBINE_INTERSECT),
             "subtract(X, empty)": combined(trees, name, "empty", cr.COMBINE_SUBTRACT), "union(X, X)": combined(trees, name, name, cr.COMBINE_UNION)}
    first = forms["union(X, empty)"]
    for what, got in forms.items():
        assert same(got, first), what
    assert len(first[0]) == len(X[0]) and np.array_equal(rows(first[1]), rows(X[1])), "X re-ordered breadth first"
    assert assert_breadth_first(sb, *first) == er.tree_depth(X[0])
    if name in ("sphere", "torus", "off"):            # the analytic builder's order is depth first: the re-ordering is one
        assert not np.array_equal(first[0], X[0])
    again = cr.combine(first, trees["empty"], cr.COMBINE_UNION)
    assert same(again, first), "a breadth-first tree is its own re-ordering"


@pytest.mark.parametrize("pair", list(PAIRS), ids="-".join)
def test_union_and_intersection_are_symmetric(trees, pair):
    a, b = pair
    for op in (cr.COMBINE_UNION, cr.COMBINE_INTERSECT):
        assert same(combined(trees, a, b, op), combined(trees, b, a, op)), OP_NAMES[op]
    assert not same(combined(trees, a, b, cr.COMBINE_SUBTRACT), combined(trees, b, a, cr.COMBINE_SUBTRACT))


@pytest.mark.parametrize("pair", list(PAIRS), ids="-".join)
def test_results_are_valid_and_have_the_prototypes_node_counts(sb, trees, pair):
    a, b = pair
    nA, nB = len(trees[a][0]), len(trees[b][0])
    for op in cr.OPS:
        S, V, counts = cr.combine(trees[a], trees[b], op, want_counts=True)
        assert same((S, V), combined(trees, a, b, op))
        assert len(S) == PAIRS[pair] <= nA + nB - 1, OP_NAMES[op]
        assert assert_breadth_first(sb, S, V) == counts["depth_out"] == max(er.tree_depth(trees[a][0]), er.tree_depth(trees[b][0]))
        # a cell is a node of the result iff it is one of A or of B: |A| + |B| - |both|
        assert counts["nodes_shared"] == nA + nB - len(S)


def test_the_depth_cut(sb, trees):
    for op in cr.OPS:
        S, V = combined(trees, "sphere", "torus", op, 0)
        assert len(S) == 1 and tuple(S[0]) == (-1, -1)
        assert np.array_equal(V, combined(trees, "sphere", "torus", op)[1][:1])
        whole = combined(trees, "sphere", "torus", op)
        assert er.tree_depth(trees["sphere"][0]) == 4 and er.tree_depth(trees["torus"][0]) == 6
        S, V = combined(trees, "sphere", "torus", op, 5)          # between the two depths
        assert assert_breadth_first(sb, S, V) == 5
        per_level = [len(level) for level in pr.levels(whole[0])]
        n = sum(per_level[:6])
        # breadth first: the cut tree is the uncut one's first levels, the deepest of them made leaves
        assert len(S) == n < len(whole[0])
        assert np.array_equal(V, whole[1][:n]) and np.array_equal(S[:, 0], whole[0][:n, 0])
        last = n - per_level[5]
        assert np.array_equal(S[:last, 1], whole[0][:last, 1]) and (S[last:, 1] == -1).all()
        assert same(combined(trees, "sphere", "torus", op, 6), whole) and same(combined(trees, "sphere", "torus", op, 12), whole)


@pytest.mark.parametrize("op", cr.OPS, ids=OP_NAMES.get)
@pytest.mark.parametrize("pair", list(PAIRS), ids="-".join)
def test_the_combined_field_has_the_sign_of_the_csg(oracle_mod, trees, pair, op):
    a, b = pair
    S, V = combined(trees, a, b, op)
    rng = np.random.default_rng(11)
    pts = rng.uniform(0.02, 0.98, size=(1500, 3))
    dA, dB = analytic(a, pts), analytic(b, pts)
    want = {cr.COMBINE_UNION: np.minimum(dA, dB), cr.COMBINE_INTERSECT: np.maximum(dA, dB), cr.COMBINE_SUBTRACT: np.maximum(dA, -dB)}[op]
    checked = 0
    for p, da, db, w in zip(pts, dA, dB, want):
        got, _, scale = oracle_mod.distance_at(S, V, *p)
        if abs(da) < 2 * scale or abs(db) < 2 * scale:
            continue
        checked += 1
        assert np.sign(got) == np.sign(w), (pair, OP_NAMES[op], p.tolist(), got, w, scale)
    assert checked >= 600, checked


def test_a_prune_at_tolerance_0_removes_what_the_loser_left(sb, trees):
    for pair in PAIRS:
        union = combined(trees, *pair, cr.COMBINE_UNION)
        S, V = pr.prune(*union, 0)
        assert len(S) < len(union[0]), pair
        assert sb.OctData(S, V).validate()[1]
    # the whole of the empty tree's side of union(X, X-with-an-empty-operand) is X: nothing to remove beyond what X's own prune removes
    X = trees["torus"]
    assert len(pr.prune(*combined(trees, "torus", "empty", cr.COMBINE_UNION), 0)[0]) == len(pr.prune(*X, 0)[0])


def test_negation_flips_the_sign_at_the_surface():
    b = np.arange(256, dtype=np.uint8)
    for d in (0, 3, 12):
        S = np.float32(2.0 ** -d)
        neg = cr.negate(b, S)
        assert neg[63] == 64 and neg[64] == 63
        assert ((b <= 63) == (neg >= 64)).all(), "a byte inside becomes one outside, and the reverse"
        assert (np.diff(neg.astype(np.int32)) <= 0).all()


def test_combine_refuses_bad_arguments_without_a_gpu(sb):
    L = sb._lib
    out = ctypes.c_void_p(1)
    good = sb.CombineOptions(None)
    assert L.lib.sdfhip_scene_combine(None, None, 0, ctypes.byref(good), ctypes.byref(out), None, None) == L.ERR_ARG
    assert b"null" in L.lib.sdfhip_last_error() and out.value is None
    assert L.lib.sdfhip_scene_combine(None, None, 0, None, ctypes.byref(out), None, None) == L.ERR_ARG
    assert L.lib.sdfhip_scene_combine(None, None, 0, ctypes.byref(good), None, None, None) == L.ERR_ARG
    for op in (-1, 3):
        assert L.lib.sdfhip_scene_combine(None, None, op, None, ctypes.byref(out), None, None) == L.ERR_ARG
        assert b"op" in L.lib.sdfhip_last_error()
    for max_depth in (13, -2):
        opt = sb.CombineOptions(max_depth)
        assert L.lib.sdfhip_scene_combine(None, None, 0, ctypes.byref(opt), ctypes.byref(out), None, None) == L.ERR_ARG
        assert b"max_depth" in L.lib.sdfhip_last_error()
    for size in (4, 9, 4100):                           # the size rules of sdfhip_prune_options
        opt = sb.CombineOptions(None)
        opt.size = size
        assert L.lib.sdfhip_scene_combine(None, None, 0, ctypes.byref(opt), ctypes.byref(out), None, None) == L.ERR_ARG
        assert b"bytes" in L.lib.sdfhip_last_error()

    class Newer(ctypes.Structure):
        _fields_ = [("size", ctypes.c_uint32), ("max_depth", ctypes.c_int32), ("unknown", ctypes.c_int32)]
    newer = Newer(12, -1, 5)
    as_options = ctypes.cast(ctypes.byref(newer), ctypes.POINTER(sb.CombineOptions))
    assert L.lib.sdfhip_scene_combine(None, None, 0, as_options, ctypes.byref(out), None, None) == L.ERR_ARG
    assert b"does not know" in L.lib.sdfhip_last_error()
    newer.unknown = -1                                  # a newer struct whose new field says "default" passes the options' check
    assert L.lib.sdfhip_scene_combine(None, None, 0, as_options, ctypes.byref(out), None, None) == L.ERR_ARG
    assert b"null" in L.lib.sdfhip_last_error()


def test_constants_and_records_match_the_header(sb):
    text = open(os.path.join(REPO, "include", "sdfhip.h")).read()
    enums = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bSDFHIP_(COMBINE_[A-Z]+)\s*=\s*(\d+)", text)}
    assert enums == {"COMBINE_UNION": 0, "COMBINE_INTERSECT": 1, "COMBINE_SUBTRACT": 2}
    for name, value in enums.items():
        assert getattr(sb, name) == value == getattr(cr, name)
    record = lambda name: re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    fields = lambda body: [f.strip() for decl in re.findall(r"(?:uint32_t|int32_t|float)\s+([^;]+);", body) for f in decl.split(",")]
    assert fields(record("sdfhip_combine_options")) == [f for f, _ in sb.CombineOptions._fields_]
    assert fields(record("sdfhip_combine_stats")) == [f for f, _ in sb.CombineStats._fields_]
    assert ctypes.sizeof(sb.CombineOptions) == 8 and sb.CombineOptions.max_depth.offset == 4
    assert ctypes.sizeof(sb.CombineStats) == 32 and sb.CombineStats.nodes_shared.offset == 16 and sb.CombineStats.kernel_ms.offset == 20
    opt = sb.CombineOptions()
    assert (opt.size, opt.max_depth) == (8, -1)
    assert "sdfhip_scene_combine" in sb._lib.EXPORTED_SYMBOLS and hasattr(sb.Scene, "Combine")

"""Prune, combine, place and measure on the tree zoo (tests/tree_zoo.py) without a GPU: the four restatements
(tests/prune_restatement.py, combine_restatement.py, place_restatement.py, measure_restatement.py) were written beside breadth-first
trees whose bytes are a distance field, and are held here, on the cases of tests/test_gpu_zoo_builders.py, to things they did not come
from -- what a prune must keep, what a combination of a tree with itself is, min and max at shared nodes, a placed byte computed point
by point, the measure's counts recounted from the links -- before the GPU is held to them.  And the trees are what the GPU tests
need them to be: leaves of many depths within one wave, a 63 against a 64 on a cut edge, children that do not follow the level
order, blocks whose removal byte straddles two words of the bitmap, and no restated result above the cap."""
import numpy as np
import pytest

import combine_restatement as cr
import edit_restatement as er
import measure_restatement as ms
import mesh_restatement as mr
import prune_restatement as pr
import query_restatement as qr
import tree_zoo as tz
from trimesh_restatement import CORNER, from_float

f32 = np.float32
EDGES = [(a, b) for a in range(8) for b in range(8) if a < b and bin(a ^ b).count("1") == 1]        # the cube's twelve edges, by corner


def cell_keys(structs, max_depth=-1):
    """{(depth, x, y, z): index} of the nodes (of depth <= max_depth, if given), from the links"""
    depth, coord = mr.walk(structs)
    keep = np.nonzero(depth <= max_depth)[0] if max_depth >= 0 else np.arange(len(depth))
    return {(int(depth[i]), *map(int, coord[i])): int(i) for i in keep}


def assert_breadth_first(S, what):
    inner = np.nonzero(S[:, 1] >= 0)[0]
    assert (S[inner, 1] == 1 + 8 * np.arange(len(inner))).all(), what
    depth, _ = mr.walk(S)
    assert (np.diff(depth.astype(np.int64)) >= 0).all(), what


# ---- prune -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tz.MESHABLE)
def test_a_pruned_zoo_tree_is_a_consistent_subsequence_of_its_input(name):
    s, v = tz.zoo()[name]
    d0 = er.tree_depth(s)
    keys_in = cell_keys(s)
    for tolerance in tz.PRUNE_TOLERANCES:
        for md in tz.prune_depths(d0):
            S, V = tz.restated_prune(name, tolerance, md)
            what = (name, tolerance, md)
            depth, coord = mr.walk(S)                               # (raises on inconsistent links)
            assert depth.max() == er.tree_depth(S) <= (d0 if md < 0 else min(d0, md)), what
            assert (S[1::8, 0] == S[8::8, 0]).all() and S[0, 0] == -1, what
            inner = np.nonzero(S[:, 1] >= 0)[0]
            assert (S[S[inner, 1], 0] == inner).all(), what           # a block's parent field names the node that points to it
            # the survivors are the input's nodes at the same places, with their bytes, in the input's order
            at = np.array([keys_in[(int(d), *map(int, c))] for d, c in zip(depth, coord)], dtype=np.int64)
            assert (np.diff(at) > 0).all(), what
            assert np.array_equal(V, v[at]), what
            # a survivor that is a leaf now and was none before lost a whole block, and nothing else changes a link
            assert (s[at, 1] >= 0)[S[:, 1] >= 0].all(), what
            if md == 0:
                assert len(S) == 1 and np.array_equal(V[0], v[0]) and S.tolist() == [[-1, -1]], what
            if md >= 0:
                assert len(S) <= int((tz.walked(name)[0] <= md).sum()), what


@pytest.mark.parametrize("name", ["chain12", "dfs_d6_a", "blocks_65", "blocks_1025", "blocks_4097"])
def test_tolerance_0_removes_nothing_from_uniform_bytes(name):
    """uniform bytes: that all 64 bytes of a block equal what the parent interpolates to has probability 256^-64"""
    s, v = tz.zoo()[name]
    S, V = tz.restated_prune(name, 0, -1)
    assert np.array_equal(S, s) and np.array_equal(V, v), "array for array, in the source's own order"
    assert S is not s and V is not v


# ---- combine ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain12", "dfs_d6_a", "dfs_d6_b", "blocks_4097", "leaf"])
def test_a_tree_united_or_intersected_with_itself_keeps_its_bytes(name):
    s, v = tz.zoo()[name]
    keys_in = cell_keys(s)
    for op in (cr.COMBINE_UNION, cr.COMBINE_INTERSECT):
        S, V, counts = (tz.restated_combine(name, name, op, -1) if name == "chain12" else cr.combine((s, v), (s, v), op, want_counts=True))
        assert len(S) == len(s) and counts == {"nodes_shared": len(s), "depth_out": er.tree_depth(s)}, (name, op)
        assert_breadth_first(S, (name, op))
        keys_out = cell_keys(S)
        assert keys_out.keys() == keys_in.keys(), (name, op)
        order = np.array([keys_in[k] for k in sorted(keys_out, key=keys_out.get)], dtype=np.int64)       # the input's index of result node 0, 1, ...
        assert np.array_equal(V, v[order]), (name, op)
        assert np.array_equal(S[:, 1] >= 0, s[order, 1] >= 0), (name, op)


@pytest.mark.parametrize("a, b", tz.COMBINE_PAIRS + tz.COMBINE_REVERSED, ids=["-".join(p) for p in tz.COMBINE_PAIRS + tz.COMBINE_REVERSED])
def test_combined_cells_are_both_operands_and_shared_bytes_are_min_and_max(a, b):
    (sa, va), (sb_, vb) = tz.zoo()[a], tz.zoo()[b]
    for md in tz.COMBINE_DEPTHS:
        ka, kb = cell_keys(sa, md), cell_keys(sb_, md)
        both = sorted(ka.keys() & kb.keys())
        ia, ib = np.array([ka[k] for k in both]), np.array([kb[k] for k in both])
        sizes = set()
        for op in cr.OPS:
            if (a, b, op, md) not in tz.combine_cases():
                continue
            S, V, counts = tz.restated_combine(a, b, op, md)
            what = (a, b, op, md)
            assert_breadth_first(S, what)
            keys = cell_keys(S)
            assert keys.keys() == ka.keys() | kb.keys(), what
            assert counts["nodes_shared"] == len(both) and counts["depth_out"] == max(k[0] for k in keys) == er.tree_depth(S), what
            at = np.array([keys[k] for k in both])
            if op == cr.COMBINE_UNION:
                assert np.array_equal(V[at], np.minimum(va[ia], vb[ib])), what
            elif op == cr.COMBINE_INTERSECT:
                assert np.array_equal(V[at], np.maximum(va[ia], vb[ib])), what
            else:                                   # a - b = max(a, -b): never further inside than a
                assert (V[at] >= va[ia]).all(), what
            # a node is a leaf exactly where neither operand goes on (or the cut ends it)
            leaf_a = {k for k, i in ka.items() if sa[i, 1] < 0 or k[0] == md}
            leaf_b = {k for k, i in kb.items() if sb_[i, 1] < 0 or k[0] == md}
            leaves = {k for k, i in keys.items() if S[i, 1] < 0}
            assert leaves == {k for k in keys if (k in leaf_a or k not in ka) and (k in leaf_b or k not in kb)}, what
            sizes.add(len(S))
        assert len(sizes) == 1, "the structure does not depend on the operation"


# ---- place -----------------------------------------------------------------------------------------------------------------------
# (chain14: the 14-deep chain, which the GPU places with a depth given and by the walk along the links alone -- the sample accepts it)
@pytest.mark.parametrize("src, depth", [(s, d) for s, name, d in tz.place_cases() if name == "identity"] + [("chain14", 4)])
def test_identity_placed_bytes_are_the_sources_sampled_point_by_point(src, depth):
    """The identity maps a corner of the result onto itself exactly (q = ((1 d0 + 0 d1) + 0 d2) * 1 with d = p - 0, and the corner
    is a float32), so a result byte is from_float of the source's sampled distance at that corner at the node's own scale: computed
    here one point at a time from the result's own links, with no level loop and no merging of equal points."""
    s, v = tz.zoo()[src]
    S, V, counts = tz.restated_place(src, "identity", depth)
    d_out, coord = mr.walk(S)
    assert d_out.max() == counts["depth_out"] == depth == counts["levels"] - 1
    assert counts["samples"] == 9 + 35 * ((len(S) - 1) // 8)
    assert_breadth_first(S, (src, depth))
    rng = np.random.default_rng(401)
    nodes = np.concatenate([[0, len(S) - 1], rng.integers(0, len(S), size=300)])
    scale = np.ldexp(f32(1), -d_out[nodes]).astype(f32)
    points = (coord[nodes][:, None, :] + CORNER[None]).astype(f32) * scale[:, None, None]           # (m, 8, 3): each corner from its own node
    got = qr.sample(s, v, points.reshape(-1, 3))                    # (every lane of a sample is looked up on its own, from the root)
    assert (got["status"] == qr.HIT).all()
    want = from_float(got["distance"].astype(f32).reshape(-1, 8), scale[:, None])
    bad = np.nonzero((V[nodes] != want).any(1))[0]
    assert not len(bad), (src, depth, nodes[bad][:4].tolist(), V[nodes[bad][:4]].tolist(), want[bad[:4]].tolist())


# ---- measure ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tz.MESHABLE)
def test_the_measures_counts_are_the_links_and_its_bounds_lie_in_the_cube(name):
    s, v = tz.zoo()[name]
    depth, _ = tz.walked(name)
    leaf = s[:, 1] < 0
    for level in tz.mesh_levels(er.tree_depth(s)):
        m = tz.restated_measure(name, level)
        cell = leaf if level < 0 else (leaf & (depth <= level)) | (~leaf & (depth == level))
        what = (name, level)
        assert m.cells == int(cell.sum()) and (m.nodes, m.depth) == (len(s), int(depth.max())), what
        assert np.array_equal(m.cells_at_depth, np.bincount(depth[cell], minlength=13)), what
        assert m.cells_inside + m.cells_cut == int((v[cell] <= 63).any(1).sum()), what
        assert m.cells_inside == int((v[cell] <= 63).all(1).sum()), what
        if m.cells_inside + m.cells_cut:
            assert (0.0 <= m.bounds_min).all() and (m.bounds_min <= m.bounds_max).all() and (m.bounds_max <= 1.0).all(), what
            assert 0.0 < m.volume <= 1.0 and np.isfinite(m.doubles()).all(), what
        else:
            assert np.isposinf(m.bounds_min).all() and np.isneginf(m.bounds_max).all() and m.volume == 0.0, what


def test_the_volume_of_flat_cells_is_the_sum_of_their_boxes_bit_for_bit():
    """blocks_2049: every cell flat, all 63 or all 64 -- no cell is cut, and the volume is a sum of powers of two no smaller than
    8^-7 = 2^-21 and below 1: exact in fp64 in any order of addition"""
    s, v = tz.zoo()["blocks_2049"]
    depth, _ = tz.walked("blocks_2049")
    m = tz.restated_measure("blocks_2049", -1)
    inside = (s[:, 1] < 0) & (v == 63).all(1)
    want = np.float64(sum(8.0 ** -int(d) for d in depth[inside]))
    assert m.cells_cut == 0 and m.area == 0.0 and m.cells_inside == int(inside.sum()) > 500
    assert ms.same_bits(m.volume, want) and 0.0 < want < 1.0


@pytest.mark.parametrize("name", ["dfs_d6_b", "blocks_4097"])
def test_the_area_is_the_restated_meshs(name):
    """the comparison of tests/test_measure.py (test_volume_and_area_are_the_meshs) under its bound, 1e-6: the mesh's vertices are
    float32.  These meshes are not closed (the bytes are no distance field), so the divergence theorem's volume does not apply."""
    s, v = tz.zoo()[name]
    tris = mr.mesh(s, v, walked=tz.walked(name))
    _, area = ms.mesh_volume_area(tris)
    m = tz.restated_measure(name, -1)
    print(f"{name}: area {m.area!r} against the mesh's {area!r} ({m.area / area - 1:.2e})")
    assert abs(m.area - area) <= 1e-6 * area
    assert (m.cells, m.cells_cut, len(tris)) == mr.count(s, v, walked=tz.walked(name))


# ---- what the cases are for ------------------------------------------------------------------------------------------------------
def test_the_cases_are_what_they_are_for():
    z = tz.zoo()
    # leaves of at least four depths among 64 consecutive nodes: k_measure_cells counts cells per depth with one ballot per depth
    for name in ("blocks_1025", "blocks_4097"):
        s = z[name][0]
        depth, _ = tz.walked(name)
        leaf = s[:, 1] < 0
        most = max(len(np.unique(depth[w:w + 64][leaf[w:w + 64]])) for w in range(0, len(s), 64))
        assert most >= 4, (name, most)
    # a cut cell with an inside 63 against an outside 64 on one edge: the cut point's divisor is 1 byte
    for name in ("dfs_d6_b", "blocks_257"):
        s, v = z[name]
        leaf = s[:, 1] < 0
        assert sum(int((leaf & (np.minimum(v[:, a], v[:, b]) == 63) & (np.maximum(v[:, a], v[:, b]) == 64)).sum()) for a, b in EDGES) > 100, name
    # depth-first order: a node's block may lie behind the blocks of deeper nodes (breadth first, the children index grows with the level)
    s = z["dfs_d6_a"][0]
    by_level = [lv[s[lv, 1] >= 0] for lv in pr.levels(s)]
    first = [s[lv, 1] for lv in by_level if len(lv)]
    assert any(upper.max() > lower.min() for upper, lower in zip(first, first[1:]))
    assert (np.diff(tz.walked("dfs_d6_a")[0][1::8].astype(np.int64)) < 0).any()
    # a block at an index with first & 31 == 25: its eight bits of the removal bitmap straddle two words
    for name in tz.MESHABLE[1:]:
        s = z[name][0]
        assert ((s[s[:, 1] >= 0, 1] & 31) == 25).any(), name
    # ... and such a block is removed in a case where not everything is: chain12 and dfs_d6_a cut one level inside the tree
    for name in ("chain12", "dfs_d6_a", "blocks_4097"):
        s = z[name][0]
        d0 = er.tree_depth(s)
        depth, _ = tz.walked(name)
        S, _ = tz.restated_prune(name, 8, d0 - 1)
        gone = s[(depth == d0 - 1) & (s[:, 1] >= 0), 1]
        assert 1 < len(S) == len(s) - 8 * len(gone) and ((gone & 31) == 25).any(), name
    # the sizes
    assert [len(tz.restated_prune(n, 8, er.tree_depth(z[n][0]) - 1)[0]) for n in ("dfs_d6_a", "blocks_1017", "blocks_2049", "blocks_4097", "chain12")] \
        == [1617, 545, 1, 2561, 89]
    assert [len(tz.restated_combine(a, b, cr.COMBINE_UNION, -1)[0]) for a, b in tz.COMBINE_PAIRS] == [17977, 13073, 1113, 257, 97]
    assert tz.restated_combine("blocks_1025", "chain12", cr.COMBINE_UNION, -1)[2]["depth_out"] == 12
    assert len(tz.restated_place("dfs_d6_a", "identity", 6)[0]) == 75753 > 8 * len(z["dfs_d6_a"][0])      # the builder's arrays grow more than once
    assert len(tz.restated_place("chain12", "identity", 6)[0]) == 45265 and len(tz.restated_place("blocks_1025", "identity", 6)[0]) == 110489
    at_4 = [len(tz.restated_place(s, n, d)[0]) for s, n, d in tz.place_cases() if d == 4]
    assert len(at_4) == 15 and 1937 == min(at_4) and max(at_4) == 4041
    sizes = [len(tz.restated_prune(n, t, md)[0]) for n in tz.MESHABLE for t in tz.PRUNE_TOLERANCES for md in tz.prune_depths(er.tree_depth(z[n][0]))]
    sizes += [len(tz.restated_combine(*c)[0]) for c in tz.combine_cases()]
    sizes += [len(tz.restated_place(*c)[0]) for c in tz.place_cases()]
    sizes += [len(tz.restated_place("chain14", n, 4)[0]) for n in tz.PLACE_NAMES]
    assert len(sizes) == 87 + 32 + 25 + 3 and max(sizes) <= tz.NODE_CAP, max(sizes)

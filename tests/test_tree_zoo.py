"""The tree zoo (tests/tree_zoo.py) without a GPU: its trees are what they claim to be, the three restatements hold on them against
the frozen oracle and their own invariants, and the preconditions that make tests/test_gpu_tree_zoo.py meaningful are true -- every
(tetrahedron, mask) pair is meshed, the second brush of a chain splits inside the blocks the first appended, one call outgrows the
edit's initial capacity, and no restated result is larger than the cap."""
import numpy as np
import pytest

import edit_restatement as er
import mesh_restatement as mr
import query_restatement as qr
import tree_zoo as tz
from conftest import CAMERAS, bits_equal, make_camera
from test_edit import assert_edit_order
from test_query import SKY, point_sets


def od_of(sb, name):
    s, v = tz.zoo()[name]
    return sb.OctData(s.copy(), v.copy())


def test_the_zoo_is_what_it_says(sb):
    z = tz.zoo()
    assert sorted(z) == sorted(tz.ALL_TREES)
    for name, (s, v) in z.items():
        assert s.dtype == np.int32 and v.dtype == np.uint8 and s.shape == (len(s), 2) and v.shape == (len(s), 8), name
        depth, consistent = od_of(sb, name).validate()
        assert consistent, name                                   # (chain14 is consistent too: it is its depth the upload refuses)
        assert depth == er.tree_depth(s), name
    assert z["leaf"][0].tolist() == [[-1, -1]] and z["leaf"][1].tolist() == [tz.LEAF_BYTES]
    assert er.tree_depth(z["chain12"][0]) == 12 and er.tree_depth(z["chain14"][0]) == 14
    assert [len(z[f"blocks_{1 + 8 * k}"][0]) for k in tz.BLOCK_COUNTS] == [65, 257, 1017, 1025, 2049, 4097]
    for tag in "ab":
        s = z[f"dfs_d6_{tag}"][0]
        assert er.tree_depth(s) == 6 and 4097 < len(s) <= 9000
        # depth-first order: blocks are not sorted by depth (a builder's level order would be)
        depth, _ = mr.walk(s)
        assert (np.diff(depth[1::8].astype(np.int64)) < 0).any()
    depth, _ = mr.walk(z["blocks_4097"][0])
    assert (np.diff(depth[1::8].astype(np.int64)) < 0).any()
    # the fillers
    rng = np.random.default_rng(3)
    assert len(np.unique(tz.fill_uniform(rng, 4000))) == 256
    assert np.unique(tz.fill_iso(rng, 500)).tolist() == [0, 63, 64, 255]
    flat = tz.fill_mostly_flat(rng, 2000)
    share = float((flat.min(1) == flat.max(1)).mean())
    assert 0.7 < share < 0.9
    f = tz.fill_flat_63_64(rng, 500)
    assert (f.min(1) == f.max(1)).all() and np.unique(f).tolist() == [63, 64]
    assert np.unique(z["dfs_d6_b"][1]).tolist() == [0, 63, 64, 255] and len(np.unique(z["chain12"][1])) > 200


def test_tree_with_blocks_counts_and_caps_its_depth(sb):
    for k, md in ((0, 3), (1, 1), (9, 2), (73, 3), (300, 12)):
        s, v = tz.tree_with_blocks(np.random.default_rng(k), k, md)
        assert len(s) == 1 + 8 * k == len(v)
        depth, consistent = sb.OctData(s, v).validate()
        assert consistent and depth <= md and (k == 0 or depth >= 1)
        assert (s[1::8, 0] == s[8::8, 0]).all()                    # blocks of eight under one parent
    with pytest.raises(ValueError):
        tz.tree_with_blocks(np.random.default_rng(0), 10, 2)       # a depth-2 tree has room for 9 blocks


@pytest.mark.parametrize("name", tz.ALL_TREES)
def test_sample_is_the_oracles_distance_at_on_the_zoo(sb, oracle_mod, name):
    od = od_of(sb, name)
    for what, pts in point_sets(od, 11).items():
        got = qr.sample(od.Structs, od.Values, pts)
        assert (got["status"] == qr.HIT).all()
        want = np.array([oracle_mod.distance_at(od.Structs, od.Values, *p) for p in pts], dtype=np.float64)
        assert bits_equal(got["distance"], want[:, 0].astype(np.float32)).all(), (name, what)
        assert (got["node"] == want[:, 1].astype(np.uint32)).all(), (name, what)
        assert bits_equal(got["scale"], want[:, 2].astype(np.float32)).all(), (name, what)


_pick_classes = {}


@pytest.mark.parametrize("name", tz.ALL_TREES)
def test_pick_agrees_with_the_oracles_frames_on_the_zoo(sb, oracle_mod, name):
    """ESCAPED exactly where the oracle's pixel is the sky constant, and there steps == alpha; everywhere else HIT or EXHAUSTED with
    steps <= alpha (alpha also counts the shadow march's steps)."""
    s, v = tz.zoo()[name]
    W, H = 48, 40
    ys, xs = np.mgrid[0:H, 0:W]
    pixels = np.stack([xs.ravel(), ys.ravel()], 1)
    for cam_name in CAMERAS:
        cam = make_camera(cam_name, W, H)
        rgba = oracle_mod.render(s, v, cam.State, W, H)[0].reshape(-1, 4)
        got = qr.pick(s, v, cam.State, pixels)
        sky = (rgba[:, :3].view(np.uint32) == SKY.view(np.uint32)).all(1)
        alpha = rgba[:, 3]
        assert np.isfinite(alpha).all()
        assert ((got["status"] == qr.ESCAPED) == sky).all(), (name, cam_name, int(((got["status"] == qr.ESCAPED) != sky).sum()))
        assert (got["steps"][sky] == alpha[sky]).all(), (name, cam_name)
        assert np.isin(got["status"][~sky], (qr.HIT, qr.EXHAUSTED)).all(), (name, cam_name)
        assert (got["steps"][~sky] <= alpha[~sky]).all(), (name, cam_name)
        assert (got["steps"][got["status"] == qr.EXHAUSTED] == 100).all()
        _pick_classes[name] = _pick_classes.get(name, 0) | (1 if sky.any() else 0) | (2 if (~sky).any() else 0)
    # (blocks_2049: every byte is 63 or 64, every point within a byte's worth of the surface -- no ray escapes)
    assert _pick_classes[name] == (2 if name == "blocks_2049" else 3), "both classes occur among the three cameras"


def cell_masks(s, v, level, walked):
    """the (tetrahedron, mask) pairs of the cut cells of `level`, as the restatement defines them: a (6, 16) count"""
    depth, _ = walked
    V = np.asarray(v)
    cut = np.nonzero(mr.cells_of(s, level, depth) & (V.min(1) <= 63) & (V.max(1) > 63))[0]
    seen = np.zeros((6, 16), dtype=np.int64)
    for t in range(6):
        ins = V[cut][:, mr.TETS[t]] <= 63
        seen[t] += np.bincount(ins[:, 0] + 2 * ins[:, 1] + 4 * ins[:, 2] + 8 * ins[:, 3], minlength=16)
    return seen, cut


def test_the_zoos_meshes_use_every_table_entry_and_count_is_len_of_mesh():
    seen = np.zeros((6, 16), dtype=np.int64)
    inner_cut = 0
    for name in tz.MESHABLE:
        s, v = tz.zoo()[name]
        walked = mr.walk(s)
        for level in tz.mesh_levels(er.tree_depth(s)):
            tris, nodes, (cells, cut) = mr.mesh(s, v, level, want_cells=True, walked=walked)
            assert mr.count(s, v, level, walked=walked) == (cells, cut, len(tris)), (name, level)
            m, cut_nodes = cell_masks(s, v, level, walked)
            assert len(cut_nodes) == cut and int((m * mr.NTRI[None, :]).sum()) == len(tris), (name, level)
            assert np.array_equal(np.unique(nodes), cut_nodes)                       # every cut cell gave a triangle
            seen += m
            if level >= 0:
                inner_cut += int((np.asarray(s)[cut_nodes, 1] >= 0).sum())
    # every (tetrahedron, mask) with a non-zero triangle count: the precondition of the GPU comparison of MESH_TRIANGLES
    assert (seen[:, 1:15] > 0).all(), np.argwhere(seen[:, 1:15] == 0).tolist()
    assert inner_cut > 100, "internal nodes with mixed bytes are meshed as cells of a level >= 0"
    s, v = tz.zoo()["blocks_2049"]
    assert mr.count(s, v, -1)[1:] == (0, 0)                                          # flat 63 / 64 cells: nothing is cut
    for name in ("blocks_65", "blocks_257", "blocks_1025", "blocks_4097"):           # the node one past the boundary is a cut cell
        s, v = tz.zoo()[name]
        assert s[-1, 1] < 0 and v[-1].min() <= 63 < v[-1].max(), name


@pytest.mark.parametrize("name", tz.EDITED)
def test_restated_edits_of_the_zoo_are_consistent_in_order_and_under_the_cap(sb, name):
    s, v = tz.zoo()[name]
    d0 = er.tree_depth(s)
    added = []
    for label, e in tz.single_edits(name):
        for md in tz.max_depths(d0):
            S, V = tz.restated_edit(name, [e], md)
            what = (name, label, md)
            assert len(S) <= tz.NODE_CAP, what
            depth, consistent = sb.OctData(S, V).validate()
            assert consistent and d0 <= depth <= max(d0, md), what
            assert_edit_order(s, S)
            assert not np.array_equal(V[:len(s)], v), what                             # every case changes bytes
            added.append(len(S) - len(s))
    assert max(added) > 0
    if name == "chain12":
        # the brush in the deep corner: bytes change at depth >= 10, and leaves split
        depth, _ = mr.walk(s)
        for label, e in tz.single_edits(name):
            S, V = tz.restated_edit(name, [e], -1)
            assert ((V[:len(s)] != v).any(1) & (depth >= 10)).any() and len(S) > len(s), label
    # the overlapping chain: two calls, and the list
    a, md_a, b, md_b = tz.overlapping_chain(name, d0)
    (SA, VA), (SB, VB), (SL, VL) = tz.restated_chain(name)
    for S, V, before in ((SA, VA, s), (SB, VB, SA)):
        assert len(S) <= tz.NODE_CAP
        assert sb.OctData(S, V).validate()[1]
        assert_edit_order(before, S)
    assert er.tree_depth(SA) == min(d0 + 2, 12) or name == "leaf"
    # B split inside the blocks A added: nodes B appended whose parent is not a node of the input
    assert len(SB) > len(SA) and (SB[len(SA):, 0] >= len(s)).any(), name
    assert (SL[:, 0] >= len(s)).any()
    # a list is its edits chained at the list's depth
    S1, V1 = tz.restated_edit(name, [a], md_b)
    S2, V2 = tz.restated_edit(name, [b], md_b, start=("after A at B's depth", S1, V1))
    assert np.array_equal(SL, S2) and np.array_equal(VL, V2)
    assert len(SL) <= tz.NODE_CAP and sb.OctData(SL, VL).validate()[1]
    assert_edit_order(s, S1); assert_edit_order(S1, SL)            # (the pinned order is per edit)


def test_one_call_outgrows_the_edits_initial_capacity():
    """sdfhip_scene_edit starts with room for n + n / 16 + 4096 nodes and grows from there: at least one case must need more in ONE
    call, and the list form of a chain must take a tree that has grown into its second brush (whose index bitmap was sized for the
    input)."""
    grew = []
    for name in tz.EDITED:
        s, v = tz.zoo()[name]
        d0 = er.tree_depth(s)
        for label, e in tz.single_edits(name):
            S, _ = tz.restated_edit(name, [e], tz.max_depths(d0)[1])
            if len(S) - len(s) > len(s) // 16 + 4096:
                grew.append((name, label))
        (SA, _), _, (SL, _) = tz.restated_chain(name)
    assert ("dfs_d6_a", "add sphere") in grew and ("blocks_1025", "add box") in grew and ("blocks_4097", "add box") in grew, grew

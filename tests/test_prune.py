"""Pruning (sdfhip_scene_prune) without a GPU: the CPU restatement (tests/prune_restatement.py) is held to the rule's properties and
to node counts from an independent prototype of the rule; the entry point refuses what it must refuse before it touches a device.
tests/test_gpu_prune.py holds the GPU to the restatement byte for byte.

One count differs from the figure the prototype reported.  For max_depth 4 on the depth-5 sphere it gave 3 465 nodes: that is the
number of nodes of depth <= 4, i.e. the cut ALONE.  The pinned rule has no prune without a tolerance (-1 means 0), and at tolerance 0
it finds 160 of the level-4 blocks redundant once the cut has made their children leaves (the same 160 blocks that are gone from
level 4 after the plain tolerance-0 prune: 7 881 nodes, 2 185 of them of depth <= 4).  The rule gives 2 185; both figures are
asserted below for what they are."""
import ctypes

import numpy as np
import pytest

import edit_restatement as er
import prune_restatement as pr
import tree_zoo

SPHERE_ADD = (er.EDIT_ADD, er.BRUSH_SPHERE, (0.5, 0.5, 0.5, 0.3))


@pytest.fixture(scope="module")
def T():
    """the depth-5 sphere an edit makes from an empty root: 13 385 nodes"""
    root = (np.array([[-1, -1]], dtype=np.int32), np.full((1, 8), 255, dtype=np.uint8))
    S, V = er.edit(*root, [SPHERE_ADD], 5)
    S.setflags(write=False); V.setflags(write=False)
    return S, V


@pytest.fixture(scope="module")
def carved_away(T):
    return er.edit(*T, [(er.EDIT_CARVE, er.BRUSH_SPHERE, (0.5, 0.5, 0.5, 1.2))], 5)


@pytest.fixture(scope="module")
def carved_box(T):
    return er.edit(*T, [(er.EDIT_CARVE, er.BRUSH_BOX, (0.5, 0.5, 0.5, 0.15, 0.5, 0.15))], 6)


def assert_consistent(sb, S, V):
    """node 0 is the root, every child's parent points back, the blocks of eight are contiguous and tile 1 .. n - 1, and
    sdfhip_octdata_validate accepts the tree"""
    n = len(S)
    assert S.dtype == np.int32 and V.dtype == np.uint8 and V.shape == (n, 8) and (n - 1) % 8 == 0
    assert S[0, 0] < 0
    inner = np.nonzero(S[:, 1] >= 0)[0]
    starts = S[inner, 1].astype(np.int64)
    assert (np.sort(starts) == 1 + 8 * np.arange((n - 1) // 8)).all(), "the blocks do not tile the nodes behind the root"
    assert (S[starts[:, None] + np.arange(8), 0] == inner[:, None]).all(), "a child's parent does not point back"
    depth, consistent = sb.OctData(S, V).validate()
    assert consistent and depth == er.tree_depth(S)
    return depth


def assert_survivors_in_order(before, after):
    """`after` is `before` with whole blocks taken out: the survivors in their order, bytes untouched, links remapped, a node that
    lost its block a leaf"""
    (S0, V0), (S1, V1) = before, after
    n0, n1 = len(S0), len(S1)
    assert (n0 - n1) % 8 == 0
    # recover the survivors: walk the result and the input together from the root (child i of a survivor is child i of its original)
    old = np.full(n1, -1, dtype=np.int64)
    old[0] = 0
    level = np.zeros(1, dtype=np.int64)
    while len(level):
        inner = level[S1[level, 1] >= 0]
        assert (S0[old[inner], 1] >= 0).all(), "a survivor has children its original had not"
        kids = (S1[inner, 1].astype(np.int64)[:, None] + np.arange(8)).reshape(-1)
        old[kids] = (S0[old[inner], 1].astype(np.int64)[:, None] + np.arange(8)).reshape(-1)
        level = kids
    assert (old >= 0).all() and (np.diff(old) > 0).all(), "the survivors are out of order"
    assert np.array_equal(V1, V0[old]), "a surviving byte changed"
    assert (S1[1:, 0] == np.searchsorted(old, S0[old[1:], 0])).all(), "a parent field is not the parent's new index"


def both(sb, before, tolerance=0, max_depth=-1):
    after = pr.prune(*before, tolerance, max_depth)
    assert_consistent(sb, *after)
    assert_survivors_in_order(before, after)
    return after


def test_the_sphere_is_the_prototypes(T):
    assert len(T[0]) == 13385 and er.tree_depth(T[0]) == 5


@pytest.mark.parametrize("tolerance, nodes", [(0, 7881), (1, 7625), (2, 7625), (4, 7561), (8, 6025)])
def test_node_counts_by_tolerance(sb, T, tolerance, nodes):
    assert len(both(sb, T, tolerance)[0]) == nodes


@pytest.mark.parametrize("max_depth, nodes", [(0, 1), (2, 73), (4, 2185)])
def test_node_counts_by_max_depth(sb, T, max_depth, nodes):
    S, V = both(sb, T, 0, max_depth)
    assert len(S) == nodes and er.tree_depth(S) <= max_depth


def test_the_cut_alone_at_depth_4_is_the_prototypes_figure(T):
    # (see the module's docstring) 3 465 = the nodes of depth <= 4; tolerance 0 then removes 160 blocks of level 4
    per_level = [len(level) for level in pr.levels(T[0])]
    assert sum(per_level[:5]) == 3465
    assert 3465 - 8 * 160 == 2185 == sum(len(level) for level in pr.levels(pr.prune(*T, 0)[0])[:5])


def test_a_carved_away_tree_cascades_through_four_levels(sb, carved_away):
    assert len(carved_away[0]) == 13385
    S, V = both(sb, carved_away, 0)
    assert len(S) == 9 and (V[0] == 135).all() and er.tree_depth(S) == 1


def test_a_box_carved_through_the_sphere(sb, carved_box):
    assert len(carved_box[0]) == 24073
    assert len(both(sb, carved_box, 0)[0]) == 14025
    assert len(both(sb, carved_box, 1)[0]) == 9993


def trees(sb, T, carved_away, carved_box):
    od = sb.sphere_d4()
    out = {"T": T, "carved_away": carved_away, "carved_box": carved_box, "sphere_d4": (od.Structs, od.Values)}
    out.update({f"zoo_{k}": v for k, v in tree_zoo.zoo().items()})
    return out


def test_properties_on_every_tree(sb, T, carved_away, carved_box):
    for name, before in trees(sb, T, carved_away, carved_box).items():
        d0 = er.tree_depth(before[0])
        for tolerance, max_depth in ((0, -1), (1, -1), (8, -1), (0, max(d0 - 1, 0)), (3, 2)):
            once = both(sb, before, tolerance, max_depth)
            twice = pr.prune(*once, tolerance, max_depth)
            assert np.array_equal(twice[0], once[0]) and np.array_equal(twice[1], once[1]), f"{name}: prune of prune is not prune"
            assert len(once[0]) <= len(before[0])
            if max_depth >= 0:
                assert er.tree_depth(once[0]) <= max_depth
        root_only = pr.prune(*before, 255)
        assert len(root_only[0]) == 1 and root_only[0][0, 1] == -1 and (root_only[1][0] == before[1][0]).all(), name
        assert len(pr.prune(*before, 0, 0)[0]) == 1, name
        assert len(pr.prune(*before, -1)[0]) == len(pr.prune(*before, 0)[0]), f"{name}: tolerance -1 is the default, 0"


def test_splitting_every_leaf_changes_nothing_a_prune_keeps(sb, T, carved_away, carved_box):
    for name, before in trees(sb, T, carved_away, carved_box).items():
        split = pr.split_leaves(*before)
        assert len(split[0]) > len(before[0])
        if name == "T":
            assert len(split[0]) == 107081
        assert_consistent(sb, *split)
        a, b = pr.prune(*split, 0), pr.prune(*before, 0)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), name
        if name == "T":
            assert len(a[0]) == 7881


def test_a_tree_with_nothing_redundant_and_a_one_node_tree_are_clones(sb, T):
    leaf = tree_zoo.zoo()["leaf"]
    for tolerance, max_depth in ((0, -1), (255, -1), (0, 0), (7, 5)):
        S, V = pr.prune(*leaf, tolerance, max_depth)
        assert np.array_equal(S, leaf[0]) and np.array_equal(V, leaf[1])
    pruned = pr.prune(*T, 0)
    S, V = pr.prune(*pruned, 0)
    assert np.array_equal(S, pruned[0]) and np.array_equal(V, pruned[1])
    assert S is not pruned[0] and V is not pruned[1]


def test_prune_refuses_bad_arguments_without_a_gpu(sb):
    L = sb._lib
    out = ctypes.c_void_p(1)
    good = sb.PruneOptions(0, None)
    assert L.lib.sdfhip_scene_prune(None, ctypes.byref(good), ctypes.byref(out), None, None) == L.ERR_ARG
    assert b"null" in L.lib.sdfhip_last_error() and out.value is None
    assert L.lib.sdfhip_scene_prune(None, None, ctypes.byref(out), None, None) == L.ERR_ARG
    assert L.lib.sdfhip_scene_prune(None, ctypes.byref(good), None, None, None) == L.ERR_ARG
    for opt, word in ((sb.PruneOptions(256, None), b"tolerance"), (sb.PruneOptions(-2, None), b"tolerance"),
                      (sb.PruneOptions(0, 13), b"max_depth"), (sb.PruneOptions(0, -2), b"max_depth")):
        assert L.lib.sdfhip_scene_prune(None, ctypes.byref(opt), ctypes.byref(out), None, None) == L.ERR_ARG
        assert word in L.lib.sdfhip_last_error()
    # the size rules of sdfhip_mesh_options: too small, not a multiple of 4, an unknown field that is set
    for size in (8, 13, 4100):
        opt = sb.PruneOptions(0, None)
        opt.size = size
        assert L.lib.sdfhip_scene_prune(None, ctypes.byref(opt), ctypes.byref(out), None, None) == L.ERR_ARG
        assert b"bytes" in L.lib.sdfhip_last_error()

    class Newer(ctypes.Structure):
        _fields_ = [("size", ctypes.c_uint32), ("tolerance", ctypes.c_int32), ("max_depth", ctypes.c_int32), ("unknown", ctypes.c_int32)]
    newer = Newer(16, 0, -1, 5)
    assert L.lib.sdfhip_scene_prune(None, ctypes.cast(ctypes.byref(newer), ctypes.POINTER(sb.PruneOptions)), ctypes.byref(out), None, None) == L.ERR_ARG
    assert b"does not know" in L.lib.sdfhip_last_error()
    newer.unknown = -1                                  # a newer struct whose new field says "default" passes the options' check
    assert L.lib.sdfhip_scene_prune(None, ctypes.cast(ctypes.byref(newer), ctypes.POINTER(sb.PruneOptions)), ctypes.byref(out), None, None) == L.ERR_ARG
    assert b"null" in L.lib.sdfhip_last_error()


def test_the_binding_names_the_symbol_and_mirrors_the_records(sb):
    assert "sdfhip_scene_prune" in sb._lib.EXPORTED_SYMBOLS
    assert ctypes.sizeof(sb.PruneOptions) == 12 and sb.PruneOptions.max_depth.offset == 8
    assert ctypes.sizeof(sb.PruneStats) == 28 and sb.PruneStats.kernel_ms.offset == 16
    assert hasattr(sb.Scene, "Prune")
    opt = sb.PruneOptions()
    assert (opt.size, opt.tolerance, opt.max_depth) == (12, -1, -1)

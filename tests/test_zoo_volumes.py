"""Volume out and compose on the tree zoo (tests/tree_zoo.py) without a GPU: the two restatements (tests/volume_restatement.py,
compose_restatement.py) were written beside breadth-first trees whose bytes are a distance field, and are held here, on the cases of
tests/test_gpu_zoo_volumes.py, to things they did not come from -- the placement's restatement of the same case, the sampler's, the
slope of the continuation -- before the GPU is held to them.  And the cases are what the GPU tests need them to be: their sizes are
pinned, the arrays grow, the stride loop makes a second trip, and no restated result is above the cap."""
import numpy as np
import pytest

import compose_restatement as cpr
import edit_restatement as er
import query_restatement as qr
import tree_zoo as tz
import volume_restatement as vr

f32 = np.float32


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- compose ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", list(tz.PLACE_DEPTHS))
def test_one_instance_of_a_zoo_tree_is_its_restated_placement(src):
    for _, name, depth in tz.place_cases(src):
        if depth > 4 and name != "identity":
            continue                                                # (the deeper ones once: they take seconds)
        want = tz.restated_place(src, name, depth)
        got = cpr.compose([(tz.zoo()[src], tz.place_args(name))], depth, want_counts=True)
        assert same(got, want) and got[2] == want[2], (src, name, depth)


def test_the_14_deep_chain_composes_only_with_a_depth_given():
    got = cpr.compose([(tz.zoo()["chain14"], tz.place_args("identity"))], 4, want_counts=True)
    want = tz.restated_place("chain14", "identity", 4)
    assert same(got, want) and got[2] == want[2]
    assert er.tree_depth(tz.zoo()["chain14"][0]) == 14 > 12, "with no depth the library has none to take: ERR_BAD_TREE on the GPU"


def test_a_composition_of_zoo_trees_is_the_fold_of_their_placements_values():
    """the root's bytes and a deep node's, from plr.value of each instance folded by hand: no level loop"""
    import place_restatement as plr
    from trimesh_restatement import CORNER, from_float
    import mesh_restatement as mr
    for name, depth in tz.compose_cases():
        S, V, _ = tz.restated_compose(name, depth)
        d_out, coord = mr.walk(S)
        rng = np.random.default_rng(17)
        nodes = np.concatenate([[0, len(S) - 1], rng.integers(0, len(S), size=40)])
        scale = np.ldexp(f32(1), -d_out[nodes]).astype(f32)
        p = ((coord[nodes][:, None, :] + CORNER[None]).astype(f32) * scale[:, None, None]).reshape(-1, 3)
        v = None
        for src, pl, op in tz.compose_parts(name):
            u = plr.value(tz.zoo()[src], p, *pl)
            v = u if v is None else np.minimum(v, u) if op == 0 else np.maximum(v, u) if op == 1 else np.maximum(v, -u)
        assert np.array_equal(V[nodes], from_float(v.reshape(-1, 8), scale[:, None])), (name, depth)


# ---- volume out ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tz.ALL_TREES)
def test_out_inside_the_cube_is_the_restated_sample(name):
    s, v = tz.zoo()[name]
    for lattice in tz.out_lattices():
        p = vr.lattice_points(*lattice)
        inside = ((p >= 0) & (p <= 1)).all(1)
        got = tz.restated_out(name, lattice)
        assert got.shape == tuple(lattice[0]) and got.dtype == np.float32
        sampled = qr.sample(s, v, p[inside])
        assert (sampled["status"] == qr.HIT).all()
        assert np.array_equal(got.reshape(-1)[inside].view(np.uint32), sampled["distance"].astype(f32).view(np.uint32)), (name, lattice)
        half = tz.restated_out(name, lattice, np.float16)
        assert half.dtype == np.float16 and np.array_equal(half.astype(f32), got.astype(np.float16).astype(f32)), (name, lattice)


@pytest.mark.parametrize("name", ["chain14", "dfs_d6_a", "blocks_257"])
def test_out_rises_at_slope_one_along_a_line_leaving_the_cube(name):
    """Along an axis from a point of a face, in dyadic steps: the clamped point stays, e is the step count times 1/4 exactly, its
    square and the root are exact, so the element is the float sum of the face's value and the distance -- one rounding, bit for bit"""
    src = tz.zoo()[name]
    for a in range(3):
        for side in (0, 1):
            shape, origin = [1, 1, 1], [0.3, 0.7, 0.45]
            shape[2 - a] = 9                                        # (shape is (nz, ny, nx))
            origin[a] = 1.0 if side else -2.0
            got = vr.volume_out(src, tuple(shape), tuple(origin), 0.25).reshape(-1)
            on_face = got[0] if side else got[8]
            steps = np.arange(9, dtype=f32) if side else np.arange(8, -1, -1, dtype=f32)
            assert np.array_equal(got.view(np.uint32), (on_face + steps * f32(0.25)).view(np.uint32)), (name, a, side)
            assert (np.diff(got) > 0).all() if side else (np.diff(got) < 0).all()


# ---- what the cases are for ------------------------------------------------------------------------------------------------------
def test_the_cases_are_what_they_are_for():
    z = tz.zoo()
    # the compositions' sizes, pinned; three ops in one list; one source in four instances; the 14-deep chain
    for name, nodes in tz.COMPOSE_NODES.items():
        for depth, n in zip(tz.COMPOSE_DEPTHS, nodes):
            S, V, counts = tz.restated_compose(name, depth)
            assert len(S) == n <= tz.NODE_CAP and counts["depth_out"] == depth == er.tree_depth(S), (name, depth)
            assert counts["samples"] == len(tz.COMPOSE_LISTS[name]) * (9 + 35 * ((len(S) - 1) // 8)), (name, depth)
    assert set(tz.COMPOSE_NODES) == set(tz.COMPOSE_LISTS)
    assert [op for _, _, op in tz.COMPOSE_LISTS["csg"]] == [0, 2, 1] and {src for src, _, _ in tz.COMPOSE_LISTS["csg"]} == {"dfs_d6_a", "blocks_4097", "chain12"}
    assert {src for src, _, _ in tz.COMPOSE_LISTS["repeated"]} == {"blocks_65"} and len({pl for _, pl, _ in tz.COMPOSE_LISTS["repeated"]}) == 4
    assert "chain14" in {src for src, _, _ in tz.COMPOSE_LISTS["chain14"]}
    # keeps: at least 20 000 nodes, more than the arrays start with (1.5 times the distinct sources together) and at most twice that:
    # they grow once
    start = sum(len(z[src][0]) for src in {src for src, _, _ in tz.COMPOSE_LISTS["keeps"]}) * 3 // 2
    assert start >= 4096 and max(20_000, start) < len(tz.restated_compose("keeps", 5)[0]) <= 2 * start
    # each later instance changes the csg tree
    full = tz.restated_compose("csg", 4)
    parts = [(z[src], pl, op) for src, pl, op in tz.compose_parts("csg")]
    for drop in (1, 2):
        other = cpr.compose([p for k, p in enumerate(parts) if k != drop], 4)
        assert not (len(other[0]) == len(full[0]) and np.array_equal(other[1], full[1])), drop
    # the lattices: one sticks out on every side, one lies inside the chains' deepest cells, and the long one makes k_volume_out's
    # loop (2^16 workgroups of 256 threads) take a second trip, with element 2^24 inside slab 254
    lattices = tz.out_lattices()
    assert len(lattices) == 4 and lattices[0][0] == (9, 9, 9) and lattices[3] == tz.DEEP_CORNER
    p = vr.lattice_points(*lattices[1])
    outside = ~((p >= 0) & (p <= 1)).all(1)
    assert outside.any() and not outside.all()
    assert vr.lattice_points(*tz.DEEP_CORNER).max() == 2.0 ** -9
    for chain in ("chain12", "chain14"):                            # the lattice's steps are cells of the chain's level 12
        deep = tz.restated_out(chain, tz.DEEP_CORNER)
        assert len(np.unique(deep)) > 300, chain
    (nz, ny, nx), origin, spacing = tz.LONG_OUT
    assert nx * ny * nz == 16_974_593 > 2 ** 24 and 254 * ny * nx < 2 ** 24 < 255 * ny * nx
    assert tz.slabs(254) == ((3, 257, 257), (0.0, 0.0, 254 / 256), 1 / 256)
    for k0 in (0, 254):                                             # exact positions: the slabs of the long lattice ARE this lattice
        z_of = f32(origin[2]) + np.arange(k0, k0 + 3).astype(f32) * f32(spacing)
        assert np.array_equal(z_of, np.unique(vr.lattice_points(*tz.slabs(k0))[:, 2]))
        assert tz.restated_out(tz.LONG_OUT_SOURCE, tz.slabs(k0)).shape == (3, 257, 257)
    # a half read in the deepest cells holds subnormals
    bits = tz.restated_out("chain12", tz.DEEP_CORNER, np.float16).view(np.uint16)
    assert ((bits & 0x7C00 == 0) & (bits & 0x03FF != 0)).sum() >= 20

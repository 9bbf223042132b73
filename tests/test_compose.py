"""Composition (sdfhip_scene_compose) without a GPU: the CPU restatement (tests/compose_restatement.py) is held to things it did
not come from -- the placement's own restatement, the monotone byte, what the fold's order must and must not change, the closed form
and the measured volume of two spheres -- the array helpers to their definitions, the entry point refuses what it must refuse before
it touches a device, and the Python mirror's records are the header's.  tests/test_gpu_compose.py holds the GPU to the restatement
byte for byte."""
import ctypes
import os
import re

import numpy as np
import pytest

import compose_cases as cc
import compose_restatement as cr
import measure_restatement as mr
import place_restatement as plr
from conftest import REPO
from test_combine import assert_breadth_first
from test_gpu_combine import tree

U, I, S = cr.COMBINE_UNION, cr.COMBINE_INTERSECT, cr.COMBINE_SUBTRACT


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", cc.ONE)
def test_one_instance_is_the_placement(name):
    # the restated placement, byte for byte, counts included, at the sources' own depth, at the root alone and two levels further
    (src, pl, _), = cc.case(name)[0]
    got = cc.restated(name)
    want = plr.place(tree(src), *pl, -1, want_counts=True)
    assert same(got, want) and got[2] == want[2], name
    for depth in (0, 2, 6):
        got = cr.compose([(tree(src), pl)], depth, want_counts=True)
        want = plr.place(tree(src), *pl, depth, want_counts=True)
        assert same(got, want) and got[2] == want[2], (name, depth)


def test_the_roots_bytes_are_the_minimum_of_the_placements_roots():
    # FromFloat is monotone (floor of a saturated affine map with a positive slope: v <= w implies byte(v) <= byte(w)), so the byte of
    # fminf(u_0, u_1) is the smaller of the two bytes EXACTLY, and the root's eight corners are evaluated at the same points in all
    # three trees
    a, b = tree("sphere_d4"), tree("nine")
    ident = (plr.IDENTITY, 1.0, (0.0, 0.0, 0.0))
    both = cr.compose([(a, ident), (b, ident)], 0)
    pa, pb = plr.place(a, *ident, 0), plr.place(b, *ident, 0)
    assert len(both[0]) == 1 and np.array_equal(both[1][0], np.minimum(pa[1][0], pb[1][0]))
    assert (pa[1][0] < pb[1][0]).any() and (pb[1][0] < pa[1][0]).any(), "each source wins at some corner"
    # ... and under an intersection the larger, under a difference the larger of a's and the byte of -u_b
    meet = cr.compose([(a, ident), (b, ident, I)], 0)
    assert np.array_equal(meet[1][0], np.maximum(pa[1][0], pb[1][0]))


def test_the_order_of_a_union_changes_no_byte():
    parts, depth = cc.case("eight")
    want = cc.restated("eight")
    rng = np.random.default_rng(11)
    for _ in range(2):
        order = rng.permutation(len(parts))
        assert not np.array_equal(order, np.arange(len(parts)))
        got = cr.compose(cc.with_trees([parts[k] for k in order]), depth, want_counts=True)
        assert same(got, want) and got[2] == want[2]


def test_the_order_of_a_difference_and_of_a_mixed_list_matters():
    a, b = tree("sphere_d4"), tree("sphere_d4")
    left = plr.as_placement(plr.IDENTITY, 0.6, (0.1, 0.2, 0.2))            # the sphere's centre lands at (0.4, 0.5, 0.5)
    right = plr.as_placement(plr.IDENTITY, 0.6, (0.3, 0.2, 0.2))           # ... and at (0.6, 0.5, 0.5)
    only_left, only_right, in_both, in_neither = (0.25, 0.5, 0.5), (0.75, 0.5, 0.5), (0.5, 0.5, 0.5), (0.5, 0.9, 0.9)
    p = np.array([only_left, only_right, in_both, in_neither], dtype=np.float32)
    ua, ub = plr.value(a, p, *left), plr.value(b, p, *right)
    assert (ua < 0).tolist() == [True, False, True, False] and (ub < 0).tolist() == [False, True, True, False]
    inst = lambda *parts: cr.as_instances(parts)
    # A - B is A's part outside B, B - A the other: they disagree exactly where one operand is solid alone
    a_b = cr.value(inst((a, left), (b, right, S)), p)
    b_a = cr.value(inst((b, right), (a, left, S)), p)
    assert (a_b < 0).tolist() == [True, False, False, False] and (b_a < 0).tolist() == [False, True, False, False]
    assert not same(cr.compose([(a, left), (b, right, S)], 4), cr.compose([(b, right), (a, left, S)], 4))
    # an intersection is symmetric: fmaxf(u_0, u_1) = fmaxf(u_1, u_0), the same tree
    assert same(cr.compose([(a, left), (b, right, I)], 4), cr.compose([(b, right), (a, left, I)], 4))
    assert (cr.value(inst((a, left), (b, right, I)), p) < 0).tolist() == [False, False, True, False]
    # (A u B) - C against (A - C) u B with C = B: the first is A - B, the second has B back
    first = cr.value(inst((a, left), (b, right, U), (b, right, S)), p)
    second = cr.value(inst((a, left), (b, right, S), (b, right, U)), p)
    assert (first < 0).tolist() == [True, False, False, False] and (second < 0).tolist() == [True, True, True, False]
    # an op the rule does not know, and a first instance that is no union
    with pytest.raises(ValueError):
        cr.compose([(a, left), (b, right, 3)], 2)
    with pytest.raises(ValueError):
        cr.compose([(a, left, S)], 2)


def test_an_instance_far_outside_leaves_the_union_unchanged():
    # nothing is special-cased: the far sphere has a value everywhere -- its field continued at slope 1 from its cube three units away,
    # above 1.9 at the corners and the centre of the result's cube -- and fminf takes it wherever it is the smaller one.  At the points
    # this tree evaluates it never is: the tree is the torus's placement alone (test_gpu_place.BIG's), twice the look-ups
    from test_gpu_place import BIG, restated as placed
    parts, depth = cc.case("far")
    assert (parts[0][0], depth) == (BIG[0], 7) and np.array_equal(parts[0][1][0], _placement_of_big()[0])
    S_, V_, counts = cc.restated("far")
    PS, PV, pcounts = placed(*BIG)
    assert np.array_equal(S_, PS) and np.array_equal(V_, PV) and len(S_) > 100_000
    assert counts["samples"] == 2 * pcounts["samples"] and counts["depth_out"] == pcounts["depth_out"] == 7
    # what the far instance is at the corners and the centre of the cube
    corners = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)] + [[0.5, 0.5, 0.5]], dtype=np.float32)
    assert (plr.value(tree(parts[1][0]), corners, *parts[1][1]) > 1.9).all()


def _placement_of_big():
    from test_gpu_place import BIG, PLACEMENTS
    return PLACEMENTS[BIG[1]]()


# ---- two disjoint spheres: the closed form and the volume ---------------------------------------------------------------------------
DEPTH = 6
H = 2.0 ** -DEPTH                                   # the sources' leaf edge; both are placed at scale 1
QUANTUM = 2.0 * H / 255.0                           # one step of a byte of that level: the byte maps [-0.5 H, 1.5 H] onto 0..255
SPHERES = [((0.3, 0.3, 0.3), 0.17), ((0.68, 0.7, 0.66), 0.2)]


@pytest.fixture(scope="module")
def two_spheres(sb):
    """[(source arrays, (R, s, t), centre of the placed sphere in double, radius)]: each sphere generated to depth 6 where it is, the
    first left there, the second turned about its own centre (the closed form does not see that, the look-ups do) and moved"""
    out = []
    for k, (c, r) in enumerate(SPHERES):
        od = sb.OctData.Generate(sb._lib.SHAPE_SPHERE, [*c, r], DEPTH)
        if k == 0:
            pl, centre = plr.as_placement(plr.IDENTITY, 1.0, (0.0, 0.0, 0.0)), np.array(c, dtype=np.float64)
        else:
            to = (0.7, 0.66, 0.7)
            pl, centre = plr.as_placement(*sb.placement(25, -40, 15, 1.0, about=c, to=to)), np.array(to, dtype=np.float64)
        out.append(((od.Structs, od.Values), pl, centre, r))
    return out


def closed_form(two, p):
    p = np.asarray(p, dtype=np.float64)
    return np.minimum(*[np.sqrt(((p - c) ** 2).sum(1)) - r for _, _, c, r in two])


def test_two_disjoint_spheres_against_the_closed_form(two_spheres):
    """The folded value against min(|p - c1| - r1, |p - c2| - r2) at points of each sphere's band.  The tolerance, derived:
      * a source byte is floor(...): decoded, it is the generator's float distance at the corner less at most one QUANTUM, provided
        it is not saturated.  A point is kept only if the eight corners of its leaf (the source's cell of edge H that contains the
        source point) all have closed-form distances inside [-0.5 H + QUANTUM, 1.5 H - QUANTUM]: then no byte is saturated, the
        centre of every ancestor is within 2 of its own edge of the surface (1.5 H + sqrt(3) / 2 E < 2 E for E >= 2 H) so the leaf
        exists, and the interpolated bytes are the interpolated distances less at most one QUANTUM
      * trilinear interpolation of f = |x - c| over a cell of edge H errs by at most H^2 / 8 times the sum of the largest second
        derivatives along the axes, each at most 1 / rho where rho >= r - 2 H is the distance to the centre: 3 H^2 / (8 (r - 2 H))
      * fp32: the inverse map and the distance are a handful of operations on numbers below 2, 16 ulps of 2 = 4e-6 is generous
    and the other sphere, more than 8 leaves away, has a value above 1.5 H there in both the closed form and the samples (asserted),
    so the minimum takes the near one in both."""
    rng = np.random.default_rng(3)
    instances = cr.as_instances([(src, pl) for src, pl, _, _ in two_spheres])
    kept = 0
    for k, (src, (R, s, t), centre, r) in enumerate(two_spheres):
        u = rng.normal(size=(4000, 3))
        u /= np.sqrt((u * u).sum(1))[:, None]
        p = (centre + u * (r + rng.uniform(0.0, H, size=(4000, 1)))).astype(np.float32)
        # the leaf of each point in the source's coordinates, and the closed form at its corners (in double)
        q = np.stack(plr.inverse_map(p, R, s, t), 1).astype(np.float64)
        base = np.floor(q / H)
        c_src = np.array(SPHERES[k][0], dtype=np.float64)
        corners = (base[:, None, :] + cr.CORNER[None].astype(np.float64)) * H
        f = np.sqrt(((corners - c_src) ** 2).sum(2)) - r
        ok = ((f >= -0.5 * H + QUANTUM) & (f <= 1.5 * H - QUANTUM)).all(1)
        assert ok.sum() > 300, ok.sum()
        p = p[ok]
        kept += len(p)
        want = closed_form(two_spheres, p)
        other = two_spheres[1 - k]
        far = np.sqrt(((p.astype(np.float64) - other[2]) ** 2).sum(1)) - other[3]
        assert (far > 8 * H).all() and (plr.value(other[0], p, *other[1]) >= 1.5 * H).all()
        tol = QUANTUM + 3.0 * H * H / (8.0 * (r - 2.0 * H)) + 4e-6
        got = cr.value(instances, p).astype(np.float64)
        err = np.abs(got - want)
        print(f"sphere {k}: {len(p)} points, max |folded - closed form| = {err.max():.3e}, tolerance {tol:.3e} (quantum {QUANTUM:.3e})")
        assert err.max() <= tol, (k, err.max(), tol)
    assert kept > 1000


def test_the_volume_of_two_disjoint_spheres_is_the_sum(two_spheres):
    """measure_restatement's volume of the composition against the sum of the two placements' volumes.  The tolerance, derived: fminf
    returns one of its operands, so a corner's byte in the composition is the byte of one of the two floats the placements round;
    where it is the other sphere's, that value is positive in both trees (the test above: the far sphere's value is at least 1.5 H
    wherever the near one's band lies, and the far sphere's own field is positive outside it), so a sign -- and with it the
    surface -- can move only by what one byte resolves: one QUANTUM along the normal.  Each surface moved by one QUANTUM changes the
    volume by at most its area times QUANTUM; the areas are the spheres'."""
    parts = [(src, pl) for src, pl, _, _ in two_spheres]
    composed = mr.measure(*cr.compose(parts, DEPTH)).volume
    alone = [mr.measure(*plr.place(src, *pl, DEPTH)).volume for src, pl in parts]
    area = sum(4.0 * np.pi * r * r for _, _, _, r in two_spheres)
    tol = area * QUANTUM
    exact = sum(4.0 / 3.0 * np.pi * r ** 3 for _, _, _, r in two_spheres)
    print(f"volume composed {composed:.9f}, placed {alone[0]:.9f} + {alone[1]:.9f} = {sum(alone):.9f} (the spheres' own: {exact:.9f}), "
          f"tolerance {tol:.3e}")
    assert alone[0] > 0.5 * 4.0 / 3.0 * np.pi * 0.17 ** 3 and alone[1] > 0.5 * 4.0 / 3.0 * np.pi * 0.2 ** 3
    assert abs(composed - sum(alone)) <= tol, (composed, alone, tol)


# ---- structure ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["eight", "csg", "many", "depth0", "deepest"])
def test_structure(sb, name):
    S_, V_, counts = cc.restated(name)
    parts, depth = cc.case(name)
    assert assert_breadth_first(sb, S_, V_) == counts["depth_out"] == counts["levels"] - 1
    assert counts["samples"] == len(parts) * (9 + 35 * ((len(S_) - 1) // 8))
    if name == "depth0":
        assert len(S_) == 1 and tuple(S_[0]) == (-1, -1), "the root alone"
    else:
        assert len(S_) > 1000 and counts["depth_out"] == (6 if depth < 0 else depth)


# ---- depth 12 in the far corner, and the instance limit -------------------------------------------------------------------------------
def test_the_far_corner_is_12_levels_deep_with_coordinates_above_2_to_the_10():
    import volume_cases as vc
    S_, V_, counts = cc.restated("corner_d12")
    parts, depth = cc.case("corner_d12")
    assert depth == 12 and len(parts) == 2 and {src for src, _, _ in parts} == {"sphere_d4"}
    assert all(float(pl[1]) == 2.0 ** -7 for _, pl, _ in parts) and np.array_equal(parts[1][1][0], plr.IDENTITY)
    assert counts["depth_out"] == 12 and len(S_) == cc.CORNER_D12_NODES == 63233 <= 400_000
    sizes = vc.level_sizes(S_)
    assert len(sizes) == 13 and sizes[12] == 48120 > 32768, "the last level is past one chunk of the shared scan"
    blocks = vc.last_blocks(S_)
    assert (blocks > 2 ** 10).all(1).any() and blocks.max() < 2 ** 11
    # the second instance sits on the face y = 1 where x and z are small: a packed word with a large y beside a small x
    assert ((blocks[:, 1] > 2 ** 10) & (blocks[:, 0] < 2 ** 5) & (blocks[:, 2] < 2 ** 5)).any()
    # one instance: the placement's restatement, array for array, in the same corner
    one, want = cc.restated("corner_d12_one"), plr.place(tree("sphere_d4"), *parts[0][1], 12, want_counts=True)
    assert same(one, want) and one[2] == want[2] and len(one[0]) == cc.CORNER_D12_ONE_NODES == 33577
    assert (vc.last_blocks(one[0]) > 2 ** 10).all(1).any()


def test_the_fold_over_distinct_pairs_is_the_restatement_on_the_first_130():
    # the 4096-long list is restated by evaluating its 16 distinct (source, placement) pairs once and folding in list order: held
    # here to compose_restatement.compose itself, instance by instance, on the list's first 130 entries -- past two waves of 64
    parts, depth = cc.case("limit_130")
    assert [(src, op) for src, _, op in parts] == [(src, op) for src, _, op in cc.case(f"limit_{cc.LIMIT}")[0][:130]]
    want = cr.compose(cc.with_trees(parts), depth, want_counts=True)
    got = cc.restated("limit_130")
    assert same(got, want) and got[2] == want[2] and len(got[0]) == cc.LIMIT_NODES[130]
    # ... and point by point on scattered points, all three ops among the 130
    p = np.random.default_rng(5).random((500, 3)).astype(np.float32)
    inst = cr.as_instances(cc.with_trees(parts))
    assert {op for _, _, op in inst} == {U, I, S}
    assert np.array_equal(cc.folded_value(inst, p).view(np.uint32), cr.value(inst, p).view(np.uint32))


def test_the_long_lists_are_what_they_are_for():
    full, depth = cc.case(f"limit_{cc.LIMIT}")
    assert len(full) == 4096 and depth in (3, 4) and full[0][2] == U
    pairs = cc.limit_pairs()
    assert len(pairs) == 16 and {src for src, _ in pairs} == {"leaf", "nine", "blocks_65"}
    assert len({(src, pl[0].tobytes(), pl[1].tobytes(), pl[2].tobytes()) for src, pl in pairs}) == 16
    assert all(full[k][0] == pairs[k % 16][0] and np.array_equal(full[k][1][2], pairs[k % 16][1][2]) for k in range(4096))
    # the ops vary with k: no pair meets the same op every time, and the list is not periodic in 16
    ops = np.array([op for _, _, op in full])
    assert {int(o) for o in ops} == {U, I, S} and not np.array_equal(ops[16:32], ops[32:48])
    assert all(len(set(ops[j::16].tolist())) >= 2 for j in range(16))
    for n in (63, 64, cc.LIMIT):
        assert len(cc.case(f"limit_{n}")[0]) == n
        S_, V_, counts = cc.restated(f"limit_{n}")
        assert len(S_) == cc.LIMIT_NODES[n] and counts["depth_out"] == depth, n
        assert counts["samples"] == n * (9 + 35 * ((len(S_) - 1) // 8)), n
    # later repeats still change the tree: without its last 16 entries, and without its second half, the list gives another tree
    whole = cc.restated(f"limit_{cc.LIMIT}")
    for n in (4080, 2048):
        part = cc.restated(f"limit_{n}")
        assert not (len(part[0]) == len(whole[0]) and np.array_equal(part[1], whole[1])), n


# ---- the array helpers --------------------------------------------------------------------------------------------------------------
def test_linear_array(sb):
    base = sb.placement(30, 20, -70, 0.37, about=(0.2, 0.6, 0.5), to=(0.2, 0.3, 0.4))
    step = (0.1, -0.03, 0.007)
    row = sb.linear_array(base, step, 5)
    assert len(row) == 5
    for i, (R, s, t) in enumerate(row):
        assert R.dtype == np.float32 and t.dtype == np.float32 and isinstance(s, np.float32)
        assert np.array_equal(R, base[0]) and s == base[1]
        # computed in double, rounded once
        assert np.array_equal(t, (base[2].astype(np.float64) + i * np.array(step)).astype(np.float32)), i
    assert np.array_equal(row[0][2], base[2]), "copy 0 is the input"
    mirror = (np.diag([-1.0, 1.0, 1.0]).astype(np.float32), 0.75, (0.95, 0.1, 0.2))
    assert all(np.linalg.det(R.astype(np.float64)) < 0 for R, _, _ in sb.linear_array(mirror, step, 3))
    with pytest.raises(ValueError):
        sb.linear_array(base, step, 0)


def test_circular_array(sb):
    base = sb.placement(30, 20, -70, 0.37, about=(0.2, 0.6, 0.5), to=(0.8, 0.5, 0.4))
    centre, axis = (0.5, 0.5, 0.5), np.array([1.0, 2.0, -0.5]) / np.sqrt(5.25)
    count = 7
    ring = sb.circular_array(base, centre, axis, count)
    assert len(ring) == count
    R0, s0, t0 = ring[0]
    assert np.array_equal(R0, base[0]) and s0 == base[1] and np.array_equal(t0, base[2]), "copy 0 is the input"
    x = np.array([0.3, 0.9, 0.1])
    c = np.array(centre)
    where = [float(s) * R.astype(np.float64) @ x + t.astype(np.float64) for R, s, t in ring]
    for i, (R, s, t) in enumerate(ring):
        assert R.dtype == np.float32 and t.dtype == np.float32 and isinstance(s, np.float32) and s == base[1]
        assert np.abs(R.astype(np.float64) @ R.astype(np.float64).T - np.eye(3)).max() < 1e-6
        assert abs(np.linalg.det(R.astype(np.float64)) - 1) < 1e-6
        # a point of the source keeps its distance from the axis' line and its height along it, and turns by 360 / count a copy
        rel = where[i] - c
        assert abs(rel @ axis - (where[0] - c) @ axis) < 1e-6
        assert abs(np.linalg.norm(rel - (rel @ axis) * axis) - np.linalg.norm((where[0] - c) - ((where[0] - c) @ axis) * axis)) < 1e-6
    radial = [w - c - ((w - c) @ axis) * axis for w in where]
    for i in range(count):
        a, b = radial[i], radial[(i + 1) % count]
        angle = np.arctan2(np.cross(a, b) @ axis, a @ b)                 # right-handed about the axis
        assert abs(angle - 2 * np.pi / count) < 1e-5, (i, angle)
    # copy `count` would be copy 0 again: in double, the turn by 360 * count / count degrees is the identity to rounding
    from sdfbox_amd.renderer import _axis_rotation
    Q = _axis_rotation(axis / np.linalg.norm(axis), 2.0 * np.pi * count / count)
    assert np.abs(Q - np.eye(3)).max() < 1e-15
    full = sb.circular_array(base, centre, axis, 1)[0]
    assert np.array_equal(full[0], base[0]) and np.array_equal(full[2], base[2])
    # a quarter turn about z through the origin: x -> y
    quarter = sb.circular_array((np.eye(3), 1.0, (1.0, 0.0, 0.0)), (0, 0, 0), (0, 0, 1), 4)[1]
    assert np.allclose(quarter[0], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-7) and np.allclose(quarter[2], (0, 1, 0), atol=1e-7)
    # the mirror's sign is preserved
    mirror = (np.diag([-1.0, 1.0, 1.0]).astype(np.float32), 0.75, (0.95, 0.1, 0.2))
    assert all(np.linalg.det(R.astype(np.float64)) < -0.99 for R, _, _ in sb.circular_array(mirror, centre, axis, 5))
    for bad in ((0, 0, 0), (0, 0, 2), (float("nan"), 0, 1)):
        with pytest.raises(ValueError):
            sb.circular_array(base, centre, bad, 3)
    with pytest.raises(ValueError):
        sb.circular_array(base, centre, axis, 0)


# ---- the entry point and the binding ------------------------------------------------------------------------------------------------
def test_compose_raises_in_python_where_python_raises(sb):
    ident = (np.eye(3), 1.0, (0, 0, 0))
    with pytest.raises(ValueError, match="no parts"):
        sb.Scene.Compose([])
    with pytest.raises(ValueError, match="part 0"):
        sb.Scene.Compose([(None, ident)])                       # not a Scene
    with pytest.raises(ValueError, match="part 0"):
        sb.Scene.Compose(["scene"])
    scene = sb.Scene.__new__(sb.Scene)                          # a Scene object that holds no handle: enough for the checks before the call
    scene._h, scene.device = ctypes.c_void_p(), 0
    with pytest.raises(ValueError, match="part 1"):
        sb.Scene.Compose([(scene, ident), (scene, (np.eye(3), 1.0))])
    with pytest.raises(ValueError, match="part 0"):
        sb.Scene.Compose([(scene, ident, 0, "more")])
    with pytest.raises(ValueError):
        sb.Scene.Compose([(scene, (np.eye(2), 1.0, (0, 0, 0)))])
    # what Python lets through the library refuses: the handle is null
    with pytest.raises(sb.SdfHipError) as e:
        sb.Scene.Compose([(scene, ident)])
    assert e.value.code == sb._lib.ERR_ARG and "instance 0: null scene" in str(e.value)


def test_compose_refuses_bad_arguments_without_a_gpu(sb):
    L = sb._lib

    def call(items, n=None, opt=None, want_out=True, data=None):
        arr = (sb.Instance * max(1, len(items)))(*items) if items is not None else None
        out = ctypes.c_void_p(1)
        rc = L.lib.sdfhip_scene_compose(arr, len(items) if n is None else n, ctypes.byref(opt) if opt is not None else None,
                                        ctypes.byref(out) if want_out else None, ctypes.byref(data) if data is not None else None, None)
        assert not want_out or out.value is None, "*out is not null after a failure"
        return rc, L.lib.sdfhip_last_error()

    good = lambda **kw: sb.Instance(**kw)
    rc, msg = call(None, n=1)
    assert rc == L.ERR_ARG and b"null instance list" in msg
    for n in (0, 4097, 0xFFFFFFFF):
        rc, msg = call([good()], n=n)
        assert rc == L.ERR_ARG and b"1..4096" in msg, n
    rc, msg = call([good()], want_out=False)
    assert rc == L.ERR_ARG and b"both outputs" in msg
    rc, msg = call([good()])                                     # a valid record reaches the handle check; NULL options are the defaults
    assert rc == L.ERR_ARG and b"instance 0: null scene" in msg
    rc, msg = call([good()], want_out=False, data=L.COctData())  # host_out alone is an output
    assert rc == L.ERR_ARG and b"null scene" in msg
    rc, msg = call([good()] * 4096)
    assert rc == L.ERR_ARG and b"instance 0: null scene" in msg
    for size in (4, 9, 4100):
        opt = sb.ComposeOptions()
        opt.size = size
        rc, msg = call([good()], opt=opt)
        assert rc == L.ERR_ARG and b"bytes" in msg, size
    for depth in (-2, 13, 100):
        rc, msg = call([good()], opt=sb.ComposeOptions(depth))
        assert rc == L.ERR_ARG and b"depth" in msg, depth
    for depth in (None, 0, 12):
        rc, msg = call([good()], opt=sb.ComposeOptions(depth))
        assert rc == L.ERR_ARG and b"null scene" in msg, depth
    # per instance, and the message names which (here always the first: without a GPU there is no handle that would let a list get
    # past instance 0; tests/test_gpu_compose.py has them further down the list): the first op, an unknown op, the placement's checks
    for op in (1, 2):
        rc, msg = call([good(op=op)])
        assert rc == L.ERR_ARG and b"instance 0" in msg and b"UNION" in msg, op
    for op in (-1, 3):
        rc, msg = call([good(op=op), good()])
        assert rc == L.ERR_ARG and b"instance 0: unknown op" in msg, op
    for bad in (float("nan"), float("inf"), -float("inf")):
        for item in (good(scale=bad), good(translation=(0, bad, 0)), good(rotation=((1, 0, 0), (0, 1, 0), (0, bad, 1)))):
            rc, msg = call([item, good()])
            assert rc == L.ERR_ARG and b"instance 0" in msg and b"finite" in msg, bad
    for scale in (0.0, -0.0, -1.0):
        rc, msg = call([good(scale=scale)])
        assert rc == L.ERR_ARG and b"instance 0" in msg and b"scale" in msg, scale
    for rotation in (((1, 0, 0), (0, 1, 0), (0, 0, 1.001)), ((1, 2e-4, 0), (0, 1, 0), (0, 0, 1)), ((0, 0, 0), (0, 0, 0), (0, 0, 0))):
        rc, msg = call([good(rotation=rotation)])
        assert rc == L.ERR_ARG and b"instance 0" in msg and b"orthogonal" in msg, rotation
    for rotation in (sb.placement(30, 20, -70)[0], ((1, 5e-5, 0), (0, 1, 0), (0, 0, 1)), ((-1, 0, 0), (0, 1, 0), (0, 0, 1))):
        rc, msg = call([good(rotation=np.asarray(rotation).tolist(), op=0)])
        assert rc == L.ERR_ARG and b"null scene" in msg, rotation


def test_records_match_the_header(sb):
    text = open(os.path.join(REPO, "include", "sdfhip.h")).read()
    record = lambda name: re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    fields = lambda body: [re.sub(r"\[.*", "", f.strip().lstrip("*")) for decl in re.findall(r"(?:sdfhip_scene|uint32_t|int32_t|uint64_t|float)\s+([^;]+);", body)
                           for f in decl.split(",")]
    assert fields(record("sdfhip_instance")) == [f for f, _ in sb.Instance._fields_]
    assert fields(record("sdfhip_compose_options")) == [f for f, _ in sb.ComposeOptions._fields_]
    assert fields(record("sdfhip_compose_stats")) == [f for f, _ in sb.ComposeStats._fields_]
    N, T = sb.Instance, sb.ComposeStats
    assert ctypes.sizeof(N) == 64 and (N.scene.offset, N.op.offset, N.rotation.offset, N.scale.offset, N.translation.offset) == (0, 8, 12, 48, 52)
    assert ctypes.sizeof(T) == 40 and (T.instances.offset, T.samples.offset, T.kernel_ms.offset, T.total_ms.offset) == (12, 16, 24, 32)
    opt = sb.ComposeOptions()
    assert (ctypes.sizeof(opt), opt.size, opt.depth) == (8, 8, -1) and sb.ComposeOptions(5).depth == 5
    item = sb.Instance()
    assert (item.scene, item.op, item.scale) == (None, 0, 1.0) and [list(r) for r in item.rotation] == np.eye(3).tolist()
    assert "sdfhip_scene_compose" in sb._lib.EXPORTED_SYMBOLS and isinstance(sb.Scene.__dict__["Compose"], staticmethod)
    # the C++ mirror and the C# stub name the entry point too
    assert "sdfhip_scene_compose(" in open(os.path.join(REPO, "include", "sdfbox.hpp")).read()
    assert "sdfhip_scene_compose(" in open(os.path.join(REPO, "INTEGRATION.md")).read()

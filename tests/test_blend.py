"""Smooth blends and morphs (sdfhip_scene_blend) without a GPU: the brute-force restatement (tests/blend_restatement.py) is held to
things it does not restate -- the offset's bytes where the rule says the two agree, the closed form of the bridge between two solids
a gap apart, the bounds of a smooth minimum, volumes through the measure's restatement -- and a NaN is shown never to reach a byte.
tests/test_gpu_blend.py holds the GPU to the restatement byte for byte."""
import math
import os
import warnings

import numpy as np
import pytest

import blend_restatement as br
import distance_restatement as dr
import measure_restatement as msr
import query_restatement as qr
import tree_zoo
from conftest import REPO

f32 = np.float32
U, I, SUB, M = br.UNION, br.INTERSECT, br.SUBTRACT, br.MORPH
EMPTY = (np.array([[-1, -1]], dtype=np.int32), np.full((1, 8), 255, dtype=np.uint8))       # all outside, no surface: dist = +inf
FULL = (np.array([[-1, -1]], dtype=np.int32), np.zeros((1, 8), dtype=np.uint8))            # all inside, no surface: dist = -inf
ULPS = 4 * 2.0 ** -24                                                                      # "a few ulps" of values below 1


def ball(r):
    return 4.0 / 3.0 * math.pi * r ** 3


@pytest.fixture(scope="module")
def sphere(sb):
    od = sb.OctData.LoadAsdf(os.path.join(REPO, "tests", "golden", "sphere_d4.asdf"))
    return od.Structs, od.Values


@pytest.fixture(scope="module")
def surf(sphere):
    return dr.Surface(*sphere)


def lattice(n=9, lo=0.0, hi=1.0):
    k = np.linspace(lo, hi, n)
    return np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3).astype(f32)


def generated_sphere(sb, centre, r, depth):
    od = sb.OctData.Generate(sb._lib.SHAPE_SPHERE, [*centre, r], depth)
    return od.Structs, od.Values


# ---- what follows from the rule: the offset's bytes --------------------------------------------------------------------------------
def test_a_morph_at_zero_is_the_offset_by_zero(sphere, surf):
    """t = 0: (b - a) * 0 is a zero and a + 0 is a, so the tree is Offset(A, 0)'s byte for byte -- with B a second surface that is
    not empty (the zoo's single leaf)."""
    leaf = tree_zoo.zoo()["leaf"]
    assert len(dr.Surface(*leaf)) > 0
    want = dr.offset(sphere, dr.GROW, 0.0, 3, surf=surf)
    got = br.blend(sphere, leaf, M, 0.0, 3, surf_a=surf)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and len(got[0]) > 9


@pytest.mark.parametrize("k", [0.0, 0.07])
def test_a_union_with_nothing_is_the_offset_by_zero(sphere, surf, k):
    """b = +inf: fabsf(a - b) = inf, h = 0, fminf(a, inf) = a -- for any k"""
    want = dr.offset(sphere, dr.GROW, 0.0, 3, surf=surf)
    got = br.blend(sphere, EMPTY, U, k, 3, surf_a=surf)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- two spheres a gap apart: the bridge ------------------------------------------------------------------------------------------
GAP, R2, DEPTH2 = 0.1, 0.15, 4
C_LEFT, C_RIGHT = (0.5 - R2 - GAP / 2, 0.5, 0.5), (0.5 + R2 + GAP / 2, 0.5, 0.5)
K_SMALL, K_LARGE = 0.05, 0.5                    # clearly below and clearly above 2 g = 0.2
MID = np.array([[0.5, 0.5, 0.5]], dtype=f32)


@pytest.fixture(scope="module")
def pair(sb):
    A, B = generated_sphere(sb, C_LEFT, R2, DEPTH2), generated_sphere(sb, C_RIGHT, R2, DEPTH2)
    return A, B, dr.Surface(*A), dr.Surface(*B)


def radius_error(surface, centre, r):
    """the largest |dist - (|p - c| - r)| at points of known analytic distance: along five directions, inside and outside, and at
    the midpoint of the pair"""
    dirs = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0.6, 0.64, 0.48], [-0.48, 0.6, -0.64]])
    radii = np.array([0.0, 0.5 * r, r + GAP / 2, r + GAP, 2 * r])
    p = np.concatenate([(np.array(centre) + dirs[:, None, :] * radii[None, :, None]).reshape(-1, 3), MID.astype(np.float64)]).astype(f32)
    true = np.linalg.norm(p.astype(np.float64) - np.array(centre), axis=1) - r
    return float(np.abs(dr.dist(surface, p) - true).max())


def test_two_solids_a_gap_apart_grow_a_bridge_iff_k_exceeds_twice_the_gap(pair):
    """At the midpoint a = b = g / 2 and the value is g / 2 - k / 4: positive for a k clearly below 2 g, negative for one clearly
    above -- with |g / 2 - k / 4| beyond what the spheres' own surfaces are off by at this depth, which is measured here."""
    A, B, sa, sb_ = pair
    err = max(radius_error(sa, C_LEFT, R2), radius_error(sb_, C_RIGHT, R2))
    want = {k: GAP / 2 - k / 4 for k in (K_SMALL, K_LARGE)}
    print(f"two spheres: radius error {err}, closed form at the midpoint {want}")
    assert all(abs(v) > err for v in want.values()), "the cases do not clear the spheres' own error"
    got = {k: float(br.value(sa, sb_, MID, U, k)[0]) for k in want}
    print("restated value at the midpoint:", got)
    assert got[K_SMALL] > 0 and got[K_LARGE] < 0
    assert all(abs(got[k] - want[k]) <= err + ULPS for k in want)


def test_the_bridge_makes_one_solid_larger_than_the_hard_union(pair):
    A, B, sa, sb_ = pair
    hard = br.blend(A, B, U, 0.0, DEPTH2, surf_a=sa, surf_b=sb_)
    soft = br.blend(A, B, U, K_LARGE, DEPTH2, surf_a=sa, surf_b=sb_)
    v_hard, v_soft = msr.measure(*hard).volume, msr.measure(*soft).volume
    print(f"hard union {len(hard[0])} nodes volume {v_hard}; k = {K_LARGE}: {len(soft[0])} nodes volume {v_soft}; two balls {2 * ball(R2)}")
    assert v_soft > v_hard > 0
    # one solid: every point of the segment between the two centres is inside with the bridge; the hard union is two solids, outside
    # at the midpoint
    seg = np.stack([np.linspace(C_LEFT[0], C_RIGHT[0], 33), np.full(33, 0.5), np.full(33, 0.5)], 1).astype(f32)
    assert (qr.sample(*soft, seg)["distance"] < 0).all()
    d = qr.sample(*hard, seg)["distance"]
    assert d[16] > 0 and d[0] < 0 and d[-1] < 0


def test_a_smooth_minimum_lies_between_the_minimum_and_a_quarter_of_k_below_it(pair):
    """value <= min(a, b) and value >= min(a, b) - k / 4 (h <= 1), to a few ulps; INTERSECT and SUBTRACT obey the mirror images"""
    A, B, sa, sb_ = pair
    p = lattice(9)
    a, b = dr.dist(sa, p), dr.dist(sb_, p)
    assert (np.abs(a - b) < K_SMALL).any() and (np.abs(a - b) > K_SMALL).any()        # inside the smaller blend's reach, and beyond it
    for k in (0.0, K_SMALL, K_LARGE):
        q = f32(k) * f32(0.25)
        v = br.value_of(a, b, U, k)
        lo = np.fmin(a, b)
        assert (v <= lo + ULPS).all() and (v >= lo - q - ULPS).all(), k
        assert k == 0 or (v < lo).any()
        v = br.value_of(a, b, I, k)
        hi = np.fmax(a, b)
        assert (v >= hi - ULPS).all() and (v <= hi + q + ULPS).all(), k
        v = br.value_of(a, b, SUB, k)
        hi = np.fmax(a, -b)
        assert (v >= hi - ULPS).all() and (v <= hi + q + ULPS).all(), k


def test_k_zero_takes_the_branch_and_is_the_hard_operation_on_exact_distances(pair):
    """k = 0: h = 0 without a division, and the value is fminf / fmaxf of the two distances bit for bit -- never a warning"""
    A, B, sa, sb_ = pair
    p = lattice(5)
    a, b = dr.dist(sa, p), dr.dist(sb_, p)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for op, want in ((U, np.fmin(a, b)), (I, np.fmax(a, b)), (SUB, np.fmax(a, -b))):
            got = br.value_of(a, b, op, 0.0)
            assert got.dtype == f32 and np.array_equal(got.view(np.uint32), (want + f32(0)).view(np.uint32)), op
        assert np.array_equal(br.smin(f32(0.25), f32(0.5), 0.0), f32(0.25))


def test_subtracting_a_solid_from_itself_leaves_nothing_away_from_the_surface(sphere, surf):
    """SUBTRACT(A, A, 0) = -fminf(-a, a) = fabsf(a) >= 0: no inside point, but for the sliver at the surface where a byte rounds
    down to 63"""
    S, V = br.blend(sphere, sphere, SUB, 0.0, 3, surf_a=surf, surf_b=surf)
    p = lattice(17)
    away = np.abs(dr.dist(surf, p)) > 2.0 ** -3
    assert away.sum() > 1000
    assert (qr.sample(S, V, p[away])["distance"] > 0).all()
    print("A - A:", len(S), "nodes, volume", msr.measure(S, V).volume, "of", msr.measure(*sphere).volume)
    assert msr.measure(S, V).volume < 0.1 * msr.measure(*sphere).volume


# ---- the morph --------------------------------------------------------------------------------------------------------------------
def test_the_morph_of_two_concentric_spheres_at_one_half(sb):
    """a = |p - c| - r1 and b = |p - c| - r2 up to each mesh's error: a + (b - a) / 2 is the sphere of radius (r1 + r2) / 2, which
    is also the smaller sphere grown by half the difference.  The margin is the larger of the two spheres' own measured shortfalls
    against their balls at this depth."""
    c, r1, r2, depth = (0.5, 0.5, 0.5), 0.2, 0.35, 4
    A, B = generated_sphere(sb, c, r1, depth), generated_sphere(sb, c, r2, depth)
    sa, sb_ = dr.Surface(*A), dr.Surface(*B)
    v1, v2 = msr.measure(*A).volume, msr.measure(*B).volume
    margin = max(ball(r1) - v1, ball(r2) - v2)
    mid = br.blend(A, B, M, 0.5, depth, surf_a=sa, surf_b=sb_)
    grown = dr.offset(A, dr.GROW, (r2 - r1) / 2, depth, surf=sa)
    vm, vg = msr.measure(*mid).volume, msr.measure(*grown).volume
    print(f"morph: operands {v1} {v2} (balls {ball(r1)} {ball(r2)}), margin {margin}; t = 0.5: {vm}; the smaller grown: {vg}; ball {ball((r1 + r2) / 2)}")
    assert margin > 0 and v1 < vm < v2
    assert abs(vm - vg) <= margin


# ---- empty operands ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [U, I, SUB])
def test_a_nan_never_reaches_a_byte(sphere, surf, op):
    """an empty A, an empty B and both empty (+inf and -inf alike): every value is a number, and the tree builds"""
    p = lattice(5, -0.25, 1.25)
    for k in (0.0, 0.1):
        for a_src, b_src in ((EMPTY, sphere), (sphere, EMPTY), (EMPTY, EMPTY), (FULL, sphere), (sphere, FULL), (FULL, FULL), (EMPTY, FULL), (FULL, EMPTY)):
            sa = surf if a_src is sphere else dr.Surface(*a_src)
            sb_ = surf if b_src is sphere else dr.Surface(*b_src)
            v = br.value(sa, sb_, p, op, k)
            assert not np.isnan(v).any(), (op, k)
            if a_src is not sphere and b_src is not sphere:
                assert np.isinf(v).all()
                S, V = br.blend(a_src, b_src, op, k, 3, surf_a=sa, surf_b=sb_)
                assert len(S) == 1 and ((V == 255).all() or (V == 0).all())
    S, V = br.blend(EMPTY, sphere, op, 0.1, 2, surf_b=surf)
    # nothing or B (the union), nothing (the intersection), nothing (nothing without B)
    assert len(S) == 1 and (V == 255).all() if op != U else len(S) > 1


def test_a_morph_of_an_empty_surface_is_refused(sphere, surf):
    for a_src, b_src in ((EMPTY, sphere), (sphere, EMPTY), (EMPTY, EMPTY)):
        with pytest.raises(ValueError):
            br.blend(a_src, b_src, M, 0.5, 2)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            br.blend(sphere, sphere, M, bad, 2, surf_a=surf, surf_b=surf)

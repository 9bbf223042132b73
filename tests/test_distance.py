"""Exact distance, offset and shell (sdfhip_scene_distance / sdfhip_scene_offset) without a GPU: the brute-force restatement
(tests/distance_restatement.py) is held to things it was not built from -- a plane's closed form, the radius of the golden sphere,
the volumes of grown, shrunk and hollowed balls -- and the gap the feature closes is stated as a test: where sdfhip_scene_sample's
distance is saturated, dist is not.  tests/test_gpu_distance.py holds the GPU's search to the restatement bit for bit."""
import math
import os

import numpy as np
import pytest

import distance_restatement as dr
import measure_restatement as msr
import query_restatement as qr
from conftest import REPO

f32 = np.float32
CENTRE, RADIUS = np.array([0.5, 0.5, 0.5]), 0.3         # tests/golden/sphere_d4.asdf
S4 = 1.0 / 16                                           # a depth-4 cell's edge


@pytest.fixture(scope="module")
def sphere(sb):
    od = sb.OctData.LoadAsdf(os.path.join(REPO, "tests", "golden", "sphere_d4.asdf"))
    S, V = od.Structs, od.Values
    S.setflags(write=False); V.setflags(write=False)
    return S, V


@pytest.fixture(scope="module")
def surf(sphere):
    return dr.Surface(*sphere)


_built = {}


def built(sphere, surf, mode, amount, depth):
    """(structs, values) of an offset or shell of the golden sphere, made once and left unchanged"""
    key = (mode, amount, depth)
    if key not in _built:
        _built[key] = dr.offset(sphere, mode, amount, depth, surf=surf)
    return _built[key]


def ball(r):
    return 4.0 / 3.0 * math.pi * max(r, 0.0) ** 3


# ---- the plane: a root-only tree whose bytes are 0 on the face x = 0 and 127 on the face x = 1 -----------------------------------
PLANE = (np.array([[-1, -1]], dtype=np.int32), np.array([[0, 127, 0, 127, 0, 127, 0, 127]], dtype=np.uint8))
X0 = 63.75 / 127                                        # where the bytes cross 63.75


def test_a_plane_is_exact():
    """Every cut vertex of the root has x = fl(63.75f / 127.0f): the surface is the plane x = x0 across the whole cube, so for a
    point of the cube dist = x - x0 up to the roundings of tri_dist2 (the difference p - q, three products, two sums, one root: a few
    ulps of values below 1)."""
    ps = dr.Surface(*PLANE)
    assert len(ps) == 8 and np.all(ps.pos[:, :, 0] == f32(63.75) / f32(127))
    rng = np.random.default_rng(5)
    p = rng.random((500, 3)).astype(f32)
    p = p[np.abs(p[:, 0] - X0) > 1e-4]                  # (next to the plane the sign is the sampled field's: the sliver of the rule)
    d = dr.dist(ps, p)
    err = np.abs(d.astype(np.float64) - (p[:, 0].astype(np.float64) - X0))
    print("plane: max |dist - (x - x0)| =", err.max())
    assert err.max() < 4 * 2.0 ** -24
    # and the nearest point is the foot of the perpendicular
    rec = dr.distance(*PLANE, p, surf=ps)
    assert np.abs(rec["nearest"][:, 0] - X0).max() < 2.0 ** -23 and np.abs(rec["nearest"][:, 1:] - p[:, 1:]).max() < 2.0 ** -22
    assert (rec["node"] == 0).all() and (rec["status"] == dr.HIT).all()


@pytest.mark.parametrize("delta", [0.1, -0.2])
def test_an_offset_plane_is_the_construct_rule_on_the_closed_form(delta):
    """offset(plane, delta) against the construct rule applied to x - x0 - delta in fp32: the same tree, and the same bytes except
    where floorf sits on a rounding boundary (the restated distance is sqrtf of a rounded square, the closed form a difference).
    Measured: delta 0.1 to depth 3, 585 nodes, no byte differs; delta -0.2, 457 nodes, no byte differs."""
    x0 = f32(63.75) / f32(127)
    got = dr.grow(PLANE, delta, 3)
    want = dr.construct(lambda p: (p[:, 0] - x0) - f32(delta), 3)
    assert np.array_equal(got[0], want[0]), "the same nodes split"
    diff = got[1].astype(np.int64) - want[1].astype(np.int64)
    where = np.argwhere(diff != 0)
    print(f"plane offset {delta}: {len(got[0])} nodes, bytes that differ (node, corner, got - want):",
          [(int(n), int(k), int(diff[n, k])) for n, k in where])
    assert np.abs(diff).max() <= 1 and len(where) <= len(got[0]) // 16
    assert len(got[0]) > 9 and (got[1] <= 63).any() and (got[1] > 63).any()


# ---- the golden sphere ------------------------------------------------------------------------------------------------------------
DIRS = np.array([[1, 0, 0], [0, 1, 0], [0.6, 0.64, 0.48], [-0.48, 0.6, -0.64], [-3 ** -0.5] * 3])
RADII = np.array([0.0, 0.05, 0.1, 0.2, 0.28, 0.32, 0.4, 0.5, 0.7, 0.85])


def ray_points():
    p = (CENTRE + DIRS[:, None, :] * RADII[None, :, None]).reshape(-1, 3).astype(f32)
    return p, np.linalg.norm(p.astype(np.float64) - CENTRE, axis=1) - RADIUS


def test_distance_to_the_sphere_is_within_a_cell_of_the_closed_form(surf):
    """The mesh's vertices lie within a depth-4 cell of the sphere of radius 0.3 (include/sdfhip.h: radii 0.277 .. 0.3008), so the
    distance to the mesh differs from |p - c| - r by less than one cell edge -- at every range, outside the cube included."""
    p, true = ray_points()
    assert (p > 1).any() and (p < 0).any()
    d = dr.dist(surf, p)
    err = np.abs(d - true)
    print("sphere: max |dist - closed form| =", err.max(), "of", S4)
    assert err.max() < S4


def test_where_the_sampled_distance_is_saturated_dist_is_not(sphere, surf):
    """The feature, stated: well away from the surface sdfhip_scene_sample's distance stalls at what a leaf's bytes can say
    ([-0.5 S, 1.5 S] of the leaf's edge S) while dist goes on to the true distance."""
    p, true = ray_points()
    far = np.abs(true) >= 0.2
    assert far.sum() >= 20
    with np.errstate(all="ignore"):
        sampled = qr.sample(*sphere, np.clip(p, 0, 1))["distance"]
    d = dr.dist(surf, p)
    print("far points: sampled", sampled[far].min(), "..", sampled[far].max(), "dist", d[far].min(), "..", d[far].max())
    assert (np.abs(sampled[far]) < 0.5 * np.abs(true[far])).all(), "the stored field is saturated there"
    assert (np.abs(sampled[far] - true[far]) > 0.1).all()
    assert (np.abs(d[far] - true[far]) < S4).all(), "... and the exact distance is not"
    assert (np.sign(d[far]) == np.sign(true[far])).all()


DELTA = 3 * S4


@pytest.mark.parametrize("sign", [+1, -1])
def test_offset_volume(sphere, surf, sign):
    """The source surface is within S of the sphere of radius r, so its offset by delta is within S of radius r + delta, and the
    result's own bytes (depth 4) are read by the measure: the volume lies between the balls of radius r + delta -+ S."""
    r = RADIUS + sign * DELTA
    S, V = built(sphere, surf, dr.GROW, sign * DELTA, 4)
    vol = msr.measure(S, V).volume
    print(f"offset {sign * DELTA:+}: {len(S)} nodes, volume {vol}, bracket {ball(r - S4)} .. {ball(r + S4)}")
    assert ball(r - S4) < vol < ball(r + S4)


def test_shell_volume(sphere, surf):
    """The wall of thickness t centred on the surface: its volume, and area * t with the source's measured area, both lie between
    the spherical shells whose two radii are each moved by S against and with the wall."""
    t = 4 * S4
    S, V = built(sphere, surf, dr.SHELL, t, 4)
    vol = msr.measure(S, V).volume
    area = msr.measure(*sphere).area
    lo = ball(RADIUS + t / 2 - S4) - ball(RADIUS - t / 2 + S4)
    hi = ball(RADIUS + t / 2 + S4) - ball(RADIUS - t / 2 - S4)
    print(f"shell {t}: {len(S)} nodes, volume {vol}, area * t {area * t}, bracket {lo} .. {hi}")
    assert 0 < lo < vol < hi and lo < area * t < hi
    # hollow: the centre is outside the wall, the sphere's surface inside it
    inside = lambda q: qr.sample(S, V, np.array([q], dtype=f32))["distance"][0] < 0
    assert not inside(CENTRE) and inside(CENTRE + [RADIUS, 0, 0]) and not inside([0.02, 0.02, 0.02])


def test_volume_is_monotone_in_delta(sphere, surf):
    vols = [msr.measure(*built(sphere, surf, dr.GROW, d, 3)).volume for d in (-0.15, -0.05, 0.0, 0.05, 0.15)]
    print("volumes over delta:", vols)
    assert all(a < b for a, b in zip(vols, vols[1:])) and vols[0] > 0


def test_an_empty_surface_and_a_surface_moved_out_give_the_root_alone(sphere, surf):
    empty = (np.array([[-1, -1]], dtype=np.int32), np.full((1, 8), 255, dtype=np.uint8))
    rec = dr.distance(*empty, [[0.5, 0.5, 0.5], [np.nan, 0, 0]])
    assert rec["distance"][0] == np.inf and rec["status"].tolist() == [dr.HIT, dr.INVALID] and rec["distance"][1] == 0
    S, V = dr.grow(empty, 0.1, 4)
    assert len(S) == 1 and (V == 255).all()
    S, V = dr.grow(sphere, -3.0, 4, surf=surf)          # shrunk until the value at the root's centre passes 2: nothing is left
    assert len(S) == 1 and (V > 63).all()
    S, V = dr.grow(sphere, 2.0, 4, surf=surf)           # grown past the cube's corners: everything is inside
    assert len(S) == 1 and (V <= 63).all()

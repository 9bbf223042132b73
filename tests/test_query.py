"""Point and ray queries (sdfhip_scene_sample / _raycast / _pick) without a GPU.  The numpy restatement of the three questions
(tests/query_restatement.py) is held to the FROZEN oracle here -- oracle.distance_at for points, the golden frames for the march --
so that tests/test_gpu_query.py, which holds the GPU to the restatement bit for bit, is not the builder's code compared with the
builder's code.  And the ABI as far as it goes without a device: names, record sizes, constants, a refused null scene."""
import ctypes
import os
import re

import numpy as np
import pytest

import edit_restatement as er
import query_restatement as qr
from conftest import CAMERAS, GOLDEN, REPO, bits_equal, make_camera

f32 = np.float32
SKY = np.array([0.005, 0.01, 0.2], dtype=np.float32)
QUERY_SYMBOLS = ("sdfhip_scene_sample", "sdfhip_scene_sample_device", "sdfhip_scene_raycast", "sdfhip_scene_raycast_device", "sdfhip_scene_pick")


def lattice_points(rng, depth, per_level=200):
    """points with coordinates on the lattice of every level 0..depth (multiples of 2^-k, 0 and 1 included): cell faces, edges and
    corners.  Per point each axis is on the lattice or uniform, at least one of them on it."""
    out = []
    for k in range(depth + 1):
        on = rng.integers(0, 2 ** k + 1, size=(per_level, 3)).astype(np.float64) / 2 ** k
        free = rng.random((per_level, 3))
        which = rng.random((per_level, 3)) < 0.6
        which[np.arange(per_level), rng.integers(0, 3, per_level)] = True
        out.append(np.where(which, on, free))
    return np.concatenate(out).astype(f32)


def outside_points(rng, per_side=100):
    """points beyond each of the six faces of [0,1]^3 (the other two coordinates inside or outside too)"""
    out = []
    for axis in range(3):
        for side in (0, 1):
            p = rng.uniform(-0.3, 1.3, size=(per_side, 3))
            p[:, axis] = rng.uniform(-0.5, -1e-4, per_side) if side == 0 else rng.uniform(1.0001, 1.5, per_side)
            out.append(p)
    return np.concatenate(out).astype(f32)


def point_sets(od, seed):
    rng = np.random.default_rng(seed)
    depth = er.tree_depth(od.Structs)
    centres, _ = er.deepest_leaf_centres(od.Structs)
    if len(centres) > 3000:
        centres = centres[rng.choice(len(centres), 3000, replace=False)]
    return {"uniform": rng.random((4000, 3)).astype(f32), "lattice": lattice_points(rng, depth), "outside": outside_points(rng),
            "leaf centres": centres.astype(f32)}


@pytest.mark.parametrize("name", ["sphere_d4", "torus_d6"])
def test_sample_is_the_oracles_distance_at(scenes, oracle_mod, name):
    od = scenes[name]
    for what, pts in point_sets(od, 11).items():
        got = qr.sample(od.Structs, od.Values, pts)
        assert (got["status"] == qr.HIT).all()
        want = np.array([oracle_mod.distance_at(od.Structs, od.Values, *p) for p in pts], dtype=np.float64)
        assert bits_equal(got["distance"], want[:, 0].astype(f32)).all(), (name, what)
        assert (got["node"] == want[:, 1].astype(np.uint32)).all(), (name, what)
        assert bits_equal(got["scale"], want[:, 2].astype(f32)).all(), (name, what)


def test_sample_flags_non_finite_points_and_nothing_else(scenes):
    od = scenes["torus_d6"]
    rng = np.random.default_rng(5)
    pts = rng.random((300, 3)).astype(f32)
    clean = qr.sample(od.Structs, od.Values, pts)
    bad = np.array([3, 64, 65, 200, 299])
    dirty = pts.copy()
    dirty[bad, [0, 1, 2, 0, 1]] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    got = qr.sample(od.Structs, od.Values, dirty)
    assert (np.nonzero(got["status"] == qr.INVALID)[0] == bad).all()
    assert not got[bad]["distance"].any() and not got[bad]["gradient"].any() and not got[bad]["node"].any() and not got[bad]["scale"].any()
    keep = np.setdiff1d(np.arange(300), bad)
    assert not qr.records_differ(got[keep], clean[keep])


def test_pick_agrees_with_the_oracles_frames(scenes):
    """Every pixel of the six golden 64x64 frames: ESCAPED exactly where the oracle's pixel is the sky constant, and there steps ==
    alpha; everywhere else HIT or EXHAUSTED with steps <= alpha (alpha also counts the shadow march's steps)."""
    g = np.load(os.path.join(GOLDEN, "frames.npz"))
    W = H = 64
    ys, xs = np.mgrid[0:H, 0:W]
    pixels = np.stack([xs.ravel(), ys.ravel()], 1)
    n_sky = n_all = 0
    for name in ("sphere_d4", "torus_d6"):
        od = scenes[name]
        for cam_name in CAMERAS:
            rgba = g[f"{name}/{cam_name}/rgba"].reshape(-1, 4)
            cam = make_camera(cam_name, W, H)
            got = qr.pick(od.Structs, od.Values, cam.State, pixels)
            sky = (rgba[:, :3].view(np.uint32) == SKY.view(np.uint32)).all(1)
            alpha = rgba[:, 3]
            assert np.isfinite(alpha).all()
            share = sky.mean()
            assert 0.03 <= share <= 0.97, (name, cam_name, share)          # neither class is a handful of pixels in any frame
            assert ((got["status"] == qr.ESCAPED) == sky).all(), (name, cam_name, int(((got["status"] == qr.ESCAPED) != sky).sum()))
            assert (got["steps"][sky] == alpha[sky]).all(), (name, cam_name)
            assert np.isin(got["status"][~sky], (qr.HIT, qr.EXHAUSTED)).all(), (name, cam_name)
            assert (got["steps"][~sky] <= alpha[~sky]).all(), (name, cam_name)
            # an EXHAUSTED pixel took every step the shader allows
            assert (got["steps"][got["status"] == qr.EXHAUSTED] == 100).all()
            n_sky += int(sky.sum()); n_all += len(sky)
    assert n_all == 6 * W * H
    assert 0.25 <= n_sky / n_all <= 0.75, n_sky / n_all                     # pooled: both classes hold a quarter of the pixels


@pytest.mark.parametrize("name", ["sphere_d4", "torus_d6"])
def test_raycast_along_the_cameras_rays_is_pick(scenes, name):
    od = scenes[name]
    W = H = 48
    ys, xs = np.mgrid[0:H, 0:W]
    pixels = np.stack([xs.ravel(), ys.ravel()], 1)
    for cam_name in CAMERAS:
        cam = make_camera(cam_name, W, H)
        o, d = qr.camera_rays(od.Structs, od.Values, cam.State, pixels)
        a = qr.pick(od.Structs, od.Values, cam.State, pixels, max_steps=60)
        b = qr.raycast(od.Structs, od.Values, o, d, cam.State.margin, cam.State.limit, max_steps=60)
        assert not qr.records_differ(b, a), (name, cam_name)


def test_raycast_refuses_bad_rays_per_element_and_counts_its_steps(scenes):
    od = scenes["sphere_d4"]
    o = np.tile(np.array([0.5, 0.5, -0.5], f32), (6, 1))
    d = np.tile(np.array([0.0, 0.0, 1.0], f32), (6, 1))
    d[1] = 0.0                      # all zero
    d[2, 1] = np.nan
    o[3, 0] = np.inf
    d[4] = (0.0, 1.0, 0.0)          # misses: leaves through the limit
    got = qr.raycast(od.Structs, od.Values, o, d, 0.001, 4.0, max_steps=100)
    assert got["status"].tolist() == [qr.HIT, qr.INVALID, qr.INVALID, qr.INVALID, qr.ESCAPED, qr.HIT]
    zero = np.zeros(1, qr.HIT_REC)
    zero["status"] = qr.INVALID
    for k in (1, 2, 3):
        assert got[k].tobytes() == zero.tobytes()
    assert not got[4]["normal"].any()
    # the sphere of radius 0.3 about the centre: the ray from z = -0.5 meets it near z = 0.2, t near 0.7
    assert abs(float(got[0]["position"][2]) - 0.2) < 0.02 and abs(float(got[0]["t"]) - 0.7) < 0.02 and got[0]["normal"][2] < -0.9
    one = qr.raycast(od.Structs, od.Values, o[:1], d[:1], 0.001, 4.0, max_steps=1)
    assert one["status"][0] == qr.EXHAUSTED and one["steps"][0] == 1 and one["t"][0] == one["prox"][0]
    # from inside the solid the distance is negative and the shader's rule steps backwards along the ray
    inside = qr.raycast(od.Structs, od.Values, [[0.5, 0.5, 0.5]], [[0.0, 0.0, 1.0]], 0.001, 4.0, max_steps=3)
    assert inside["prox"][0] < 0 or inside["t"][0] < 0


@pytest.mark.parametrize("name", ["sphere_d4", "torus_d6"])
def test_gradient_is_the_difference_quotient_of_the_trilinear_field(scenes, name):
    """Inside one cell the field is trilinear in the local coordinates, so along axis k it is linear and gradient[k] at p equals
    (D(b) - D(a)) / ((b - a) * 2 * scale), D = sample's distance at p with its local coordinate along k moved to a = 0.25, b = 0.75.

    Tolerance, from fp32 (eps = 2^-24 relative per rounding), in units of the decoded corner values v in [0, 1] (distance =
    (v - 0.25) * scale * 2, exact scalings):
      * the blend behind D is three nested lerps, each one rounding of a value <= 1, plus the rounding of the local coordinate
        feeding each of them (its error is scaled by a corner difference <= 1): <= 6 roundings of magnitude <= 1 per D, so
        |err D| <= 6 eps in v units, and the quotient divides the difference of two such by (b - a) = 1/2: <= 24 eps;
      * gradient[k] itself is the difference of two blends of two nested lerps each: <= 4 roundings per blend + 1 for the
        subtraction: <= 9 eps;
      * the moved coordinates (lower + 0.25 scale, lower + 0.75 scale) are exact for a cell of level <= 12 in fp32, but p's own
        local coordinates on the other two axes are recomputed from the same p in all three lookups: no further error.
    Bound: 33 eps, rounded up to 40 eps = 40 * 2^-24 ~ 2.4e-6."""
    od = scenes[name]
    rng = np.random.default_rng(23)
    centres, _ = er.deepest_leaf_centres(od.Structs)
    base = np.concatenate([rng.random((1500, 3)), centres[rng.choice(len(centres), min(1500, len(centres)), replace=False)]]).astype(f32)
    at = qr.sample(od.Structs, od.Values, base)
    scale = at["scale"].astype(np.float64)
    # the cell's lower corner, from the point and the scale (cells are dyadic: floor(p / scale) * scale; interior points only)
    lower = np.floor(base.astype(np.float64) / scale[:, None]) * scale[:, None]
    interior = ((base > lower + 0.01 * scale[:, None]) & (base < lower + 0.99 * scale[:, None])).all(1) & (base > 0).all(1) & (base < 1).all(1)
    assert interior.sum() > 2000
    tol = 40 * 2.0 ** -24
    checked = 0
    for k in range(3):
        pa, pb = base.astype(np.float64), base.astype(np.float64)
        pa[:, k] = lower[:, k] + 0.25 * scale
        pb[:, k] = lower[:, k] + 0.75 * scale
        a = qr.sample(od.Structs, od.Values, pa.astype(f32))
        b = qr.sample(od.Structs, od.Values, pb.astype(f32))
        same = interior & (a["node"] == at["node"]) & (b["node"] == at["node"])
        assert (same == interior).all(), "interior taps must stay in the cell of the point"
        quotient = (b["distance"].astype(np.float64) - a["distance"].astype(np.float64)) / (0.5 * 2.0 * scale)
        err = np.abs(quotient - at["gradient"][:, k].astype(np.float64))[same]
        assert err.max() <= tol, (name, k, float(err.max()), tol)
        checked += int(same.sum())
    assert checked > 6000
    # and the gradient points away from the solid: outside the torus / sphere's surface band the field grows outwards
    assert np.abs(at["gradient"]).max() > 0.1


# ---- the ABI without a device ---------------------------------------------------------------------------------------------------
def test_query_entry_points_are_declared_bound_and_exported(sb):
    from test_abi import declared_symbols, exported_symbols
    for name in QUERY_SYMBOLS:
        assert name in sb._lib.EXPORTED_SYMBOLS, name
        assert name in declared_symbols(), name
        assert name in exported_symbols(sb._lib.LIB_PATH), name
        assert name in exported_symbols(sb._lib.LAB_LIB_PATH), name


def test_query_records_and_constants_match_the_header(sb):
    text = open(os.path.join(REPO, "include", "sdfhip.h")).read()
    enums = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bSDFHIP_(QUERY_[A-Z]+)\s*=\s*(\d+)", text)}
    assert enums == {"QUERY_HIT": 0, "QUERY_ESCAPED": 1, "QUERY_EXHAUSTED": 2, "QUERY_INVALID": 3}
    for name, value in enums.items():
        assert getattr(sb, name) == value == getattr(qr, name[len("QUERY_"):])
    assert (ctypes.sizeof(sb.Probe), ctypes.sizeof(sb.Ray), ctypes.sizeof(sb.Hit)) == (32, 32, 48)
    # the restatement's records are the C records, field for field
    for mine, theirs in ((qr.PROBE, np.dtype(sb.Probe)), (qr.HIT_REC, np.dtype(sb.Hit))):
        assert mine.itemsize == theirs.itemsize
        for f in mine.names:
            assert mine.fields[f][1] == theirs.fields[f][1] and mine.fields[f][0] == theirs.fields[f][0], f
    assert sb.Ray.dir.offset == 16 and sb.Hit.status.offset == 32 and sb.Probe.gradient.offset == 16


def test_queries_refuse_a_null_scene_without_a_gpu(sb):
    L = sb._lib.lib
    buf = (ctypes.c_uint8 * 64)()
    info = sb.Logic(64, 64).State
    calls = {
        "sdfhip_scene_sample": lambda: L.sdfhip_scene_sample(None, buf, 1, buf),
        "sdfhip_scene_sample_device": lambda: L.sdfhip_scene_sample_device(None, buf, 1, buf, None),
        "sdfhip_scene_raycast": lambda: L.sdfhip_scene_raycast(None, buf, 1, 0.001, 4.0, 100, buf),
        "sdfhip_scene_raycast_device": lambda: L.sdfhip_scene_raycast_device(None, buf, 1, 0.001, 4.0, 100, buf, None),
        "sdfhip_scene_pick": lambda: L.sdfhip_scene_pick(None, ctypes.byref(info), buf, 1, 100, buf),
    }
    assert set(calls) == set(QUERY_SYMBOLS)
    for name, call in calls.items():
        assert call() == sb._lib.ERR_ARG, name
        assert b"null" in L.sdfhip_last_error(), name
    assert not any(buf)

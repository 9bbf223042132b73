"""Placement (sdfhip_scene_place) without a GPU: the CPU restatement (tests/place_restatement.py) is held to things it did not come
from -- which way the rotation turns and the scale scales, the closed form of a placed sphere, the structure of a breadth-first
tree -- the entry point refuses what it must refuse before it touches a device, and the Python mirror's records are the header's.
tests/test_gpu_place.py holds the GPU to the restatement byte for byte."""
import ctypes
import os
import re

import numpy as np
import pytest

import place_restatement as plr
import query_restatement as qr
from conftest import REPO
from test_combine import assert_breadth_first

OFF = (0.66, 0.5, 0.42, 0.17)                  # the off-centre sphere, depth 7
TURN_Z = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], dtype=np.float32)      # 90 degrees about z: x -> y
# |sampled distance - closed form| within one leaf of the placed sphere's surface, measured with the cases of
# test_against_the_closed_form: the translation 4.706e-3, the generic rotation at half size 5.996e-3, of a
# leaf of 7.81e-3.  Most of it is saturation, not resampling: inside, a byte cannot say less than -0.5 of its leaf's edge, and the
# half-size source's bytes stop at 1.5 of ITS leaf, which is 0.75 of the result's (outside the surface, where the result's own bytes do
# not saturate: 8.95e-4 and 2.91e-3).  The bound is twice the larger: the margin covers the source's own quantisation and trilinear
# error, which the test does not control.
CLOSED_FORM_BOUND = 2 * 5.996e-3


@pytest.fixture(scope="module")
def off(sb):
    od = sb.OctData.Generate(sb._lib.SHAPE_SPHERE, list(OFF), 7)
    S, V = od.Structs, od.Values
    S.setflags(write=False); V.setflags(write=False)
    return S, V


_placed = {}


def placed(sb, off, name):
    """(structs, values, counts, (R, s, t)) of the named placements of the off-centre sphere, made once and left unchanged"""
    if name not in _placed:
        depth = -1
        if name == "turned_half":
            pl = (TURN_Z, 0.5, (0.5, 0.4, 0.2))
        elif name == "moved":
            pl = (plr.IDENTITY, 1.0, (-0.11, 0.07, 0.13))
        elif name == "generic_half":
            pl = sb.placement(30, 20, 0, 0.5, about=OFF[:3], to=(0.4, 0.5, 0.55))
        elif name == "outside":
            pl = (plr.IDENTITY, 1.0, (3.0, 0.0, 0.0))
        elif name == "depth_0":
            pl, depth = (plr.IDENTITY, 1.0, (0.0, 0.0, 0.0)), 0
        _placed[name] = plr.place(off, *pl, depth, want_counts=True) + (plr.as_placement(*pl),)
    return _placed[name]


def distance(S, V, points):
    return qr.sample(S, V, np.asarray(points, dtype=np.float32).reshape(-1, 3))["distance"]


def test_conventions(sb, off):
    # a source point x lands at s R x + t: the sphere's centre, and with it the inside, lands THERE -- not where the transposed
    # rotation or the inverted scale would have put it
    S, V, _, (R, s, t) = placed(sb, off, "turned_half")
    c = np.array(OFF[:3], dtype=np.float64)
    R, t = R.astype(np.float64), t.astype(np.float64)
    here, transposed, inverted = float(s) * R @ c + t, float(s) * R.T @ c + t, (1.0 / float(s)) * R @ c + t
    assert np.allclose(here, (0.25, 0.73, 0.41)) and np.allclose(transposed, (0.75, 0.07, 0.41))
    assert ((here > 0.1) & (here < 0.9)).all() and ((transposed > 0) & (transposed < 1)).all()
    d = distance(S, V, [here, transposed, inverted])
    assert d[0] < 0 and d[1] > 0 and d[2] > 0, d.tolist()
    # the source itself is negative at c and positive at the three
    d0 = distance(*off, [c, here, transposed])
    assert d0[0] < 0 and d0[1] > 0 and d0[2] > 0


@pytest.mark.parametrize("name", ["moved", "generic_half"])
def test_against_the_closed_form(sb, off, name):
    S, V, counts, (R, s, t) = placed(sb, off, name)
    centre = float(s) * R.astype(np.float64) @ np.array(OFF[:3]) + t.astype(np.float64)
    radius = float(s) * OFF[3]
    leaf = 2.0 ** -counts["depth_out"]
    rng = np.random.default_rng(5)
    u = rng.normal(size=(3000, 3))
    u /= np.sqrt((u * u).sum(1))[:, None]
    p = (centre + u * (radius + rng.uniform(-leaf, leaf, size=(3000, 1)))).astype(np.float32)
    assert ((p > 0.02) & (p < 0.98)).all(), "the placed sphere and its band lie inside the cube"
    want = np.sqrt(((p.astype(np.float64) - centre) ** 2).sum(1)) - radius
    err = np.abs(distance(S, V, p).astype(np.float64) - want)
    print(f"{name}: {len(S)} nodes, depth {counts['depth_out']}, max |sampled - closed form| = {err.max():.3e} (leaf {leaf:.3e}); "
          f"outside the surface, where no byte saturates: {err[want > 0].max():.3e}")
    assert err.max() <= CLOSED_FORM_BOUND, (name, err.max())


@pytest.mark.parametrize("name", ["turned_half", "moved", "generic_half", "outside", "depth_0"])
def test_structure(sb, off, name):
    S, V, counts, _ = placed(sb, off, name)
    assert assert_breadth_first(sb, S, V) == counts["depth_out"] == counts["levels"] - 1
    n_blocks = (len(S) - 1) // 8
    assert counts["samples"] == 9 + 35 * n_blocks
    if name in ("outside", "depth_0"):
        assert len(S) == 1 and tuple(S[0]) == (-1, -1), "the root alone"
    else:
        assert counts["depth_out"] == 7 and len(S) > 1000
    if name == "outside":
        assert (V == 255).all(), "far outside: every byte saturated"
    if name == "depth_0":                          # the root's bytes are the uncut placement's root's
        whole = plr.place(off, plr.IDENTITY, 1.0, (0, 0, 0), 1)
        assert np.array_equal(V, whole[1][:1]) and len(whole[0]) == 9


def test_the_identity_is_a_resampling_not_a_clone(sb):
    od = sb.sphere_d4()
    S, V = plr.place((od.Structs, od.Values), plr.IDENTITY, 1.0, (0, 0, 0))
    assert (len(od.Structs), len(S)) == (3465, 4681)                  # include/sdfhip.h quotes both
    assert len(plr.place((od.Structs, od.Values), plr.IDENTITY, 1.0, (0.25, 0, 0))[0]) == 3849


def test_the_placement_helper(sb):
    R, s, t = sb.placement(0, 0, 0)
    assert R.dtype == np.float32 and t.dtype == np.float32 and isinstance(s, np.float32)
    assert np.array_equal(R, np.eye(3)) and s == 1 and np.array_equal(t, np.zeros(3))
    # yaw turns about y (z towards x), pitch about x (y towards z), roll about z (x towards y): right-handed
    for angles, src, dst in (((90, 0, 0), (0, 0, 1), (1, 0, 0)), ((0, 90, 0), (0, 1, 0), (0, 0, 1)), ((0, 0, 90), (1, 0, 0), (0, 1, 0))):
        R, _, _ = sb.placement(*angles, about=(0, 0, 0), to=(0, 0, 0))
        assert np.allclose(R @ np.array(src, dtype=np.float32), dst, atol=1e-7), angles
    R, s, t = sb.placement(30, 20, -70, 0.37, about=(0.2, 0.6, 0.5), to=(0.7, 0.3, 0.4))
    assert np.abs(R.astype(np.float64) @ R.astype(np.float64).T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R.astype(np.float64)) - 1) < 1e-6
    assert np.allclose(float(s) * R.astype(np.float64) @ np.array((0.2, 0.6, 0.5)) + t, (0.7, 0.3, 0.4), atol=1e-6)
    # R = Ry(yaw) Rx(pitch) Rz(roll): the roll is applied to the source first
    Ry, Rx, Rz = sb.placement(30, 0, 0)[0], sb.placement(0, 20, 0)[0], sb.placement(0, 0, -70)[0]
    assert np.allclose(R, Ry.astype(np.float64) @ Rx.astype(np.float64) @ Rz.astype(np.float64), atol=1e-6)


def test_place_refuses_bad_arguments_without_a_gpu(sb):
    L = sb._lib

    def call(pl, scene=None, want_out=True, data=None):
        out = ctypes.c_void_p(1)
        rc = L.lib.sdfhip_scene_place(scene, ctypes.byref(pl) if pl is not None else None, ctypes.byref(out) if want_out else None,
                                      ctypes.byref(data) if data is not None else None, None)
        assert not want_out or out.value is None, "*out is not null after a failure"
        return rc, L.lib.sdfhip_last_error()

    good = lambda **kw: sb.Placement(**kw)
    assert call(None) == (L.ERR_ARG, b"scene_place: null placement")
    rc, msg = call(good())                              # a valid placement reaches the scene check
    assert rc == L.ERR_ARG and b"null scene" in msg
    rc, msg = call(good(), want_out=False)
    assert rc == L.ERR_ARG and b"both outputs" in msg
    rc, msg = call(good(), want_out=False, data=L.COctData())       # host_out alone is an output
    assert rc == L.ERR_ARG and b"null scene" in msg
    for size in (4, 56, 61, 4100):                      # the size rules of sdfhip_prune_options
        pl = good()
        pl.size = size
        rc, msg = call(pl)
        assert rc == L.ERR_ARG and b"bytes" in msg, size

    class Newer(ctypes.Structure):
        _fields_ = sb.Placement._fields_ + [("unknown", ctypes.c_int32)]
    newer = Newer()
    ctypes.memmove(ctypes.byref(newer), ctypes.byref(good()), 60)
    newer.size, newer.unknown = 64, 5
    as_placement = ctypes.cast(ctypes.pointer(newer), ctypes.POINTER(sb.Placement)).contents
    rc, msg = call(as_placement)
    assert rc == L.ERR_ARG and b"does not know" in msg
    newer.unknown = -1                                  # a newer struct whose new field says "default" passes the record's check
    rc, msg = call(as_placement)
    assert rc == L.ERR_ARG and b"null scene" in msg
    for bad in (float("nan"), float("inf"), -float("inf")):
        for pl in (good(scale=bad), good(translation=(0, bad, 0)), good(rotation=((1, 0, 0), (0, 1, 0), (0, bad, 1)))):
            rc, msg = call(pl)
            assert rc == L.ERR_ARG and b"finite" in msg, bad
    for scale in (0.0, -0.0, -1.0):
        rc, msg = call(good(scale=scale))
        assert rc == L.ERR_ARG and b"scale" in msg, scale
    for rotation in (((1, 0, 0), (0, 1, 0), (0, 0, 1.001)), ((1, 2e-4, 0), (0, 1, 0), (0, 0, 1)), ((0, 0, 0), (0, 0, 0), (0, 0, 0)),
                     ((2, 0, 0), (0, 0.5, 0), (0, 0, 1))):
        rc, msg = call(good(rotation=rotation))
        assert rc == L.ERR_ARG and b"orthogonal" in msg, rotation
    # inside the bound: a rotation rounded to float32, one off by 5e-5, a mirror
    for rotation in (sb.placement(30, 20, -70)[0], ((1, 5e-5, 0), (0, 1, 0), (0, 0, 1)), ((-1, 0, 0), (0, 1, 0), (0, 0, 1))):
        rc, msg = call(good(rotation=np.asarray(rotation).tolist()))
        assert rc == L.ERR_ARG and b"null scene" in msg, rotation
    for depth in (-2, 13, 100):
        rc, msg = call(good(depth=depth))
        assert rc == L.ERR_ARG and b"depth" in msg, depth
    for depth in (None, 0, 12):
        rc, msg = call(good(depth=depth))
        assert rc == L.ERR_ARG and b"null scene" in msg, depth


def test_a_valid_placement_needs_a_gpu_and_says_so(sb):
    # the product has no CPU path: with valid arguments the call runs on the device, or there is no scene to place
    import torch
    od = sb.sphere_d4()
    if torch.cuda.is_available():
        with sb.Scene(od) as scene, scene.Place(*sb.placement(30, 20, 0, 0.5)) as res:
            assert res.Length > 1
    else:
        with pytest.raises(sb.SdfHipError) as e:
            sb.Scene(od).Place(*sb.placement(30, 20, 0, 0.5))
        assert e.value.code == sb._lib.ERR_DEVICE


def test_records_match_the_header(sb):
    text = open(os.path.join(REPO, "include", "sdfhip.h")).read()
    record = lambda name: re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    fields = lambda body: [re.sub(r"\[.*", "", f.strip()) for decl in re.findall(r"(?:uint32_t|int32_t|uint64_t|float)\s+([^;]+);", body)
                           for f in decl.split(",")]
    assert fields(record("sdfhip_placement")) == [f for f, _ in sb.Placement._fields_]
    assert fields(record("sdfhip_place_stats")) == [f for f, _ in sb.PlaceStats._fields_]
    P, T = sb.Placement, sb.PlaceStats
    assert ctypes.sizeof(P) == 60 and (P.rotation.offset, P.scale.offset, P.translation.offset, P.depth.offset) == (4, 40, 44, 56)
    assert ctypes.sizeof(T) == 40 and (T.samples.offset, T.kernel_ms.offset, T.total_ms.offset) == (16, 24, 32)
    pl = sb.Placement()
    assert (pl.size, pl.scale, pl.depth) == (60, 1.0, -1) and [list(r) for r in pl.rotation] == np.eye(3).tolist()
    assert "sdfhip_scene_place" in sb._lib.EXPORTED_SYMBOLS and hasattr(sb.Scene, "Place")
    assert not re.search(r"sdfhip_place\w*_default", text), "no entry point that cannot throw"

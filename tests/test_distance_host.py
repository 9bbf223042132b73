"""The host half of sdfhip_scene_distance / sdfhip_scene_offset without a GPU: the Python mirror's records are the header's, field
for field and byte for byte, the options record grows by the rule of sdfhip_prune_options, and the entry points refuse what they
must refuse before they touch a device -- every refusal of the options comes ahead of the scene check, so a null scene reaches all
of them with no device present.  What needs a handle (SDFHIP_ERR_BAD_TREE, the query's null pointers behind a valid scene) is in
tests/test_gpu_distance.py."""
import ctypes
import os
import re

import numpy as np

import distance_restatement as dr
from conftest import REPO


def test_records_match_the_header(sb):
    text = open(os.path.join(REPO, "include", "sdfhip.h")).read()
    record = lambda name: re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    fields = lambda body: [re.sub(r"\[.*", "", f.strip()) for decl in re.findall(r"(?:uint32_t|int32_t|uint64_t|float)\s+([^;]+);", body)
                           for f in decl.split(",")]
    C, O, T = sb.Clearance, sb.OffsetOptions, sb.OffsetStats
    assert fields(record("sdfhip_clearance")) == [f for f, _ in C._fields_]
    assert fields(record("sdfhip_offset_options")) == [f for f, _ in O._fields_]
    assert fields(record("sdfhip_offset_stats")) == [f for f, _ in T._fields_]
    assert ctypes.sizeof(C) == 32 and (C.distance.offset, C.node.offset, C.nearest.offset, C.status.offset, C.visited.offset, C.pad_.offset) == (0, 4, 8, 20, 24, 28)
    assert ctypes.sizeof(O) == 20 and (O.size.offset, O.mode.offset, O.amount.offset, O.depth.offset, O.level.offset) == (0, 4, 8, 12, 16)
    assert ctypes.sizeof(T) == 48 and (T.levels.offset, T.points.offset, T.visited.offset, T.kernel_ms.offset, T.total_ms.offset) == (12, 16, 24, 32, 40)
    # the restatement's record and numpy's view of the ctypes one are the same layout
    assert np.dtype(C).itemsize == dr.CLEARANCE.itemsize == 32
    assert {n: np.dtype(C).fields[n][1] for n in dr.CLEARANCE.names} == {n: dr.CLEARANCE.fields[n][1] for n in dr.CLEARANCE.names}
    enum = dict(re.findall(r"SDFHIP_(OFFSET_\w+) = (\d+)", text))
    assert enum == {"OFFSET_GROW": "0", "OFFSET_SHELL": "1"} and (sb.OFFSET_GROW, sb.OFFSET_SHELL) == (0, 1) == (dr.GROW, dr.SHELL)
    opt = sb.OffsetOptions()
    assert (opt.size, opt.mode, opt.amount, opt.depth, opt.level) == (20, 0, 0.0, -1, -1)
    for name in ("sdfhip_scene_distance", "sdfhip_scene_distance_device", "sdfhip_scene_offset"):
        assert name in sb._lib.EXPORTED_SYMBOLS
    assert all(hasattr(sb.Scene, m) for m in ("Distance", "DistanceDevice", "Offset", "Shell"))


def test_offset_refuses_bad_arguments_without_a_gpu(sb):
    L = sb._lib

    def call(opt, scene=None, want_out=True, data=None):
        out = ctypes.c_void_p(1)
        rc = L.lib.sdfhip_scene_offset(scene, ctypes.byref(opt) if opt is not None else None, ctypes.byref(out) if want_out else None,
                                       ctypes.byref(data) if data is not None else None, None)
        assert not want_out or out.value is None, "*out is not null after a failure"
        return rc, L.lib.sdfhip_last_error()

    good = lambda **kw: sb.OffsetOptions(**dict(dict(mode=L.OFFSET_GROW, amount=0.03), **kw))
    assert call(None) == (L.ERR_ARG, b"scene_offset: null options")
    rc, msg = call(good())                              # valid options reach the scene check
    assert rc == L.ERR_ARG and b"null scene" in msg
    for ok in (good(amount=-0.5), good(amount=0.0), good(mode=L.OFFSET_SHELL, amount=1e-3), good(depth=0), good(depth=12), good(level=0), good(level=12)):
        rc, msg = call(ok)
        assert rc == L.ERR_ARG and b"null scene" in msg, msg
    rc, msg = call(good(), want_out=False)
    assert rc == L.ERR_ARG and b"both outputs" in msg
    rc, msg = call(good(), want_out=False, data=L.COctData())       # host_out alone is an output
    assert rc == L.ERR_ARG and b"null scene" in msg
    for bad, word in ((good(amount=float("nan")), b"finite"), (good(amount=float("inf")), b"finite"), (good(amount=-float("inf")), b"finite"),
                      (good(mode=L.OFFSET_SHELL, amount=0.0), b"thickness"), (good(mode=L.OFFSET_SHELL, amount=-0.25), b"thickness"),
                      (good(mode=2), b"mode"), (good(mode=-1), b"mode"), (good(depth=13), b"depth"), (good(depth=-2), b"depth"),
                      (good(level=13), b"level"), (good(level=-2), b"level")):
        rc, msg = call(bad)
        assert rc == L.ERR_ARG and word in msg and b"null scene" not in msg, (bad.mode, bad.amount, bad.depth, bad.level, msg)
    for size in (4, 16, 21, 4100):                      # the size rules of sdfhip_prune_options
        opt = good()
        opt.size = size
        rc, msg = call(opt)
        assert rc == L.ERR_ARG and b"bytes" in msg, size

    class Newer(ctypes.Structure):
        _fields_ = sb.OffsetOptions._fields_ + [("unknown", ctypes.c_int32)]
    newer = Newer()
    ctypes.memmove(ctypes.byref(newer), ctypes.byref(good()), 20)
    newer.size, newer.unknown = 24, 5
    as_options = ctypes.cast(ctypes.pointer(newer), ctypes.POINTER(sb.OffsetOptions)).contents
    rc, msg = call(as_options)
    assert rc == L.ERR_ARG and b"does not know" in msg
    newer.unknown = -1                                  # a newer struct whose new field says "default" passes the record's check
    rc, msg = call(as_options)
    assert rc == L.ERR_ARG and b"null scene" in msg


def test_distance_refuses_a_null_scene_without_a_gpu(sb):
    # (the level and the pointers are checked behind the scene pointer: with a handle, in tests/test_gpu_distance.py)
    L = sb._lib
    p = np.zeros((2, 3), np.float32)
    out = np.zeros(2, dr.CLEARANCE)
    assert L.lib.sdfhip_scene_distance(None, p.ctypes.data, 2, -1, out.ctypes.data) == L.ERR_ARG
    assert b"scene_distance: null scene" in L.lib.sdfhip_last_error()
    assert L.lib.sdfhip_scene_distance_device(None, None, 0, -1, None, None) == L.ERR_ARG
    assert b"scene_distance_device: null scene" in L.lib.sdfhip_last_error()

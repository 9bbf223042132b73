"""sdfhip_trimesh_build on the GPU, both flavours of the library: `structs` and `values` are the numpy restatement's
(tests/trimesh_restatement.py: brute force over all records, no pruning; held to closed-form truth by tests/test_trimesh.py) byte for
byte when it is given the library's own records; the returned handle renders what its host arrays render; the pruning changes no
byte (the laboratory's SDFHIP_TRI_PRUNE=0 keeps every record in every block) and saves work; memory failures and bad arguments are
status codes."""
import ctypes
import os

import numpy as np
import pytest

import mesh_restatement as mr
import trimesh_restatement as tr
from conftest import assert_frames_identical, make_camera

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module", params=["product", "lab"])
def sb(request):
    import sdfbox_amd
    if request.param == "product":
        return sdfbox_amd
    import sdfbox_amd.lab
    return sdfbox_amd.lab.load()


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def soup_of(name):
    import sdfbox_amd as base
    if name == "sphere":
        return cached(("soup", name), lambda: mr.mesh(base.sphere_d4().Structs, base.sphere_d4().Values, -1)[..., :3].copy())
    if name == "torus":
        def make():
            with base.Scene(base.torus_d6()) as scene:         # (bit for bit mesh_restatement's: tests/test_gpu_mesh.py)
                return scene.Mesh(-1, want_stats=False)[..., :3].copy()
        return cached(("soup", name), make)
    return cached(("soup", name), getattr(tr, name))


def assert_tree(got, want, what):
    S, V = want
    assert got.Length == len(S), (what, got.Length, len(S))
    assert (got.Structs == S).all(), (what, "structs", np.nonzero((got.Structs != S).any(1))[0][:5])
    bad = np.nonzero((got.Values != V).any(1))[0]
    assert not len(bad), (what, "values", len(bad), bad[:5], got.Values[bad[:2]], V[bad[:2]])


@pytest.mark.parametrize("name", ["tetrahedron", "cube", "l_prism"])
def test_small_meshes_are_the_restatements(sb, name):
    with sb.TriMesh.FromSoup(soup_of(name)) as m:
        R = m.records.copy()
        for depth in (0, 1, 4, 5):
            want = cached(("build", name, depth), lambda: tr.build(R, depth, want_float=True))
            scene, od, st = m.Build(depth, want_octdata=True, want_stats=True)
            with scene:
                assert scene.Length == od.Length and scene.stack_kernel_ok
                assert (st.nodes, st.records) == (od.Length, len(R)) and st.levels == scene.depth + 1 and st.candidate_entries >= len(R)
                assert st.build_ms > 0 and st.total_ms >= st.scene_ms >= 0
            assert_tree(od, want[:2], (name, depth))
            if depth == 4:
                assert scene.depth == 4
    if name == "l_prism":
        # split nodes on both sides of the reflex edge: inside the solid and in the notch
        coords, _, mv = cached(("build", name, 5), None)[2][4]
        S = 2.0 ** -4
        c = (coords + 0.5) * S
        split = np.abs(mv) < f32(2 * S)
        near = split & (np.abs(c[:, 0] - tr.L_REFLEX) < 2 * S) & (np.abs(c[:, 1] - tr.L_REFLEX) < 2 * S) & (c[:, 2] > 0.3) & (c[:, 2] < 0.7)
        notch = near & (c[:, 0] > tr.L_REFLEX) & (c[:, 1] > tr.L_REFLEX)
        assert (mv[notch] > 0).any() and (mv[near & ~notch] < 0).any()
        assert len(cached(("build", name, 5), None)[2]) == 6


def test_sphere_mesh_depth_4(sb):
    soup = soup_of("sphere")
    assert len(soup) == 2520
    with sb.TriMesh.FromSoup(soup) as m:                       # fit = 0: the mesh of the scene lands where the scene was
        R = m.records.copy()
        want = cached(("build", "sphere", 4), lambda: tr.build(R, 4))
        scene, od = m.Build(4, want_octdata=True)
    assert_tree(od, want, "sphere")
    cam = make_camera("rotated", 64, 64)
    with scene, sb.Scene(od) as again:
        assert scene.stack_kernel_ok and scene.depth == 4 and scene.Length == od.Length
        assert_frames_identical(scene.Draw(cam, 64, 64), again.Draw(cam, 64, 64), "handle against its host arrays")


def test_pruning_is_invisible_and_saves_work():
    import sdfbox_amd as product
    import sdfbox_amd.lab
    lab = sdfbox_amd.lab.load()
    soup = soup_of("torus")
    assert len(soup) == 31880
    with product.TriMesh.FromSoup(soup) as m:
        R = m.records.copy()
        scene, od, st = m.Build(7, want_octdata=True, want_stats=True)
        scene.close()
    os.environ["SDFHIP_TRI_PRUNE"] = "0"
    try:
        with lab.TriMesh.FromSoup(soup) as m:
            brute, st_brute = m.Build(7, want_scene=False, want_octdata=True, want_stats=True)
    finally:
        del os.environ["SDFHIP_TRI_PRUNE"]
    assert_tree(od, (brute.Structs, brute.Values), "pruned against every record in every block")
    blocks = 1 + int((od.Structs[:, 1] >= 0).sum())             # the root's, and one per internal node
    assert st_brute.candidate_entries == blocks * len(R)
    assert st.candidate_entries < st_brute.candidate_entries // 10 and st.nodes == st_brute.nodes == od.Length
    # 256 seeded nodes against the restatement at their boxes
    depth, coord = mr.walk(od.Structs)
    internal = od.Structs[:, 1] >= 0
    rng = np.random.default_rng(7)
    pick = np.concatenate([rng.choice(np.nonzero(sel)[0], n, replace=False) for sel, n in
                           ((internal & (depth < 7), 96), (~internal & (depth < 7), 64), (depth == 7, 96))])
    assert len(pick) == 256 and internal[pick].any() and (~internal[pick]).any()
    for d in np.unique(depth[pick]):
        nodes = pick[depth[pick] == d]
        cv, mv = tr.node_values(R, coord[nodes], int(d))
        S = f32(2.0 ** -int(d))
        assert (tr.from_float(cv, S) == od.Values[nodes]).all(), d
        assert ((np.abs(mv) < f32(2) * S) & (d < 7) == internal[nodes]).all(), d       # both split outcomes are among them


def test_memory_and_stats(sb):
    L = sb._lib
    with sb.TriMesh.FromSoup(soup_of("l_prism")) as m:
        scene = m.Build(5)                                      # host_out NULL: a handle and nothing copied out
        with scene:
            n = scene.Length
            assert n > 100 and scene.depth == 5
        od = m.Build(5, want_scene=False, want_octdata=True)    # scene NULL: the arrays alone
        assert od.Length == n
        if L.EXPERIMENTS:
            for k in (0, 2, 7, 15):
                os.environ["SDFHIP_TRI_FAIL_ALLOC"] = str(k)
                try:
                    h = ctypes.c_void_p()
                    raw = L.COctData()
                    rc = L.lib.sdfhip_trimesh_build(0, ctypes.byref(m._raw), 5, ctypes.byref(h), ctypes.byref(raw), None)
                finally:
                    del os.environ["SDFHIP_TRI_FAIL_ALLOC"]
                assert rc == L.ERR_NOMEM and not h.value and raw.length == 0 and not raw.structs, k
                assert b"out of device memory" in L.lib.sdfhip_last_error()
            with m.Build(5) as scene:
                assert scene.Length == n


def test_errors_are_status_codes(sb):
    L = sb._lib
    with sb.TriMesh.FromSoup(soup_of("cube")) as m:
        h = ctypes.c_void_p()
        raw = L.COctData()
        build = L.lib.sdfhip_trimesh_build
        assert build(0, None, 3, ctypes.byref(h), None, None) == L.ERR_ARG
        assert build(0, ctypes.byref(m._raw), 3, None, None, None) == L.ERR_ARG            # both outputs NULL
        assert build(0, ctypes.byref(m._raw), 13, ctypes.byref(h), None, None) == L.ERR_ARG
        assert build(0, ctypes.byref(m._raw), -1, ctypes.byref(h), None, None) == L.ERR_ARG
        empty = L.CTriMesh()
        assert build(0, ctypes.byref(empty), 3, ctypes.byref(h), None, None) == L.ERR_ARG
        assert build(99, ctypes.byref(m._raw), 3, ctypes.byref(h), None, None) == L.ERR_DEVICE
        assert not h.value
        assert build(0, ctypes.byref(m._raw), 3, ctypes.byref(h), ctypes.byref(raw), None) == L.OK and h.value and raw.length > 8
        L.lib.sdfhip_scene_free(h)
        L.lib.sdfhip_octdata_free(ctypes.byref(raw))

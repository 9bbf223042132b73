"""sdfhip_trimesh_build on the GPU, both flavours of the library: `structs` and `values` are the numpy restatement's
(tests/trimesh_restatement.py: brute force over all records, no pruning; held to closed-form truth by tests/test_trimesh.py) byte for
byte when it is given the library's own records; the returned handle renders what its host arrays render; the pruning changes no
byte (the laboratory's SDFHIP_TRI_PRUNE=0 keeps every record in every block) and saves work; memory failures and bad arguments are
status codes.  The adversarial soups of the restatement (far coordinates, long thin strips, a fan, two sheets that tie with opposite
signs, a triangle whose D is NaN, fit = 1) hold the pruning's slack, the tie rule and the work done by the lists
(`candidate_entries` equals build_pruned's, exactly); a level of more than 262 144 nodes holds the scans' carry."""
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


def pruned_of(name, R, depth):
    """build_pruned's candidate_entries at `depth` and its per-level list lengths: one run at the deepest depth any test asks of
    the soup (a level's lists do not depend on the levels below it)"""
    deepest = 6 if name == "two_sheets" else 5
    tree = cached(("pruned", name), lambda: tr.build_pruned(R, deepest, want_lists=True))
    lengths = tree[3][:depth + 1]
    return sum(int(l.sum()) for l in lengths), lengths, tree


@pytest.mark.parametrize("name", list(tr.ADVERSARIAL))
def test_adversarial_meshes_are_the_restatements(sb, name):
    fit = tr.ADVERSARIAL[name]
    soup = soup_of(name)
    with sb.TriMesh.FromSoup(soup, fit=fit) as m:
        R = m.records.copy()
        if fit:
            _, s, mid = tr.fit_positions(soup, 0.8)
            assert np.float32(m.scale) == s and (np.asarray(m.offset, dtype=f32) == mid).all()
            assert (R[:, :9].view(np.uint32) == (tr.fit_positions(soup, 0.8)[0] + f32(0)).reshape(-1, 9).view(np.uint32)).all()
        for depth in ((0, 5) if name in ("far_away", "cube_fit") else (5,)):
            want = cached(("build", name, depth), lambda: tr.build(R, depth, want_float=True))
            od, st = m.Build(depth, want_scene=False, want_octdata=True, want_stats=True)
            assert_tree(od, want[:2], (name, depth))
            entries, lengths, _ = pruned_of(name, R, depth)
            assert st.candidate_entries == entries, (name, depth, st.candidate_entries, entries)
            assert st.levels == len(lengths) and st.records == len(R)
    if name == "far_away":
        assert od.Length == 1 and (od.Values == 255).all()
    if name == "strips_far":
        assert np.abs(R[:, :9]).max() > 900
    if name == "two_sheets":
        # corners on z = 0.5 over the sheets: a record of sheet B and its image in sheet A tie; had the higher index won, the sign
        # and with it the byte would be the other one
        flipped = 0
        for lvl, (coords, cv, _) in enumerate(want[2]):
            S = f32(2.0 ** -lvl)
            c = ((coords[:, None, :] + tr.CORNER[None]).astype(f32) * S).reshape(-1, 3)
            over = (c[:, 2] == 0.5) & (c[:, 0] >= 0.375) & (c[:, 0] <= 0.625) & (c[:, 1] >= 0.4375) & (c[:, 1] <= 0.5703125)
            v = cv.reshape(-1)[over]
            assert (v == f32(-0.125)).all()
            flipped += int((tr.from_float(-v, S) != tr.from_float(v, S)).sum())
            assert (tr.from_float(v, S) == od.Values[sum(len(f[0]) for f in want[2][:lvl]):][:len(coords)].reshape(-1)[over]).all()
        assert flipped >= 64


def test_pruning_is_invisible_on_adversarial_meshes():
    import sdfbox_amd as product
    import sdfbox_amd.lab
    lab = sdfbox_amd.lab.load()
    for name in ("strips_far", "cone_fan", "two_sheets", "sliver"):
        soup = soup_of(name)
        with product.TriMesh.FromSoup(soup) as m:
            od, st = m.Build(6, want_scene=False, want_octdata=True, want_stats=True)
        os.environ["SDFHIP_TRI_PRUNE"] = "0"
        try:
            with lab.TriMesh.FromSoup(soup) as m:
                brute, st_brute = m.Build(6, want_scene=False, want_octdata=True, want_stats=True)
        finally:
            del os.environ["SDFHIP_TRI_PRUNE"]
        assert_tree(od, (brute.Structs, brute.Values), (name, "pruned against every record in every block"))
        blocks = 1 + int((od.Structs[:, 1] >= 0).sum())
        assert st_brute.candidate_entries == blocks * st.records and st.levels == 7
        assert st.candidate_entries < st_brute.candidate_entries, name


def test_both_wave_widths_see_long_lists(sb):
    """two_sheets at depth 6: its last level has 512 blocks or more, so k_tri_eval<4> runs it, 256 records a chunk, and some of those
    blocks still carry more than 256 records: several chunks under pruning.  (The first levels run k_tri_eval<16> over 2176.)"""
    name = "two_sheets"
    with sb.TriMesh.FromSoup(soup_of(name)) as m:
        R = m.records.copy()
        entries, lengths, tree = pruned_of(name, R, 6)
        assert len(lengths) == 7 and len(lengths[6]) >= 512 and lengths[6].max() > 256 and (lengths[6] > 256).sum() >= 64
        assert len(lengths[3]) < 512 and lengths[3].max() > 1024       # and the wide form walks more than one chunk of 1024
        od, st = m.Build(6, want_scene=False, want_octdata=True, want_stats=True)
    assert_tree(od, tree[:2], name)
    assert st.candidate_entries == entries


SCAN_PASS = 1024 * 256        # TRI_SCAN_CHUNK * TRI_SCAN_THREADS: the nodes k_tri_scan_chunks takes in one pass


def test_scan_carries_past_one_pass(sb):
    """The scans run over every level but the last, so the level that has to exceed one pass is one that SPLITS: the sphere mesh's
    level 8 under depth 9 (at depth 8 no scanned level of the sphere or the torus reaches 262 144 nodes)."""
    depth = 9
    with sb.TriMesh.FromSoup(soup_of("sphere")) as m:
        R = m.records.copy()
        od, st = m.Build(depth, want_scene=False, want_octdata=True, want_stats=True)
    S = od.Structs
    n = len(S)
    lvl, coord = mr.walk(S)                                     # (raises on a node that is not within its parent's block)
    count = np.bincount(lvl, minlength=depth + 1)
    first = np.concatenate([[0], np.cumsum(count)])
    assert st.levels == depth + 1 and count[depth - 1] > SCAN_PASS and (np.diff(lvl) >= 0).all()
    internal = S[:, 1] >= 0
    assert n == 1 + 8 * int(internal.sum()) and S[0, 0] == -1 and not internal[lvl == depth].any()
    for d in range(depth):
        at = np.nonzero(internal & (lvl == d))[0]
        # child blocks of eight in ascending parent index, one behind the other from the next level's first node
        assert (S[at, 1] == first[d + 1] + 8 * np.arange(len(at))).all(), d
        assert (S[first[d + 1]:first[d + 2], 0] == np.repeat(at, 8)).all(), d
    # seeded nodes against the restatement at their boxes: beyond one pass of the scan and before it, both split outcomes
    local = np.arange(n) - first[lvl]
    rng = np.random.default_rng(9)
    beyond = (lvl == depth - 1) & (local >= SCAN_PASS)
    pick = np.concatenate([rng.choice(np.nonzero(sel)[0], k, replace=False) for sel, k in
                           ((beyond & internal, 48), (beyond & ~internal, 48), ((lvl == depth - 1) & ~beyond, 32),
                            ((lvl == depth) & (local >= 8 * SCAN_PASS // 4), 64), (lvl < depth - 1, 64))])
    assert len(pick) == 256 and (local[pick] >= SCAN_PASS).sum() >= 64
    sibling = S[S[pick[:96], 0], 1]                             # the first sibling of those beyond the pass: their parents' blocks
    assert (sibling - first[depth - 1] >= SCAN_PASS - 7).all()
    for d in np.unique(lvl[pick]):
        nodes = pick[lvl[pick] == d]
        cv, mv = tr.node_values(R, coord[nodes], int(d))
        Sd = f32(2.0 ** -int(d))
        assert (tr.from_float(cv, Sd) == od.Values[nodes]).all(), d
        assert ((np.abs(mv) < f32(2) * Sd) & (d < depth) == internal[nodes]).all(), d


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

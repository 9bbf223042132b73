"""N1: point cloud -> ASDF.  CPU: the readers and the SdfGen oracle (the restatement of
SdfGen/dllmain.cpp) against the facts SURVEY.md recorded from a real SdfGen run.
GPU: the level-synchronous HIP builder against the oracle, byte for byte."""
import ctypes
import os
import re
import struct
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest


def fib_sphere(n, r=0.5, centre=(0.0, 0.0, 0.0)):
    i = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * i / n)
    th = np.pi * (1 + 5 ** 0.5) * i
    p = np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1)
    return np.concatenate([p * r + np.asarray(centre), p], 1).astype(np.float32)


def torus_cloud(n, R=0.6, r=0.2, seed=0):
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    nrm = np.stack([np.cos(u) * np.cos(v), np.sin(v), np.sin(u) * np.cos(v)], 1)
    pos = np.stack([np.cos(u) * R, np.zeros(n), np.sin(u) * R], 1) + nrm * r
    return np.concatenate([pos, nrm], 1).astype(np.float32)


def write_ply(path, verts, fmt="binary_little_endian"):
    with open(path, "wb") as f:
        f.write((f"ply\nformat {fmt} 1.0\ncomment made by tests\nelement vertex {len(verts)}\n"
                 "property float x\nproperty float y\nproperty float z\n"
                 "property float nx\nproperty float ny\nproperty float nz\nend_header\n").encode())
        f.write(np.ascontiguousarray(verts, dtype="<f4").tobytes())


def levels_of(structs):
    lvl = np.zeros(len(structs), dtype=np.int32)
    for i in range(len(structs)):
        c = structs[i, 1]
        if c >= 0:
            lvl[c:c + 8] = lvl[i] + 1
    return lvl


# ---- readers ------------------------------------------------------------------------------
def test_ply_reader(sb, tmp_path):
    v = fib_sphere(1234)
    p = tmp_path / "s.ply"
    write_ply(p, v)
    got = sb.OctData.LoadPly(str(p))
    assert got.shape == (1234, 6) and (got == v).all()
    for fmt in ("ascii", "binary_big_endian"):                     # refused, as in ply_reader.cpp:47-54
        write_ply(p, v, fmt)
        with pytest.raises(sb.SdfHipError):
            sb.OctData.LoadPly(str(p))
    p.write_bytes(b"plx\n")
    with pytest.raises(sb.SdfHipError):
        sb.OctData.LoadPly(str(p))
    write_ply(p, v)
    p.write_bytes(p.read_bytes()[:-100])                           # truncated payload
    with pytest.raises(sb.SdfHipError):
        sb.OctData.LoadPly(str(p))
    with pytest.raises(sb.SdfHipError):
        sb.OctData.LoadPly(str(tmp_path / "missing.ply"))


def test_obj_reader(sb, tmp_path):
    p = tmp_path / "m.obj"
    p.write_text("# a comment\no thing\nv 0 0 0\nv 1 0 0\nv 0 1 0\nv 0.5 0.5 1\nvt 0 0\nvn 0 0 1\nvn 1 0 0\ns off\n"
                 "f 1/1/1 2/1/1 3/1/1\nf 2//2 3//2\n")
    got = sb.OctData.LoadObj(str(p))
    assert got.shape == (4, 6)
    assert got[:, :3].tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0.5, 1]]
    # a face assigns its normals to its vertices (later faces win); unmentioned vertices keep (0,0,0)
    assert got[:, 3:].tolist() == [[0, 0, 1], [1, 0, 0], [1, 0, 0], [0, 0, 0]]
    p.write_text("v 0 0 0\nvn 0 0 1\nf 1/1/2\n")                   # normal index out of range
    with pytest.raises(sb.SdfHipError):
        sb.OctData.LoadObj(str(p))
    p.write_text("v 0 0 0\nq nonsense\n")
    with pytest.raises(sb.SdfHipError):
        sb.OctData.LoadObj(str(p))


# ---- the SdfGen oracle against the reference's recorded run -----------------------------------
def test_oracle_reproduces_the_survey_run(oracle_mod):
    # SURVEY.md / BASELINE.md: sphere point cloud r = 0.5 with normals, 20 000 points, depth 4,
    # real SdfGen: 4 529 nodes, 72 472-byte file, level histogram 1/8/64/512/3944
    o = oracle_mod.sdfgen(fib_sphere(20000), 4)
    assert len(o["structs"]) == 4529 and 8 + 16 * len(o["structs"]) == 72472
    assert np.bincount(levels_of(o["structs"])).tolist() == [1, 8, 64, 512, 3944]
    assert abs(o["scale"] - 1.1) < 1e-3 and all(abs(c - 0.003) < 1e-4 for c in o["offset"])
    # corner values are distances to the sphere in unit-cube units: check the root's
    s = o["scale"]
    for k in range(8):
        corner_model = (np.array([k % 2, 1 - (k // 2 % 2), k // 4 % 2]) - 0.5) * s + np.array(o["offset"])
        assert abs(o["float_values"][0, k] - (np.linalg.norm(corner_model) - 0.5) / s) < 0.02


def test_oracle_structure_and_inheritance(oracle_mod):
    o = oracle_mod.sdfgen(torus_cloud(6000), 5)
    s, fv = o["structs"], o["float_values"]
    assert s[0].tolist()[0] == -1
    internal = np.nonzero(s[:, 1] >= 0)[0]
    for i in internal[:300]:
        c = s[i, 1]
        assert (s[c:c + 8, 0] == i).all()
        for k in range(8):                      # child k inherits corner k (dllmain.cpp:181)
            assert fv[c + k, k] == fv[i, k]
    # the reference throws "Did not find" / "NaN distance" when no point can be the nearest one
    # (the pruning radius always keeps the nearest point, so that takes NaN input); the oracle
    # reports it as an error
    with pytest.raises(RuntimeError):
        oracle_mod.sdfgen(np.full((10, 6), np.nan, dtype=np.float32), 3)


# ---- the HIP builder -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["default", "sibling blocks everywhere"])
@pytest.mark.parametrize("cloud,depth", [("sphere20k", 4), ("sphere20k", 6), ("torus", 5), ("torus", 7), ("two", 5)])
def test_gpu_builder_equals_oracle(sb, oracle_mod, cloud, depth, form, monkeypatch):
    # two kernel forms per level: several 256-thread workgroups per node (levels of fewer than 16 384 nodes, or with long lists) and a
    # wavefront per block of eight siblings, their shared list staged through LDS (the others; the last level's centre and corner
    # searches fused); SDFHIP_GEN_WIDE=8 takes even the smallest levels below the root through the second
    if form != "default":                   # (a measurement knob: the laboratory library reads it, the product does not)
        import sdfbox_amd.lab
        sb = sdfbox_amd.lab.load()
        monkeypatch.setenv("SDFHIP_GEN_WIDE", "8")
    v = {"sphere20k": fib_sphere(20000), "torus": torus_cloud(30000),
         "two": np.concatenate([fib_sphere(4000, 0.3, (-0.2, 0.1, 0.0)), fib_sphere(3000, 0.25, (0.35, -0.1, 0.2))])}[cloud]
    o = oracle_mod.sdfgen(v, depth)
    od, st = sb.OctData.SdfGen(v, depth, want_stats=True)
    assert od.Length == len(o["structs"]) == st.nodes
    assert (od.Structs == o["structs"]).all()
    assert (od.Values == o["values"]).all()
    assert st.global_scale == np.float32(o["scale"]) and tuple(st.global_offset) == tuple(np.float32(c) for c in o["offset"])
    assert od.validate() == (int(levels_of(od.Structs).max()), True)


# Exact ties.  Every search of the builder keeps the reference's strict `<` scan: of equal distances the earliest list position
# wins (the segments' 64-bit atomic minima of {distance bits, position}, the sub_min shuffles and the sibling-block butterfly).
# Only exact duplicates tie bit for bit after the cloud's transform, so every point gets a copy with the OPPOSITE normal: the
# sign of a corner value comes from the winner's normal, and a builder that picked another of the tied points would change the
# bytes.  Orders: the copies far behind the originals (the tie crosses 1 024-entry segments and 256-entry LDS chunks), the two
# interleaved (one wavefront), three copies, and a random choice per point of which copy comes first (the two blocks far apart).
TIE_ORDERS = ("behind", "interleaved", "triplicates", "mixed")


def tie_cloud(base, order, swapped=False):
    a, b = base, base.copy()
    b[:, 3:] *= -1
    if swapped:
        a, b = b, a
    if order == "behind":
        return np.concatenate([a, b])
    if order == "interleaved":
        return np.stack([a, b], 1).reshape(-1, 6)
    if order == "triplicates":
        return np.concatenate([a, b, a])
    first = np.random.default_rng(len(base)).random(len(base)) < 0.5
    return np.concatenate([np.where(first[:, None], a, b), np.where(first[:, None], b, a)])


_tie_refs = {}


def tie_reference(oracle_mod, cloud, order, swapped, depth):
    # (the oracle's trees, shared by both flavours of the library)
    key = (cloud, order, swapped, depth)
    if key not in _tie_refs:
        base = {"sphere": fib_sphere(6000), "torus": torus_cloud(8000)}[cloud]
        v = tie_cloud(base, order, swapped)
        _tie_refs[key] = (v, oracle_mod.sdfgen(v, depth))
    return _tie_refs[key]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["default", "sibling blocks everywhere"])
@pytest.mark.parametrize("cloud", ["sphere", "torus"])
def test_gpu_builder_breaks_exact_ties_like_the_oracle(sb, oracle_mod, cloud, form, monkeypatch):
    # lists of 12 000 - 24 000 entries at the root: the segment kernels take them in 12 - 24 segments (default form), and the
    # sibling-block kernels in chunks of 256 from level 1 on (SDFHIP_GEN_WIDE=8, the laboratory library)
    if form != "default":
        import sdfbox_amd.lab
        sb = sdfbox_amd.lab.load()
        monkeypatch.setenv("SDFHIP_GEN_WIDE", "8")
    for depth in (4, 5, 6, 7):
        for order in TIE_ORDERS:
            for swapped in (False, True):
                v, o = tie_reference(oracle_mod, cloud, order, swapped, depth)
                what = f"{cloud} depth {depth}, copies {order}{', swapped' if swapped else ''}"
                od, st = sb.OctData.SdfGen(v, depth, want_stats=True)
                assert od.Length == len(o["structs"]) == st.nodes, what
                assert (od.Structs == o["structs"]).all(), what
                assert (od.Values == o["values"]).all(), f"{what}: {int((od.Values != o['values']).sum())} value bytes differ"
                assert st.global_scale == np.float32(o["scale"]), what
                assert tuple(st.global_offset) == tuple(np.float32(c) for c in o["offset"]), what
            # not vacuous: which of the tied points wins decides the bytes
            a, b = tie_reference(oracle_mod, cloud, order, False, depth)[1], tie_reference(oracle_mod, cloud, order, True, depth)[1]
            assert (a["structs"] == b["structs"]).all() and (a["values"] != b["values"]).mean() > 0.5, f"{cloud} depth {depth} {order}"


@pytest.mark.gpu
def test_builder_gives_its_pool_back(sb):
    # the builder keeps its work arrays' device memory for the next build; sdfhip_sdfgen_trim returns it, and the next build is the same
    import torch
    v = fib_sphere(20000)
    a = sb.OctData.SdfGen(v, 6)
    held = torch.cuda.mem_get_info()[0]
    sb.sdfgen_trim()
    assert torch.cuda.mem_get_info()[0] >= held + (64 << 20)
    sb.sdfgen_trim()                                     # (nothing left: still fine)
    b = sb.OctData.SdfGen(v, 6)
    assert (a.Structs == b.Structs).all() and (a.Values == b.Values).all()


@pytest.mark.gpu
def test_gpu_builder_end_to_end(sb, oracle_mod, tmp_path):
    # .ply -> SdfGen on the GPU -> .asdf -> render: the whole of Logic.MakeData + Program.Draw
    v = fib_sphere(20000)
    ply = tmp_path / "sphere.ply"
    write_ply(ply, v)
    od = sb.OctData.SdfGen(sb.OctData.LoadPly(str(ply)), 5)
    od.Save(str(tmp_path / "sphere.asdf"))
    back = sb.OctData.LoadAsdf(str(tmp_path / "sphere.asdf"))
    cam = sb.Logic(96, 96)
    ref, _ = oracle_mod.render(back.Structs, back.Values, cam.State, 96, 96, nthreads=8)
    with sb.Scene(back) as sc:
        img = sc.Draw(cam, 96, 96)
    same = (img.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(img) & np.isnan(ref))
    assert same.all()
    assert (img[..., 0] > 0.0051).sum() > 500                 # the sphere is there and lit
    with pytest.raises(sb.SdfHipError):                      # no usable point: an error code, not a crash
        sb.OctData.SdfGen(np.full((10, 6), np.nan, dtype=np.float32), 3)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [9, 10])
def test_mesh_scale_import_and_render(sb, oracle_mod, tmp_path, depth):
    # The reference's mesh flow at dragon scale (Program.cs:613-650, Model.MaxDepth = 10): a 1 M-point .ply ->
    # LoadPly -> SdfGen on the GPU -> Save -> LoadAsdf -> 1080p render, checked against the oracle on sampled rows
    # (the builder's bytes for this cloud are held to the oracle's at depth 10 in test_gpu_builder_mesh_scene_equals_oracle below;
    # here the GPU's own tree goes through the file and the renderer)
    W, H = 1920, 1080
    ply = tmp_path / "knot.ply"
    sb.write_ply(str(ply), sb.knot_point_cloud(1_000_000))
    pts = sb.OctData.LoadPly(str(ply))
    assert pts.shape == (1_000_000, 6)
    od, st = sb.OctData.SdfGen(pts, depth, want_stats=True)
    assert od.validate() == (depth, True) and st.nodes == od.Length > (2_000_000 if depth == 9 else 8_000_000)
    od.Save(str(tmp_path / "knot.asdf"))
    back = sb.OctData.LoadAsdf(str(tmp_path / "knot.asdf"))
    assert (back.Structs == od.Structs).all() and (back.Values == od.Values).all()
    cam = sb.Logic(W, H); cam.Position = (0.5, 0.5, -0.35); cam.Heading = (-0.2, 0.35)
    with sb.Scene(back) as sc:
        assert sc.stack_kernel_ok and sc.depth == depth and sc.top_grid_level > 0
        img, stt = sc.Draw(cam, W, H, sb.FLAG_COUNT, want_stats=True)
        img2 = sc.Draw(cam, W, H, sb.KERNEL_GENERIC)          # the shader's own traversal, and the compaction kernel, beside the default
        img3 = sc.Draw(cam, W, H, sb.FLAG_COMPACT)
    assert ((img.view(np.uint32) == img2.view(np.uint32)) | (np.isnan(img) & np.isnan(img2))).all()
    assert ((img.view(np.uint32) == img3.view(np.uint32)) | (np.isnan(img) & np.isnan(img3))).all()
    assert int(img[..., 3].astype(np.float64).sum()) == stt.n_steps
    hit = img[..., 2] != np.float32(0.2)
    assert 0.05 < hit.mean() < 0.6 and (img[..., 0][hit] > 0).sum() > 10000        # the knot is there and lit
    rows = list(range(3, H, 41))
    ref, cnt = oracle_mod.render(back.Structs, back.Values, cam.State, W, H, row0=3, nrows=len(rows), row_step=41, nthreads=16)
    got = img[rows]
    assert ((got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))).all()


@pytest.mark.gpu
def test_points_to_scene_without_leaving_the_device(sb):
    # sdfhip_sdfgen_scene (the viewer's generate -> upload flow in one call): the handle it returns renders what
    # sdfhip_sdfgen + sdfhip_scene_upload render, and the host copy it can also return is the same tree, byte for byte
    from conftest import assert_frames_identical, make_camera
    v = torus_cloud(60_000)
    for depth in (5, 8):
        od = sb.OctData.SdfGen(v, depth)
        sc, od2, st = sb.Scene.FromPoints(v, depth, want_octdata=True, want_stats=True)
        try:
            assert st.nodes == od.Length == sc.Length and sc.depth == depth
            assert (od2.Structs == od.Structs).all() and (od2.Values == od.Values).all()
            with sb.Scene(od) as ref:
                assert (sc.top_grid_level, sc.top_grid_bytes) == (ref.top_grid_level, ref.top_grid_bytes)
                for cname, (W, H) in (("default", (160, 120)), ("rotated", (200, 96)), ("closeup", (64, 64))):
                    cam = make_camera(cname, W, H)
                    assert_frames_identical(sc.Draw(cam, W, H), ref.Draw(cam, W, H), f"depth {depth} {cname}")
                    assert_frames_identical(sc.Draw(cam, W, H, sb.KERNEL_GENERIC), ref.Draw(cam, W, H), f"depth {depth} {cname}, generic kernel")
        finally:
            sc.close()
        only = sb.Scene.FromPoints(v, depth)                     # without the host copy
        try:
            cam = make_camera("rotated", 96, 96)
            with sb.Scene(od) as ref:
                assert_frames_identical(only.Draw(cam, 96, 96), ref.Draw(cam, 96, 96), "no host copy")
        finally:
            only.close()
    with pytest.raises(sb.SdfHipError):
        sb.Scene.FromPoints(np.full((10, 6), np.nan, np.float32), 3)


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", ["product", "lab"])
def test_builder_scene_agrees_with_the_uploaded_tree_on_edge_clouds(flavour, oracle_mod):
    # sdfhip_sdfgen_scene hands its own tree to the scene without validating it again (the product; the laboratory
    # library validates it and refuses a verdict that differs from the builder's word).  On the clouds where a builder could
    # stop early or build a single node, the scene it makes must be the scene an upload of the same tree makes: depth, kernel
    # choice, grid, pixels -- or both ways must fail.
    from conftest import assert_frames_identical, make_camera
    if flavour == "lab":
        import sdfbox_amd.lab
        sb = sdfbox_amd.lab.load()
    else:
        import sdfbox_amd as sb
    one = np.array([[0.1, 0.2, 0.3, 0.0, 0.0, 1.0]], np.float32)
    opposite = np.repeat(one, 2, 0)
    opposite[1, 3:] *= -1                                   # an exact tie whose winner decides the signs: the first point must win
    cases = {"one point": (one, 3), "two coincident points": (np.repeat(one, 2, 0), 4),
             "two coincident points, opposite normals": (opposite, 4), "two coincident points, opposite normals, the other first": (opposite[::-1].copy(), 4),
             "eight points, depth 10": (fib_sphere(8), 10), "depth 0: the root alone": (fib_sphere(500), 0),
             "depth 1": (fib_sphere(500), 1), "a flat cloud (one plane)": (np.concatenate([fib_sphere(300)[:, :2], np.zeros((300, 1), np.float32),
                                                                           np.tile(np.float32([0, 0, 1]), (300, 1))], 1), 6)}
    for name, (v, depth) in cases.items():
        if "coincident" in name:                            # ... and these trees are the oracle's, byte for byte
            o = oracle_mod.sdfgen(v, depth)
            od = sb.OctData.SdfGen(v, depth)
            assert (od.Structs == o["structs"]).all() and (od.Values == o["values"]).all(), name
        try:
            od = sb.OctData.SdfGen(v, depth)
        except sb.SdfHipError:
            with pytest.raises(sb.SdfHipError):
                sb.Scene.FromPoints(v, depth)
            continue
        sc = sb.Scene.FromPoints(v, depth)
        try:
            with sb.Scene(od) as ref:
                assert (sc.Length, sc.depth, sc.stack_kernel_ok) == (ref.Length, ref.depth, ref.stack_kernel_ok), name
                assert (sc.top_grid_level, sc.top_grid_bytes) == (ref.top_grid_level, ref.top_grid_bytes), name
                assert od.validate() == (sc.depth, True), name
                cam = make_camera("rotated", 96, 64)
                assert_frames_identical(sc.Draw(cam, 96, 64), ref.Draw(cam, 96, 64), name)
        finally:
            sc.close()


# ---- the builder against the oracle at every depth, kernel form and edge cloud ------------------------------------------------
# Every check below holds both entry points (sdfhip_sdfgen, and sdfhip_sdfgen_scene with its host copy) to the oracle's tree:
# {parent, children} records, corner bytes, node count, global scale and offset, the number of levels, and a scene whose depth
# and kernel choice are those of an upload of the oracle's tree -- or, where the oracle fails (code 2, the reference throws), an
# error from both and no scene.  The oracle's trees are built once per session, several at a time (ctypes lets go of the GIL).
_oracle_pool = None
_oracle_trees = {}          # (cloud name, depth) -> Future of the oracle's tree


def level_counts(structs):
    """Nodes per level of a tree in the reference's layout, a level at a time (not a Python loop over 12 M nodes)."""
    counts, frontier = [1], np.zeros(1, np.int64)
    while True:
        first = structs[frontier, 1]
        first = first[first >= 0].astype(np.int64)
        if not len(first):
            return counts
        frontier = (first[:, None] + np.arange(8)).ravel()
        counts.append(len(frontier))


def _oracle_build(oracle_mod, v, depth, keep_floats):
    t0 = time.perf_counter()
    try:
        o = oracle_mod.sdfgen(v, depth)
    except RuntimeError as e:
        return {"error": str(e), "seconds": time.perf_counter() - t0}
    if not keep_floats:
        del o["float_values"]
    o["level_counts"] = level_counts(o["structs"])
    o["seconds"] = time.perf_counter() - t0
    return o


def oracle_submit(oracle_mod, key, v, keep_floats=False):
    global _oracle_pool
    if key not in _oracle_trees:
        if _oracle_pool is None:
            oracle_mod.lib()                                  # (bound once, before the threads)
            _oracle_pool = ThreadPoolExecutor(min(16, os.cpu_count() or 1))
        _oracle_trees[key] = _oracle_pool.submit(_oracle_build, oracle_mod, np.ascontiguousarray(v, np.float32), key[1], keep_floats)
    return _oracle_trees[key]


def oracle_tree(oracle_mod, key, v, keep_floats=False):
    return oracle_submit(oracle_mod, key, v, keep_floats).result()


_clouds = {}


def cloud(name):
    """sphere<n>, torus<n>, knot<n>: fib_sphere(n), torus_cloud(n), knot_point_cloud(n)."""
    if name not in _clouds:
        kind, n = re.fullmatch(r"([a-z]+)(\d+)", name).groups()
        if kind == "knot":
            import sdfbox_amd
            _clouds[name] = sdfbox_amd.knot_point_cloud(int(n))
        else:
            _clouds[name] = {"sphere": fib_sphere, "torus": torus_cloud}[kind](int(n))
    return _clouds[name]


def f32_bits(x):
    return np.float32(x).view(np.uint32)


def assert_tree_is_the_oracles(od, st, o, what):
    assert od.Length == st.nodes == len(o["structs"]), f"{what}: {od.Length} / {st.nodes} nodes, the oracle's {len(o['structs'])}"
    assert (od.Structs == o["structs"]).all(), f"{what}: {int((od.Structs != o['structs']).any(1).sum())} records differ"
    bad = od.Values != o["values"]
    assert not bad.any(), f"{what}: {int(bad.sum())} corner bytes differ, in {int(bad.any(1).sum())} nodes"
    assert st.levels == len(o["level_counts"]), f"{what}: {st.levels} levels, the oracle's tree {len(o['level_counts'])}"
    assert f32_bits(st.global_scale) == f32_bits(o["scale"]), f"{what}: global scale {st.global_scale} against {o['scale']}"
    assert [f32_bits(c) for c in st.global_offset] == [f32_bits(c) for c in o["offset"]], what


def assert_both_entry_points_fail(sb, v, depth, what):
    with pytest.raises(sb.SdfHipError):
        sb.OctData.SdfGen(v, depth)
    with pytest.raises(sb.SdfHipError):
        sb.Scene.FromPoints(v, depth)
    # ... and the scene entry point leaves no handle and no host tree behind (the handle starts out non-null on purpose)
    v = np.ascontiguousarray(v, np.float32)
    h, raw = ctypes.c_void_p(0x5DF), sb._lib.COctData()
    raw.length = 7
    rc = sb._lib.lib.sdfhip_sdfgen_scene(0, v.ctypes.data, len(v), int(depth), ctypes.byref(h), ctypes.byref(raw), None)
    assert rc != sb._lib.OK and not h.value and raw.length == 0 and not raw.structs and not raw.values, what


LEVEL_LINE = re.compile(r"sdfgen: level\s+(\d+):\s+(\d+) nodes,\s+(\d+) entries kept")


def level_lines(text):
    """SDFHIP_GEN_LEVELS=1 (laboratory library): -> [(level, nodes, list entries kept for the next level)]."""
    return [tuple(int(g) for g in m.groups()) for m in LEVEL_LINE.finditer(text)]


def assert_builder_is_the_oracle(sb, v, depth, o, what, capfd=None):
    """Both entry points against the oracle's tree o.  capfd (the laboratory library under SDFHIP_GEN_LEVELS=1): -> the level lines."""
    if "error" in o:
        assert "code 2" in o["error"], o["error"]
        assert_both_entry_points_fail(sb, v, depth, what)
        return None
    if capfd is not None:
        capfd.readouterr()
    od, st = sb.OctData.SdfGen(v, depth, want_stats=True)
    lines = level_lines(capfd.readouterr().err) if capfd is not None else None
    assert_tree_is_the_oracles(od, st, o, what)
    del od
    sc, od2, st2 = sb.Scene.FromPoints(v, depth, want_octdata=True, want_stats=True)
    try:
        if capfd is not None:
            assert level_lines(capfd.readouterr().err) == lines, f"{what}: the scene entry point built other levels"
        assert_tree_is_the_oracles(od2, st2, o, f"{what}, scene entry point")
        del od2
        with sb.Scene(sb.OctData(o["structs"], o["values"])) as ref:
            assert (sc.Length, sc.depth, sc.stack_kernel_ok, sc.top_grid_level) == \
                   (ref.Length, ref.depth, ref.stack_kernel_ok, ref.top_grid_level), f"{what}: the scene is not an upload of the oracle's tree"
    finally:
        sc.close()
    return lines


def flavour_lib(flavour):
    import sdfbox_amd
    if flavour == "product":
        return sdfbox_amd
    import sdfbox_amd.lab
    return sdfbox_amd.lab.load()


# 1. Deep byte parity.  (Oracle, one core: 1.5 s for the 3 000-point sphere at depth 11, 9 s for the 200 k-point knot at depth 8.)
DEEP = [("sphere3000", 8), ("sphere3000", 9), ("sphere3000", 11), ("sphere3000", 12), ("sphere200", 12), ("sphere8", 12),
        ("sphere20000", 8), ("torus30000", 8), ("knot200000", 7), ("knot200000", 8), ("knot200000", 9)]
MESH = ("knot1000000", 10)      # bench_configs.py's mesh scene (cfg2_mesh_knot_d10): 12 M nodes, 80 - 90 s of the oracle
_level_log = {}                 # (cloud, depth) -> the level lines of its laboratory build without a knob


def prefetch_deep(oracle_mod):
    for key in [MESH] + DEEP:                                # (the longest first: the others are built beside it)
        oracle_submit(oracle_mod, key, cloud(key[0]))


def deep_case(flavour, key, oracle_mod, capfd, monkeypatch):
    sb = flavour_lib(flavour)
    prefetch_deep(oracle_mod)
    if flavour == "lab":
        monkeypatch.setenv("SDFHIP_GEN_LEVELS", "1")        # (prints the levels; changes nothing the kernels do)
    o = oracle_tree(oracle_mod, key, cloud(key[0]))
    lines = assert_builder_is_the_oracle(sb, cloud(key[0]), key[1], o, f"{flavour}: {key[0]} at depth {key[1]}",
                                         capfd if flavour == "lab" else None)
    if flavour == "lab":
        assert [n for _, n, _ in lines] == o["level_counts"], f"{key}: the builder's levels are not the oracle's"
        _level_log[key] = lines


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", ["product", "lab"])
@pytest.mark.parametrize("name,depth", DEEP)
def test_gpu_builder_equals_oracle_deep(oracle_mod, name, depth, flavour, capfd, monkeypatch):
    deep_case(flavour, (name, depth), oracle_mod, capfd, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", ["product", "lab"])
def test_gpu_builder_mesh_scene_equals_oracle(oracle_mod, flavour, capfd, monkeypatch):
    # the 1 M-point knot at depth 10, built through sdfhip_sdfgen_scene as bench.py's mesh scene is (and through sdfhip_sdfgen)
    deep_case(flavour, MESH, oracle_mod, capfd, monkeypatch)


# 2. Which kernel form every level took: a mirror of the rule in sdfgen_impl, applied to the SDFHIP_GEN_LEVELS lines.
WIDE_LEVEL, WIDE_MAX_LIST, PIPE_MIN_LIST, SCAN_ONE_PASS = 16384, 8192, 512, 1 << 20


def builder_forms(lines, n_points, depth):
    """-> [(level, set of form names)] for a build of n_points to `depth` whose level lines are `lines`."""
    out, entries = [], n_points
    for lvl, n, kept in lines:
        last = lvl >= depth
        avg = entries // (n // 8) if n >= 8 else entries
        big = n >= WIDE_LEVEL and lvl >= 1 and n % 8 == 0
        wide = big and avg <= WIDE_MAX_LIST
        pipe = wide and avg > PIPE_MIN_LIST
        fused = wide and not pipe and last
        forms = set()
        if lvl == 0:
            forms.add("root")
        elif not wide:
            forms.add("segments on the last level" if last else "segments below the root")
            if big:
                forms.add("segments on a wide level (long lists)")
        elif pipe:
            forms.add("pipe on the last level" if last else "pipe, not on the last level")
        elif fused:
            forms.add("fused")
        else:
            forms.add("sibling blocks without pipe")
        if n > SCAN_ONE_PASS:
            forms.add(f"a level of more than {SCAN_ONE_PASS} nodes")
        out.append((lvl, forms))
        entries = kept
    return out


ALL_FORMS = ("root", "segments below the root", "segments on the last level", "segments on a wide level (long lists)",
             "sibling blocks without pipe", "pipe, not on the last level", "pipe on the last level", "fused",
             f"a level of more than {SCAN_ONE_PASS} nodes")


def test_level_counts_is_levels_of(oracle_mod):
    o = oracle_mod.sdfgen(torus_cloud(6000), 5)
    assert level_counts(o["structs"]) == np.bincount(levels_of(o["structs"])).tolist()


def test_builder_form_mirror():
    # the mirror itself, on made-up lines: (level, nodes, entries kept for the next level); a level's mean list length comes
    # from the line before it
    lines = [(0, 1, 1000), (1, 8, 2048 * 8193), (2, 16384, 2048 * 513), (3, 16384, 2048 * 512), (4, 16384, 2048 * 600),
             (5, 16384, 100), (6, 2 * SCAN_ONE_PASS, 0)]
    assert [sorted(f) for _, f in builder_forms(lines, 5000, 6)] == [
        ["root"], ["segments below the root"], ["segments below the root", "segments on a wide level (long lists)"],
        ["pipe, not on the last level"], ["sibling blocks without pipe"], ["pipe, not on the last level"],
        ["a level of more than 1048576 nodes", "fused"]]
    assert [sorted(f) for _, f in builder_forms([(0, 1, 99), (1, 8, 2048 * 600), (2, 16384, 0)], 99, 2)] == \
           [["root"], ["segments below the root"], ["pipe on the last level"]]
    assert [sorted(f) for _, f in builder_forms([(0, 1, 99), (1, 8, 0)], 99, 1)] == [["root"], ["segments on the last level"]]
    # a tree that stops before its depth: its deepest level is not the last one the builder plans for
    assert [sorted(f) for _, f in builder_forms([(0, 1, 99), (1, 16384, 0)], 99, 3)] == [["root"], ["sibling blocks without pipe"]]


@pytest.mark.gpu
def test_gpu_builder_runs_reach_every_form(oracle_mod, capfd, monkeypatch):
    # proven from the laboratory library's level lines, not assumed: the runs above (no knob) take every form of sdfgen_impl
    reached = {}
    for key in DEEP + [MESH]:
        if key not in _level_log:                            # (this test alone: build the laboratory runs again)
            deep_case("lab", key, oracle_mod, capfd, monkeypatch)
        for lvl, forms in builder_forms(_level_log[key], len(cloud(key[0])), key[1]):
            for f in forms:
                reached.setdefault(f, []).append(f"{key[0]} depth {key[1]} level {lvl}")
    report = "\n".join(f"  {f}: {', '.join(reached.get(f, ['NOT REACHED'])[:3])}" for f in ALL_FORMS)
    trees = [f.result() for f in _oracle_trees.values() if f.done()]
    print(f"\nbuilder forms reached:\n{report}\noracle: {len(trees)} trees, {sum(t['seconds'] for t in trees):.1f} s")
    assert set(ALL_FORMS) <= set(reached), report


# 3. The laboratory's knobs: segments per node, and the node count from which sibling blocks take a level.
@pytest.mark.gpu
@pytest.mark.parametrize("knob,value,name,depth", [("SDFHIP_GEN_SEGS", s, "torus30000", 7) for s in ("1", "3", "4096", "1048576")] +
                                                  [("SDFHIP_GEN_WIDE", w, "knot200000", 8) for w in ("8", "64", "4096")])
def test_gpu_builder_knobs_keep_the_bytes(oracle_mod, knob, value, name, depth, monkeypatch):
    sb = flavour_lib("lab")
    o = oracle_tree(oracle_mod, (name, depth), cloud(name))
    monkeypatch.setenv(knob, value)
    assert_builder_is_the_oracle(sb, cloud(name), depth, o, f"{knob}={value}: {name} at depth {depth}")


# 4. List-length boundaries: the root's list is the whole cloud -- 1 024-entry trips, 256-entry LDS chunks, the 512 pipe threshold.
BOUNDARY_POINTS = (1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049, 4097)
BUILDER_FORMS = {"product": ("product", {}), "lab": ("lab", {}), "lab, sibling blocks from 8 nodes": ("lab", {"SDFHIP_GEN_WIDE": "8"}),
                 "lab, one segment per node": ("lab", {"SDFHIP_GEN_SEGS": "1"})}


def boundary_cases():
    return [(f"sphere{n}", cloud(f"sphere{n}"), 6) for n in BOUNDARY_POINTS]


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(BUILDER_FORMS))
def test_gpu_builder_list_length_boundaries(oracle_mod, form, monkeypatch):
    flavour, env = BUILDER_FORMS[form]
    sb = flavour_lib(flavour)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cases = boundary_cases()
    for name, v, depth in cases:
        oracle_submit(oracle_mod, (name, depth), v)
    for name, v, depth in cases:
        assert_builder_is_the_oracle(sb, v, depth, oracle_tree(oracle_mod, (name, depth), v), f"{form}: {name} at depth {depth}")


# 5. Edge clouds.
def write_obj_without_some_normals(path, v, unreferenced):
    """An .obj whose faces name every vertex except those in `unreferenced`: the reader leaves those with the normal (0,0,0)."""
    named = [i for i in range(len(v)) if not unreferenced[i]]
    with open(path, "w") as f:
        f.writelines(f"v {x!r} {y!r} {z!r}\n" for x, y, z in v[:, :3].tolist())
        f.writelines(f"vn {x!r} {y!r} {z!r}\n" for x, y, z in v[:, 3:].tolist())
        f.writelines("f " + " ".join(f"{i + 1}//{i + 1}" for i in named[k:k + 3]) + "\n" for k in range(0, len(named), 3))


def tiny_normals(v):
    # normals whose squared length underflows to 0 in fp32: the near-surface branch divides by a zero length, +-inf corners
    v = v.copy()
    v[:, 3:] = np.sign(v[:, 3:]) * np.float32(1e-25)
    return v


def edge_clouds(sb, tmp_path):
    """-> [(name, points, depth)].  The .obj clouds are read back through `sb`'s reader."""
    one = np.array([[0.1, 0.2, 0.3, 0.0, 0.0, 1.0]], np.float32)
    rng = np.random.default_rng(5)
    x = np.linspace(-0.5, 0.5, 400)
    a = np.linspace(0, 8 * np.pi, 400)
    line = np.stack([x, np.zeros(400), np.zeros(400), np.zeros(400), np.cos(a), np.sin(a)], 1).astype(np.float32)
    flat = np.concatenate([fib_sphere(300)[:, :2], np.zeros((300, 1), np.float32), np.tile(np.float32([0, 0, 1]), (300, 1))], 1)
    # a box of 1.0 x 0.3 x 0.05, points on its faces with the faces' outward normals
    half = np.array([0.5, 0.15, 0.025])
    face = rng.integers(0, 6, 6000)
    axis, sign = face // 2, np.where(face % 2, 1.0, -1.0)
    box_p = rng.uniform(-1, 1, (6000, 3)) * half
    box_p[np.arange(6000), axis] = sign * half[axis]
    box_n = np.zeros((6000, 3))
    box_n[np.arange(6000), axis] = sign
    box = np.concatenate([box_p, box_n], 1).astype(np.float32)
    nonunit = fib_sphere(3000)
    nonunit[:, 3:] *= (10.0 ** rng.uniform(-3, 3, 3000)).astype(np.float32)[:, None]
    moved = fib_sphere(3000)
    moved[:, :3] += np.float32([1000, -2000, 3000])
    with_nan = fib_sphere(3000)
    with_nan[0, :3] = with_nan[-1, :3] = with_nan[::100, :3] = np.nan
    with_inf = fib_sphere(500)
    with_inf[7, 1] = np.inf
    cases = [("one point", one, 0), ("one point", one, 3), ("one point", one, 12),
             ("one point at (0.2, 0.2, 0.2): global scale 0", np.float32([[0.2, 0.2, 0.2, 0, 0, 1]]), 3),
             ("sphere500", cloud("sphere500"), 0), ("sphere500", cloud("sphere500"), 1),
             ("sphere8", cloud("sphere8"), 10), ("sphere8", cloud("sphere8"), 12),
             ("a flat cloud", flat, 8), ("a line", line, 9), ("sphere3000 at (1000, -2000, 3000)", moved, 8),
             ("sphere of radius 1e-4", fib_sphere(3000, 1e-4), 8), ("sphere of radius 1e4", fib_sphere(3000, 1e4), 8),
             ("a box of 1.0 x 0.3 x 0.05", box, 7), ("normals of length 1e-3 .. 1e3", nonunit, 7),
             ("NaN positions (first, last, every 100th)", with_nan, 7), ("a point at y = inf", with_inf, 5)]
    for what, every, depth in (("every third normal zero (.obj)", 3, 6), ("every normal zero (.obj)", 1, 7)):
        path = tmp_path / f"zero{every}.obj"
        base = fib_sphere(5000)
        write_obj_without_some_normals(path, base, np.arange(5000) % every == 0)
        v = sb.OctData.LoadObj(str(path))
        assert (v[:, :3] == base[:, :3]).all() and ((v[:, 3:] == 0).all(1) == (np.arange(5000) % every == 0)).all(), what
        cases.append((what, v, depth))
    return cases


def inherited_infinities(o):
    """-> (corners a child inherited as +inf, those of them the oracle recomputed to another value)"""
    s, fv = o["structs"], o["float_values"]
    c = np.arange(1, len(s))
    p = s[1:, 0]
    slot = c - s[p, 1]
    inherited = np.isposinf(fv[p, slot])
    return int(inherited.sum()), int((inherited & ~np.isposinf(fv[c, slot])).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", ["product", "lab"])
def test_gpu_builder_edge_clouds_equal_the_oracle(oracle_mod, flavour, tmp_path):
    sb = flavour_lib(flavour)
    cases = edge_clouds(sb, tmp_path)
    for name, v, depth in cases:
        oracle_submit(oracle_mod, (name, depth), v)
    for name, v, depth in cases:
        o = oracle_tree(oracle_mod, (name, depth), v)
        if name == "sphere of radius 1e-4":
            assert len(o["structs"]) == 1, "the root alone"
        if name.startswith("one point at (0.2") or name == "a point at y = inf":
            assert "error" in o, f"{name}: the oracle fails"
        assert_builder_is_the_oracle(sb, v, depth, o, f"{flavour}: {name} at depth {depth}")


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", ["product", "lab"])
@pytest.mark.parametrize("name", ["sphere5000", "torus8000"])
def test_gpu_builder_recomputes_inherited_infinite_corners(oracle_mod, flavour, name):
    # The reference recomputes every corner still at INFINITY (dllmain.cpp:171-172), so a child that inherits a +inf corner from
    # its parent recomputes it over its own, pruned, list; the builder must not copy the +inf down.
    sb = flavour_lib(flavour)
    v = tiny_normals(cloud(name))
    for depth in (5, 7):
        o = oracle_tree(oracle_mod, (f"{name}, normals of 1e-25", depth), v, keep_floats=True)
        inherited, recomputed = inherited_infinities(o)
        assert recomputed > 0, f"{name} at depth {depth}: {inherited} +inf corners inherited, none recomputed -- the case does not bite"
        assert_builder_is_the_oracle(sb, v, depth, o, f"{flavour}: {name} with normals of 1e-25 at depth {depth} "
                                                      f"({recomputed} inherited +inf corners recomputed by the oracle)")


# 6. Reuse: the pooled arena chunks and the page the scans report through, over builds of very different sizes in turn.
@pytest.mark.gpu
def test_gpu_builder_reuses_its_buffers_across_builds(oracle_mod, tmp_path, monkeypatch):
    import sdfbox_amd as sb
    cases = boundary_cases() + edge_clouds(sb, tmp_path) + [(f"{n}, normals of 1e-25", tiny_normals(cloud(n)), d)
                                                            for n in ("sphere5000", "torus8000") for d in (5, 7)]
    trees = [oracle_tree(oracle_mod, (name, depth), v, keep_floats="1e-25" in name) for name, v, depth in cases]
    size = [len(t["structs"]) if "error" not in t else 0 for t in trees]
    order = np.argsort(size, kind="stable")
    alternating = [int(order[i // 2] if i % 2 else order[len(order) - 1 - i // 2]) for i in range(len(order))]
    assert sorted(alternating) == list(range(len(cases)))
    monkeypatch.delenv("SDFHIP_GEN_POOL", raising=False)
    for step, i in enumerate(alternating):
        if step == len(alternating) // 2:
            sb.sdfgen_trim()
        name, v, depth = cases[i]
        assert_builder_is_the_oracle(sb, v, depth, trees[i], f"{name} at depth {depth}, build {step} of the process")
    monkeypatch.setenv("SDFHIP_GEN_POOL", "0")
    for i in alternating[::3]:
        name, v, depth = cases[i]
        assert_builder_is_the_oracle(sb, v, depth, trees[i], f"{name} at depth {depth}, without the pool")
    monkeypatch.delenv("SDFHIP_GEN_POOL")
    # a thread of its own gets a report page of its own, numbered from 0 again, beside this thread's
    for i in alternating[:2]:
        name, v, depth = cases[i]
        with ThreadPoolExecutor(1) as other:
            other.submit(assert_builder_is_the_oracle, sb, v, depth, trees[i], f"{name} at depth {depth}, another thread").result()

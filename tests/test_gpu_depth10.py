"""cfg-2 at the reference application's own depth (Model.MaxDepth = 10): the 141 M-node depth-10 stand-in that bench.py times as
cfg2_depth10, held to the oracle on every pixel.  It is the first scene whose fused node array (16 bytes a node) passes 2 GiB, the
first with two-level blocks under its split grid at scale (millions of blocks), and its path-traced bounce grid is the largest the
upload builds; the depth-9 scene of tests/test_gpu_parity.py reaches none of these."""
import numpy as np
import pytest

from conftest import assert_frames_identical, make_camera
from test_gpu_parity import assert_display_close

pytestmark = pytest.mark.gpu

DEPTH = 10
COARSE = 8                 # the split grid's coarse level at depth 10: blocks of the two levels below (bench key "grid8+blocks")
CELL = 16                  # bytes of a grid cell (TopCell)


@pytest.fixture(scope="module")
def d10(sb):
    od = sb.dragon_standin(DEPTH, nthreads=16)
    sc = sb.Scene(od)
    yield od, sc
    sc.close()


def bench_camera(sb, W, H):
    cam = sb.Logic(W, H)
    cam.Position = (0.5, 0.5, -0.35); cam.Heading = (-0.2, 0.35)          # cfg-2/3's camera
    return cam


def counters(st):
    return (st.n_nodes, st.n_samples, st.n_steps, st.n_shadow_rays)


def tree_levels(structs):
    """([the number of nodes with children at level 0, 1, ..., depth], [the highest-numbered such node of each level, or of the
    last level its highest-numbered leaf]) of a consistent tree: a cell of a grid level is internal (it holds a block of the finer
    levels) exactly where the tree has an internal node at that level."""
    counts, last = [], []
    level = np.zeros(1, dtype=np.int64)
    while len(level):
        kids = structs[level, 1]
        has = kids >= 0
        counts.append(int(has.sum()))
        last.append(int(level[has].max()) if has.any() else int(level.max()))
        level = (kids[has].astype(np.int64)[:, None] + np.arange(8)).reshape(-1)
    return counts, last


def grid_now(sb, sc):
    """(level, bytes) of sdfhip_scene_top_grid as they are now (Scene.top_grid_* are the upload's)"""
    import ctypes
    lvl, nb = ctypes.c_int32(), ctypes.c_uint64()
    sb._lib.check(sb._lib.lib.sdfhip_scene_top_grid(sc._h, ctypes.byref(lvl), ctypes.byref(nb)))
    return lvl.value, nb.value


def assert_split_grid_of_depth10(sc, internal):
    """The grid the bench line records for this scene: a dense level-8 grid, and under each of its internal cells a block of
    the 8^2 cells of levels 9 and 10 -- every byte of it accounted for, so that an upload that fell back to a plain grid (or
    a split at another level) fails here instead of passing on another path."""
    import bench_configs
    assert (sc.top_grid_level, bench_configs.grid_suffix(sc)) == (COARSE, f":grid{COARSE}+blocks"), \
        f"the upload built grid level {sc.top_grid_level} ({sc.top_grid_bytes} bytes), not a split grid at level {COARSE}"
    blocks = internal[COARSE]
    assert blocks > 1_000_000                       # millions of blocks: fine cells numbered into the hundreds of millions (id << 6)
    assert sc.top_grid_bytes == (CELL << (3 * COARSE)) + blocks * CELL * 8 ** (DEPTH - COARSE)


def bounce_grid_bytes(internal, FB):
    """sdfhip_scene_top_grid's growth when the path-traced mode builds its grid of 8^FB-cell blocks"""
    return (CELL << (3 * (DEPTH - FB))) + internal[DEPTH - FB] * CELL * 8 ** FB


@pytest.fixture(scope="module")
def levels(d10):
    return tree_levels(d10[0].Structs)


@pytest.fixture(scope="module")
def internal(levels):
    return levels[0]


def test_the_upload_of_the_depth10_scene(sb, d10, internal):
    od, sc = d10
    assert od.Length == sc.Length == 141_498_793 and od.Length * 16 > 2 << 30          # the fused records pass 2 GiB
    assert sc.depth == DEPTH and sc.stack_kernel_ok
    assert od.validate() == (DEPTH, True)
    assert len(internal) == DEPTH + 1 and internal[DEPTH] == 0 and sum(internal) * 8 + 1 == od.Length
    assert_split_grid_of_depth10(sc, internal)


def test_cfg2_at_depth10_equals_the_oracle_on_every_pixel(sb, oracle_mod, d10):
    # 1920x1080, the bench camera, all 2 073 600 pixels and the four counters: the default kernel (k_march through the split grid),
    # wavefront compaction, the shader's own traversal (reads the 2.26 GB node array during the frame), and the tile-order flag
    # (its second frame launches the tiles in the first one's cost order)
    od, sc = d10
    W, H = 1920, 1080
    cam = bench_camera(sb, W, H)
    ref, cnt = oracle_mod.render(od.Structs, od.Values, cam.State, W, H, nthreads=16)
    cnt = tuple(int(c) for c in cnt)
    for what, flags in (("default kernel", 0), ("FLAG_COMPACT", sb.FLAG_COMPACT), ("KERNEL_GENERIC", sb.KERNEL_GENERIC),
                        ("FLAG_TILE_ORDER", sb.FLAG_TILE_ORDER), ("FLAG_TILE_ORDER, second frame", sb.FLAG_TILE_ORDER)):
        img, st = sc.Draw(cam, W, H, flags | sb.FLAG_COUNT, want_stats=True)
        assert_frames_identical(img, ref, f"depth-10 cfg-2 frame, {what}")
        assert counters(st) == cnt, what
    assert_frames_identical(sc.Draw(cam, W, H), ref, "depth-10 cfg-2 frame, the timed (non-counting) kernel")


def test_cfg3_frame_at_depth10_equals_the_oracle_on_every_pixel(sb, oracle_mod, d10):
    # 3840x2160 (cfg-3's frame), all 8 294 400 pixels: the default kernel with its counters, and compaction
    od, sc = d10
    W, H = 3840, 2160
    cam = bench_camera(sb, W, H)
    ref, cnt = oracle_mod.render(od.Structs, od.Values, cam.State, W, H, nthreads=16)
    img, st = sc.Draw(cam, W, H, sb.FLAG_COUNT, want_stats=True)
    assert_frames_identical(img, ref, "depth-10 4K frame, default kernel")
    assert counters(st) == tuple(int(c) for c in cnt)
    assert_frames_identical(sc.Draw(cam, W, H, sb.FLAG_COMPACT), ref, "depth-10 4K frame, FLAG_COMPACT")


def test_camera_inside_the_object_and_the_display_pass(sb, oracle_mod, d10):
    # the close-up camera sits inside the ball, between the gyroid's sheets: short marches through the deepest cells and the
    # flat cells (all pixels, counters too); then the fused display pass of the same frame
    od, sc = d10
    W, H = 1920, 1080
    cam = make_camera("closeup", W, H)
    ref, cnt = oracle_mod.render(od.Structs, od.Values, cam.State, W, H, nthreads=16)
    for what, flags in (("default kernel", 0), ("FLAG_COMPACT", sb.FLAG_COMPACT), ("KERNEL_GENERIC", sb.KERNEL_GENERIC)):
        img, st = sc.Draw(cam, W, H, flags | sb.FLAG_COUNT, want_stats=True)
        assert_frames_identical(img, ref, f"depth-10 close-up, {what}")
        assert counters(st) == tuple(int(c) for c in cnt), what
    assert_display_close(sc.DrawDisplay(cam, W, H), oracle_mod.display(ref), "depth-10 close-up, display pass")
    assert (sc.DrawDisplay(cam, W, H, debug=True) == oracle_mod.display(ref, debug=True)).all(), "depth-10 close-up, heat map"


def test_path_traced_frame_at_depth10(sb, oracle_mod, d10, internal):
    # the bounce levels read a second split grid, built in front of the first path-traced frame: blocks of 16^3 cells under a
    # level-6 grid (6.6 GB here, of the 1/32 of the device's memory it may take; it would fall back to smaller blocks beyond)
    od, sc = d10
    W, H = 480, 270
    cam = bench_camera(sb, W, H)
    pt = sb.PathTrace(spp=2)
    ref, cnt = oracle_mod.render_pt(od.Structs, od.Values, cam.State, W, H, spp=pt.spp, max_bounces=pt.max_bounces, seed=pt.seed,
                                    albedo=pt.albedo, nthreads=16)
    own = grid_now(sb, sc)[1]
    for what, kernel in (("KERNEL_STACK", sb.KERNEL_STACK), ("KERNEL_GENERIC", sb.KERNEL_GENERIC)):
        img, st = sc.DrawPath(cam, W, H, pt, flags=kernel | sb.FLAG_COUNT, want_stats=True)
        assert_frames_identical(img, ref, f"depth-10 path-traced frame, {what}")
        assert counters(st) == tuple(int(c) for c in cnt), what
    level, after = grid_now(sb, sc)
    assert level == COARSE and after - own == bounce_grid_bytes(internal, 4), (after - own, bounce_grid_bytes(internal, 4))


def test_the_grid_arrays_a_frame_reads(d10, internal):
    # the laboratory's line-touch hook reports the sizes of the arrays a frame's lookups read: the split grid's blocks ("fine")
    # are there for the frame, and the bounce grid's ("fine2") for the bounce levels of a path-traced frame
    import sdfbox_amd.lab
    lab = sdfbox_amd.lab.load()
    od, _ = d10
    W, H = 320, 180
    with lab.Scene(od, device=0) as sc:
        assert_split_grid_of_depth10(sc, internal)
        sc.touch_begin()
        sc.Draw(bench_camera(lab, W, H), W, H, lab.FLAG_COUNT)
        ab = sc.touch_end()["array_bytes"]
        assert ab["coarse"] == CELL << (3 * COARSE) and ab["fine"] == internal[COARSE] * CELL * 64, ab
        sc.DrawPath(bench_camera(lab, W, H), W, H, lab.PathTrace(spp=4))      # (builds the bounce grid: touch_begin counts the grids that exist)
        sc.touch_begin()
        sc.DrawPath(bench_camera(lab, W, H), W, H, lab.PathTrace(spp=4), flags=lab.FLAG_COUNT)
        t = sc.touch_end()
        ab = t["array_bytes"]
        assert ab["coarse2"] == CELL << (3 * (DEPTH - 4)) and ab["coarse2"] + ab["fine2"] == bounce_grid_bytes(internal, 4), ab
        assert any(p["grid"] == "bounce" and p["fine_lines"] > 0 for p in t["phases"]), t["phases"]


@pytest.mark.parametrize("broken", ["children block past the end", "parent out of range"])
def test_upload_refuses_a_broken_deep_link(sb, d10, levels, broken):
    # the device validation (k_validate_*: pointer jumping over 141 M nodes) must refuse a tree with one bad link in its last
    # levels, as the host function does: SDFHIP_ERR_BAD_TREE
    od, _ = d10
    s = od.Structs.copy()
    N = len(s)
    if broken == "children block past the end":
        s[levels[1][DEPTH - 1], 1] = N - 3                # the last internal node of level 9: its block of eight would end past the array
    else:
        s[levels[1][DEPTH], 0] = N + 10                  # the last leaf of level 10 names a parent that does not exist
    tree = sb.OctData(s, od.Values)
    with pytest.raises(sb.SdfHipError) as host:
        tree.validate()
    with pytest.raises(sb.SdfHipError) as dev:
        sb.Scene(tree)
    assert host.value.code == dev.value.code == sb._lib.ERR_BAD_TREE

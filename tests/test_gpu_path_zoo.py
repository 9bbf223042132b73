"""The path-traced mode on the cases of tests/test_path_zoo.py, both flavours of the library: the pipeline of kernels over its hit queues
(k_pt_primary, k_pt_bounce per level, k_pt_resolve; the laboratory's k_pt_key / k_pt_scan / k_pt_scatter and k_pt_bounce_refill) and
the one-kernel k_path, where the queues are FULL: trees whose paths go on hitting through all 65 levels, blocks_2049 on which every
path hits at every level.  Every frame is oracle.render_pt's bit for bit, NaN equal to NaN, with its four counters, from the kernels
that count and from those that do not.  Every frame comes through the synchronous entry point at least once, which reports a hit
queue that overflowed (SDFHIP_ERR_NOMEM, raised as SdfHipError): that no case raises is the check that the queues' capacity covers
the worst case.  No overflow is provoked."""
import os

import numpy as np
import pytest

import test_path_zoo as pz
from conftest import assert_frames_identical
from test_path_zoo import DEEP, FULL, H0, SPP0, W0

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["product", "lab"])
def sb(request):
    import sdfbox_amd
    if request.param == "product":
        return sdfbox_amd
    import sdfbox_amd.lab
    return sdfbox_amd.lab.load()


def octdata(sb, name):
    s, v = pz.tree(name)
    return sb.OctData(s, v)


def depth_of(name):
    import edit_restatement as er
    return er.tree_depth(pz.tree(name)[0])


def counters(st):
    return (st.n_nodes, st.n_samples, st.n_steps, st.n_shadow_rays)


def kernels_of(sb, scene):
    return (sb.KERNEL_STACK, sb.KERNEL_GENERIC) if scene.stack_kernel_ok else (sb.KERNEL_AUTO, sb.KERNEL_GENERIC)


def draw(sb, scene, name, what, W=W0, H=H0, spp=SPP0, max_bounces=DEEP, seed=pz.DEFAULT_SEED, albedo=1.0, view=None, kernels=None):
    """The case through DrawPath with each kernel selector, counting and not: frame and counters are the oracle's.
    -> the statistics of the first selector's counting render"""
    ref, cnt = pz.reference(name, W, H, spp, max_bounces, seed, albedo, view)
    cam = pz.camera(view or pz.VIEW.get(name, "zoo"), W, H)
    pt = sb.PathTrace(spp=spp, max_bounces=max_bounces, seed=seed, albedo=albedo)
    first = None
    for kernel in kernels if kernels is not None else kernels_of(sb, scene):
        tag = f"{name} {W}x{H} spp {spp} bounces {max_bounces} seed {seed:#x} albedo {albedo!r}: {what}, kernel selector {kernel}"
        img, st = scene.DrawPath(cam, W, H, pt, flags=kernel | sb.FLAG_COUNT, want_stats=True)
        assert_frames_identical(img, ref, tag + ", counting")
        assert counters(st) == cnt, tag
        assert_frames_identical(scene.DrawPath(cam, W, H, pt, flags=kernel), ref, tag + ", not counting")
        first = first or st
    return first


def through_the_pipeline(scene, st):
    """a frame of the pipeline reports the entries its bounce levels took from the queues; k_path has no queue"""
    assert st.n_hits >= st.n_shadow_rays > 0
    return st


# ---- 1. every level, every tree --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pz.PATH_TREES)
def test_every_level_of_every_tree(sb, name):
    with sb.Scene(octdata(sb, name)) as scene:
        one_kernel = name in ("chain14", pz.BAD_PARENT)
        assert scene.stack_kernel_ok == (not one_kernel)
        st = draw(sb, scene, name, "the upload's own grid")
        if one_kernel or scene.top_grid_level < max(scene.depth, 1):  # k_path: the shader's traversal, or a cursor stack under a partial grid
            assert st.n_hits == 0 and (one_kernel or name in ("chain12", "leaf")), (name, scene.top_grid_level)
            assert (st.kernel_used & 0xF) == (sb.KERNEL_GENERIC if one_kernel else sb.KERNEL_STACK)
        else:
            through_the_pipeline(scene, st)
        if name == FULL:
            assert st.n_hits == W0 * H0 * SPP0 * (DEEP + 1) == st.n_shadow_rays


# ---- 2. frame and sample edges on the full-queue tree ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_scene(sb):
    with sb.Scene(octdata(sb, FULL)) as scene:
        yield scene


@pytest.mark.parametrize("size", pz.EDGE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frame_sample_and_seed_edges_on_full_queues(sb, full_scene, size):
    W, H = size
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    # a wave of k_pt_primary is a tile and pushes into ONE of the 64 sub-queues: with fewer tiles than sub-queues most stay empty
    assert tiles <= 9
    partial = 0
    for spp, mb, seed in pz.edge_cases(size):
        st = through_the_pipeline(full_scene, draw(sb, full_scene, FULL, "edges", W, H, spp, mb, seed, kernels=(sb.KERNEL_STACK,)))
        assert st.n_hits == W * H * spp * (mb + 1)                    # every path is in every level's queue
        # sub-queue fills that were all multiples of 64 would sum to one: otherwise some sub-queue's last chunk is partial
        partial += (st.n_hits // (mb + 1)) % 64 != 0
    assert (partial > 0) == (size != (8, 8)), size                    # (8 x 8: 64 pixels, every level IS whole chunks -- the other edge)
    draw(sb, full_scene, FULL, "edges, the one-kernel form", W, H, 3, DEEP, 0xFFFFFFFF, kernels=(sb.KERNEL_GENERIC,))


# ---- 3. albedo -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("albedo", [0.0, 1.0, -0.5, float("nan")], ids=repr)
def test_albedo_zero_one_negative_and_nan(sb, albedo):
    # the throughput is replayed (albedo multiplied level times onto 1), and an unlit vertex leaves +0 for the resolve to add: neither
    # may change a bit when the products are 0, alternate in sign or are NaN.  The ABI takes any float.
    with sb.Scene(octdata(sb, "dfs_d6_b")) as scene:
        through_the_pipeline(scene, draw(sb, scene, "dfs_d6_b", "hostile tree", albedo=albedo))
    with sb.Scene(octdata(sb, "torus_d6")) as scene:
        through_the_pipeline(scene, draw(sb, scene, "torus_d6", "torus", 40, 40, 3, 8, 7, albedo, view="closeup"))


# ---- 4. grids --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pz.tz.MESHABLE)
def test_behind_a_split_grid(sb, name):
    depth = depth_of(name)
    if depth < 2:                                                     # the leaf: no level to split at, the request falls back
        with sb.Scene(octdata(sb, name), top_grid_split=1) as scene:
            draw(sb, scene, name, "split grid asked of a leaf")
        return
    split = max(depth // 2, depth - 6)
    with sb.Scene(octdata(sb, name), top_grid_split=split) as scene:
        assert scene.stack_kernel_ok and scene.top_grid_level == split < depth
        st = through_the_pipeline(scene, draw(sb, scene, name, f"split grid, coarse level {split}"))
        if name == FULL:
            assert st.n_hits == W0 * H0 * SPP0 * (DEEP + 1)


@pytest.mark.parametrize("order", [1, 0])
@pytest.mark.parametrize("blocks", [0, 1, 2, 3, 4])
def test_through_every_scatter_grid(sb, blocks, order):
    # the bounce levels' second grid (blocks of `blocks` levels): a leaf and the depth-6 trees are shallower than a block of 4 + a coarse
    # level, chain12 has no full-depth grid of its own -- whatever the library falls back to, the frame is the oracle's
    for name, split in (("leaf", None), ("dfs_d6_a", None), ("dfs_d6_b", None), (FULL, None), ("chain12", None), ("chain12", 6)):
        with sb.Scene(octdata(sb, name), top_grid_split=split, scatter_grid=blocks, scatter_order=order) as scene:
            st = draw(sb, scene, name, f"scatter grid {blocks}, order {order}, split {split}", kernels=(sb.KERNEL_STACK,))
            if name != "leaf" and (name != "chain12" or split):
                through_the_pipeline(scene, st)
            else:
                assert st.n_hits == 0                                 # k_path


# ---- 5. bands with padding rows --------------------------------------------------------------------------------------------------
BAND_W, BAND_SPP, BAND_BOUNCES = 40, 2, 3
BAND_CASES = [("torus_d6", "rotated"), (FULL, "zoo")]


@pytest.mark.parametrize("name,view", BAND_CASES)
def test_bands_with_padding_rows_reassemble_the_frame(sb, name, view):
    import torch
    BandLayout, deinterleave, render_bands = sb.tiles.BandLayout, sb.tiles.deinterleave, sb.tiles.render_bands
    W = BAND_W
    pt = sb.PathTrace(spp=BAND_SPP, max_bounces=BAND_BOUNCES, albedo=1.0)
    stream = torch.cuda.current_stream().cuda_stream
    idle = 0
    with sb.Scene(octdata(sb, name)) as scene:
        for H in (37, 65):
            ref, cnt = pz.reference(name, W, H, BAND_SPP, BAND_BOUNCES, albedo=1.0, view=view)
            cam = pz.camera(view, W, H)
            for band_rows in (8, 16):
                for world in (2, 3, 5):
                    lay = BandLayout(H, world, band_rows)
                    assert lay.n_bands * band_rows > H                 # the last band has rows that are no pixel
                    what = f"{name} {W}x{H}, {world} ranks, bands of {band_rows} rows"
                    for count in (sb.FLAG_COUNT, 0):
                        gathered = torch.full((world, lay.rows_per_rank, W, 4), -2.0, dtype=torch.float32, device="cuda")
                        total = np.zeros(4, dtype=np.int64)
                        for r in range(world):
                            idle += not lay.bands_of(r)                # a rank without a band still launches: every row of its share is padding
                            st = sb.Stats() if count else None
                            render_bands(scene, cam, W, lay, r, gathered[r].data_ptr(), flags=count, stream=stream, stats=st, pt=pt)
                            if count:
                                total += np.array(counters(st), dtype=np.int64)
                        frame = torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda")
                        deinterleave(0, gathered.data_ptr(), frame.data_ptr(), W, lay, stream=stream)
                        torch.cuda.synchronize()
                        assert_frames_identical(frame.cpu().numpy(), ref, what + (", counting" if count else ""))
                        assert not count or tuple(int(c) for c in total) == cnt, what
    assert idle > 0


@pytest.mark.parametrize("name,view", BAND_CASES)
def test_bands_with_padding_rows_over_three_ranks_of_one_device(sb, name, view):
    pt = sb.PathTrace(spp=BAND_SPP, max_bounces=BAND_BOUNCES, albedo=1.0)
    with sb.MultiScene(octdata(sb, name), [0, 0, 0]) as ms:
        for weighted in (False, True):
            if weighted:
                ms.configure(band_rows=8, rank0_weight=0.7)
            for H in (37, 65):
                ref, _ = pz.reference(name, BAND_W, H, BAND_SPP, BAND_BOUNCES, albedo=1.0, view=view)
                got = ms.Draw(pz.camera(view, BAND_W, H), BAND_W, H, pt=pt)
                assert_frames_identical(got, ref, f"{name} {BAND_W}x{H} over three ranks, {'bands of 8 rows, rank 0 at 0.7' if weighted else 'the default deal'}")


# ---- 6. scratch ------------------------------------------------------------------------------------------------------------------
def test_the_streams_path_buffers_grow_and_are_kept(sb, oracle_mod, full_scene):
    import torch
    small, large = (8, 8, 1, DEEP), (64, 48, 4, DEEP)
    for W, H, spp, mb in (small, large, small):                       # the buffer grows once and serves the small frame again
        st = through_the_pipeline(full_scene, draw(sb, full_scene, FULL, "small, large, small", W, H, spp, mb, kernels=(sb.KERNEL_STACK,)))
        assert st.n_hits == W * H * spp * (mb + 1)
    # an ordinary frame between two path-traced ones, on the same stream's scratch
    s, v = pz.tree(FULL)
    cam = pz.camera("zoo", 64, 48)
    plain = pz.tz.restated(("render", FULL, 64, 48), lambda: oracle_mod.render(s, v, cam.State, 64, 48, nthreads=8))
    img, st = full_scene.Draw(cam, 64, 48, sb.KERNEL_STACK | sb.FLAG_COUNT, want_stats=True)
    assert_frames_identical(img, plain[0], "an ordinary frame between two path-traced ones")
    assert counters(st) == tuple(int(c) for c in plain[1])
    draw(sb, full_scene, FULL, "after an ordinary frame", *small, kernels=(sb.KERNEL_STACK,))
    # two frames of different sizes in flight on two streams: each stream has its own buffers, grown on its own
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    jobs = [(a, large), (b, small)]
    bufs = [torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda") for _, (W, H, _, _) in jobs]
    torch.cuda.synchronize()                                          # (the fills run on torch's stream, the renders on their own)
    for rep in range(2):                                              # (the second round finds both buffers in place)
        for (stream, (W, H, spp, mb)), buf in zip(jobs, bufs):
            full_scene.DrawPathDevice(pz.camera("zoo", W, H), W, H, buf.data_ptr(), pt=sb.PathTrace(spp=spp, max_bounces=mb, albedo=1.0),
                                      flags=sb.KERNEL_STACK, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    for (_, (W, H, spp, mb)), buf in zip(jobs, bufs):
        assert_frames_identical(buf.cpu().numpy(), pz.reference(FULL, W, H, spp, mb)[0], f"{W}x{H} in flight beside the other")
    del a, b


# ---- 7. the laboratory's forms on full queues ---------------------------------------------------------------------------------------
def test_laboratory_forms_on_full_queues(sb, full_scene):
    if not sb._lib.EXPERIMENTS:
        pytest.skip("include/sdfhip_experimental.h: the experiments build only")
    W, H, spp, mb = 40, 24, 3, 8
    knobs = ("SDFHIP_PT_SORT", "SDFHIP_PT_SORT_FROM", "SDFHIP_PT_SORT_XCD", "SDFHIP_PT_REFILL")
    prev = {k: os.environ.get(k) for k in knobs}
    try:
        for values in (("1", "0", "0", "0"), ("2", "0", "0", "0"), ("3", "0", "0", "0"), ("3", "1", "0", "0"), ("2", "5", "0", "0"),
                       ("3", "0", "1", "0"), ("2", "1", "1", "0"), ("0", "0", "0", "1")):
            os.environ.update(zip(knobs, values))
            what = ", ".join(f"{k}={v}" for k, v in zip(knobs, values))
            st = through_the_pipeline(full_scene, draw(sb, full_scene, FULL, what, W, H, spp, mb, kernels=(sb.KERNEL_STACK,)))
            assert st.n_hits == W * H * spp * (mb + 1), what
    finally:
        for k, v in prev.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

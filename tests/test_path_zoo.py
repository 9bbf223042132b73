"""The path-traced mode's hostile cases, and the oracle's own word that they are hostile.  tests/test_gpu_path_zoo.py holds the
pipeline of kernels (k_pt_primary -> k_pt_bounce per level -> k_pt_resolve, and the one-kernel k_path) to oracle.render_pt on the
trees of tests/tree_zoo.py, whose bytes are no distance field: a path there goes on hitting, level after level, where a path on
sphere_d4 or torus_d6 has left for the sky after two bounces.  What makes those cases worth their time is asserted HERE, from the
oracle alone, so that a later change of a tree or of the camera cannot quietly empty one:

  full queues   on blocks_2049 (every cell flat 63 or 64) every path hits at every one of the 65 levels;
  deep levels   on every other tree the level-64 vertices still exist (the counters at max_bounces = 64 differ from those at 63);
  NaN normals   zero gradients (rg = inf, a NaN normal, a NaN bounce direction) reach the frame as NaN channels;
  step field    a path's march steps, which the pipeline keeps in 16 bits beside its vertex count, stay far below 65 536;
  determinism   the oracle's frame and counters do not depend on its thread count.

This module is also the one place the two files take their cases and references from: a reference frame is rendered once per
process (reference()), whichever test and whichever flavour of the library asks for it."""
import numpy as np
import pytest

import tree_zoo as tz
from conftest import bits_equal, make_camera

W0, H0, SPP0 = 24, 16, 2                                    # the frame of the per-tree cases
DEEP = 64                                                   # max_bounces: the ABI's limit, 65 levels
ZOO_POSITION = (0.3, 0.4, -0.2)                             # the camera of test_degenerate_and_deep_trees, heading 0
DEFAULT_SEED = 0x5DFB0C5
FULL = "blocks_2049"                                        # the full-queue tree
BAD_PARENT = "dfs_d6_a_bad_parent"                          # dfs_d6_a with a block that names a sibling of its parent as its parent
PATH_TREES = tz.ALL_TREES + [BAD_PARENT]
# From ZOO_POSITION no path on blocks_65 or blocks_4097 lives to level 64 (the oracle's counters at max_bounces = 63 and 64 are equal);
# from conftest's "rotated" camera one does on every tree of the zoo.
VIEW = {name: "rotated" if name in ("blocks_65", "blocks_4097") else "zoo" for name in PATH_TREES}
MAX_STEPS_PER_PATH = (DEEP + 1) * (100 + 40)                # per level at most 100 steps of a segment and 40 of a shadow ray: 9 100


def tree(name):
    """(structs, values) of a zoo tree, of the inconsistent one, or of one of the two tame scenes"""
    if name in ("sphere_d4", "torus_d6"):
        import sdfbox_amd
        od = getattr(sdfbox_amd, name)()
        return od.Structs, od.Values
    if name == BAD_PARENT:
        def make():
            s, v = tz.zoo()["dfs_d6_a"]
            s = s.copy()
            first = int(s[1:, 1][s[1:, 1] > 0][0])         # the first block below the root's own
            parent = int(s[first, 0])
            assert 1 <= parent <= 8
            s[first:first + 8, 0] = parent % 8 + 1          # ... claims its parent's neighbour
            s.setflags(write=False)
            return s, v
        return tz.restated(("path tree", name), make)
    return tz.zoo()[name]


def camera(view, W, H):
    """"zoo" = the camera every zoo tree is seen from; else one of conftest.CAMERAS"""
    if view != "zoo":
        return make_camera(view, W, H)
    import sdfbox_amd
    cam = sdfbox_amd.Logic(W, H)
    cam.Position = ZOO_POSITION
    return cam


def reference(name, W=W0, H=H0, spp=SPP0, max_bounces=DEEP, seed=DEFAULT_SEED, albedo=1.0, view=None, nthreads=8):
    """oracle.render_pt of the case (view: the tree's own, VIEW) -> (frame, (nodes, samples, steps, shadow rays)); rendered once per process"""
    import oracle
    view = view or VIEW.get(name, "zoo")
    key = ("render_pt", name, W, H, spp, max_bounces, seed, repr(float(albedo)), view, nthreads)

    def make():
        s, v = tree(name)
        img, cnt = oracle.render_pt(s, v, camera(view, W, H).State, W, H, spp=spp, max_bounces=max_bounces, seed=seed, albedo=albedo,
                                    nthreads=nthreads)
        img.setflags(write=False)
        return img, tuple(int(c) for c in cnt)
    return tz.restated(key, make)


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_mod):
    return oracle_mod


def test_every_path_hits_at_every_level_on_the_full_queue_tree():
    img, (nodes, samples, steps, rays) = reference(FULL)
    assert rays == W0 * H0 * SPP0 * (DEEP + 1) == 49_920       # a shadow ray per vertex: no path ever escapes, no vertex faces away
    assert samples == steps == int(img[..., 3].astype(np.float64).sum())
    # ... at every frame size, sample count and depth of tests/test_gpu_path_zoo.py's edge cases (their queue fills are computed from this)
    for (W, H), spp, mb, seed in EDGE_PRECONDITIONS:
        _, cnt = reference(FULL, W, H, spp, mb, seed)
        assert cnt[3] == W * H * spp * (mb + 1), (W, H, spp, mb, seed)


@pytest.mark.parametrize("name", [n for n in PATH_TREES if n != FULL])
def test_the_last_level_is_populated(name):
    deep, shallower = reference(name)[1], reference(name, max_bounces=DEEP - 1)[1]
    assert deep != shallower, f"{name}: no path reaches level {DEEP} from this camera"
    assert deep[3] > shallower[3] or deep[2] > shallower[2]


def test_zero_gradients_reach_the_frame_as_nan():
    share = {n: float(np.isnan(reference(n)[0][..., :3]).mean()) for n in ("dfs_d6_b", FULL)}
    assert all(0.001 < f < 0.05 for f in share.values()), share      # (0.26 % and 1.04 % of the channels when this was written)
    for n in ("dfs_d6_b", FULL):
        assert np.isfinite(reference(n)[0][..., 3]).all()             # the step count is a count, whatever the colour


@pytest.mark.parametrize("name", PATH_TREES)
def test_a_paths_steps_fit_the_sixteen_bits_the_pipeline_gives_them(name):
    # spp = 1: a pixel's alpha is ONE path's step total (the oracle exposes nothing per path)
    alpha = reference(name, spp=1)[0][..., 3]
    assert alpha.max() <= MAX_STEPS_PER_PATH == 9_100 < 65_536, (name, float(alpha.max()))
    # and with more samples the mean per path obeys the same bound in every case the GPU file renders at 24 x 16
    assert reference(name)[0][..., 3].max() <= SPP0 * MAX_STEPS_PER_PATH


@pytest.mark.parametrize("name", PATH_TREES)
def test_the_oracle_does_not_depend_on_its_thread_count(name, oracle_mod):
    s, v = tree(name)
    ref, cnt = reference(name)
    for nthreads in (1, 3):
        img, c = oracle_mod.render_pt(s, v, camera(VIEW[name], W0, H0).State, W0, H0, spp=SPP0, max_bounces=DEEP, seed=DEFAULT_SEED, albedo=1.0,
                                      nthreads=nthreads)
        assert bits_equal(img, ref).all() and tuple(int(x) for x in c) == cnt, (name, nthreads)


# ---- the edge cases of the full-queue tree: frame sizes, sample counts, depths, seeds (tests/test_gpu_path_zoo.py renders them) --------
EDGE_SIZES = [(1, 1), (7, 3), (8, 8), (9, 9), (63, 1), (1, 65)]
EDGE_SPP = (1, 3, 64)
EDGE_BOUNCES = (0, 1, 2, DEEP)
EDGE_SEEDS = (0, 0xFFFFFFFF)                                # seed + pixel wraps past 2^32 on every pixel but the first


def edge_cases(size):
    """[(spp, max_bounces, seed)] of one frame size: the whole product, and 4096 samples on the single pixel"""
    out = [(spp, mb, seed) for spp in EDGE_SPP for mb in EDGE_BOUNCES for seed in EDGE_SEEDS]
    if size == (1, 1):
        out += [(4096, mb, seed) for mb, seed in ((DEEP, 0), (2, 0xFFFFFFFF))]
    return out


# the deepest, widest cases of every size, for the full-queue assertion above (the others are their prefixes in depth)
EDGE_PRECONDITIONS = [(size, spp, DEEP, seed) for size in EDGE_SIZES for spp in (1, 64) for seed in EDGE_SEEDS]

"""Volume out and compose on the tree zoo (tests/tree_zoo.py), both flavours of the library: the two calls that take any uploaded
handle and had only met trees the project's own builders lay out -- here depth-first order, blocks appended under random leaves, the
12-deep and the 14-deep chain, one node, node counts one past a wave, a row and a scan chunk, bytes that are no distance field, through
every cursor form.  Every element and every byte is the numpy restatement's (tests/volume_restatement.py, compose_restatement.py;
tests/test_zoo_volumes.py holds those to things they did not come from on these same cases), with no tolerance anywhere.  Then a
lattice long enough for a second trip of k_volume_out's loop, and the calls chained on the handles they return."""
import ctypes

import numpy as np
import pytest

import edit_restatement as er
import prune_restatement as pr
import tree_zoo as tz
import volume_restatement as vr
from conftest import assert_frames_identical, make_camera
from test_gpu_prune import assert_same_tree

pytestmark = pytest.mark.gpu
W, H = 64, 48
FORMS = ("default", "none", "split")


@pytest.fixture(scope="module", params=["product", "lab"])
def sb(request):
    import sdfbox_amd
    if request.param == "product":
        return sdfbox_amd
    import sdfbox_amd.lab
    return sdfbox_amd.lab.load()


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


def split_level(name):
    depth = er.tree_depth(tz.zoo()[name][0])
    return max(depth // 2, depth - 6)


def has_split(name):
    """a split grid is the sources' to have where its coarse level lies below the depth, and the tree is one the grids take"""
    depth = er.tree_depth(tz.zoo()[name][0])
    return 1 <= split_level(name) < depth <= 12


def upload(sb, name, form="default"):
    """the zoo tree with the default cursor, with no grid (the walk along the links), or with a split grid"""
    s, v = tz.zoo()[name]
    kw = {"default": {}, "none": dict(top_grid_level=0), "split": dict(top_grid_split=split_level(name))}[form]
    scene = sb.Scene(sb.OctData(s, v), **kw)
    depth = er.tree_depth(s)
    if depth > 12:                                                  # no grid is built for a tree the stack kernels refuse
        assert not scene.stack_kernel_ok and scene.top_grid_level == 0, (name, form)
    elif form == "none":
        assert scene.top_grid_level == 0, name
    elif form == "split":
        assert scene.top_grid_level == split_level(name) < scene.depth, name
    return scene


def forms_of(name):
    return [f for f in FORMS if f != "split" or has_split(name) or name == "chain14"]


# ---- volume out ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tz.ALL_TREES)
def test_a_zoo_tree_on_a_lattice_is_the_restatement_and_the_samplers(sb, name):
    import torch
    assert "none" in forms_of(name) and (name in ("leaf",) or "split" in forms_of(name))
    for form in forms_of(name):
        with upload(sb, name, form) as scene:
            for lattice in tz.out_lattices():
                shape, origin, spacing = lattice
                what = (name, form, lattice)
                want, want16 = tz.restated_out(name, lattice), tz.restated_out(name, lattice, np.float16)
                got = scene.Volume(*lattice)
                assert got.shape == tuple(shape) and got.dtype == np.float32
                assert np.array_equal(bits(got), bits(want)), what
                # inside the cube the element IS the sample at the same float32 coordinates
                p = vr.lattice_points(shape, origin, spacing)
                inside = ((p >= 0) & (p <= 1)).all(1)
                assert np.array_equal(bits(got.reshape(-1)[inside]), bits(scene.Sample(p[inside])["distance"])), what
                half = scene.Volume(*lattice, dtype=np.float16)
                assert half.dtype == np.float16 and np.array_equal(bits(half), bits(want16)), what
                # the device form, on the current torch stream
                for dtype, host in ((torch.float32, want), (torch.float16, want16)):
                    out = torch.full(tuple(shape), 7.0, dtype=dtype, device="cuda")
                    assert scene.Volume(shape, origin, spacing, out=out) is out
                    torch.cuda.current_stream().synchronize()
                    assert np.array_equal(bits(out.cpu().numpy()), bits(host)), (what, dtype)


def test_a_lattice_past_the_first_stride_of_the_out_kernel(sb):
    """257^3 elements against k_volume_out's 2^16 workgroups of 256 threads = 2^24: the last 197 377 elements are a thread's second
    trip, and slab 254 straddles element 2^24.  The positions are exact, so the first and the last three slabs are lattices of
    their own -- which the same call fills bit for bit, and which the restatement restates in 0.7 s each (the whole: 50 s)."""
    (nz, ny, nx), origin, spacing = tz.LONG_OUT
    assert nz * ny * nx > 2 ** 24 > 254 * ny * nx
    with upload(sb, tz.LONG_OUT_SOURCE) as scene:
        got = scene.Volume(*tz.LONG_OUT)
        assert got.shape == (257, 257, 257)
        for k0 in (0, 254):
            want = tz.restated_out(tz.LONG_OUT_SOURCE, tz.slabs(k0))
            assert np.array_equal(bits(got[k0:k0 + 3]), bits(want)), f"slabs {k0}..{k0 + 2} of the long lattice"
            assert np.array_equal(bits(scene.Volume(*tz.slabs(k0))), bits(want)), f"slabs {k0}..{k0 + 2} read alone"
        del got
        half = scene.Volume(*tz.LONG_OUT, dtype=np.float16)
        want16 = tz.restated_out(tz.LONG_OUT_SOURCE, tz.slabs(254), np.float16)
        assert half.dtype == np.float16 and np.array_equal(bits(half[254:257]), bits(want16)), "the tail slabs as float16"


# ---- compose ---------------------------------------------------------------------------------------------------------------------
class Uploaded:
    """one handle per distinct source of a list and per cursor form the source has, closed at the end of the `with`"""

    def __init__(self, sb, names):
        self.scenes = {(src, form): upload(sb, src, form) for src in dict.fromkeys(names) for form in forms_of(src)}

    def handle(self, src, form):
        return self.scenes[(src, form) if (src, form) in self.scenes else (src, "default")]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for s in self.scenes.values():
            s.close()


@pytest.mark.parametrize("name", list(tz.COMPOSE_LISTS))
def test_composed_bytes_are_the_restatements_on_the_zoo_in_every_cursor_form(sb, name):
    parts = tz.compose_parts(name)
    with Uploaded(sb, [src for src, _, _ in parts]) as up:
        for depth in tz.COMPOSE_DEPTHS:
            S, V, counts = tz.restated_compose(name, depth)
            # every instance in one form, then the forms mixed within one call: instance k in form k, k + 1, k + 2 (mod 3)
            choices = [[form] * len(parts) for form in FORMS] + [[FORMS[(k + turn) % 3] for k in range(len(parts))] for turn in range(3)]
            for forms in choices:
                handles = [(up.handle(src, form), pl, op) for (src, pl, op), form in zip(parts, forms)]
                res, got, st = sb.Scene.Compose(handles, depth, want_octdata=True, want_stats=True)
                with res:
                    what = f"compose({name}) depth={depth} forms={forms}"
                    assert_same_tree(got, S, V, what)
                    assert (st.nodes_out, st.depth_out, st.levels, st.instances) == (len(S), counts["depth_out"], counts["levels"], len(parts)), what
                    assert st.samples == counts["samples"] and st.depth_out == er.tree_depth(S), what
                    assert res.Length == len(S) and res.depth == st.depth_out and res.stack_kernel_ok, what


def test_the_14_deep_chain_is_refused_without_a_depth_and_leaves_both_handles_usable(sb):
    L = sb._lib
    parts = tz.compose_parts("chain14")
    with upload(sb, "leaf") as leaf, upload(sb, "chain14") as deep:
        assert not deep.stack_kernel_ok and deep.depth == 14
        handle = {"leaf": leaf, "chain14": deep}
        items = [sb.Instance(handle[src]._h, op, np.asarray(pl[0]).tolist(), float(pl[1]), [float(x) for x in pl[2]]) for src, pl, op in parts]
        arr = (sb.Instance * len(items))(*items)
        for opt in (None, ctypes.byref(sb.ComposeOptions(None))):
            h = ctypes.c_void_p(1)
            assert L.lib.sdfhip_scene_compose(arr, len(items), opt, ctypes.byref(h), None, None) == L.ERR_BAD_TREE
            assert not h.value, "*out is null after the refusal"
            assert b"instance 1" in L.lib.sdfhip_last_error()
        # both handles afterwards: the same list with a depth, and each source read on a lattice
        S, V, _ = tz.restated_compose("chain14", 4)
        res, got = sb.Scene.Compose([(handle[src], pl, op) for src, pl, op in parts], 4, want_octdata=True)
        with res:
            assert_same_tree(got, S, V, "compose(chain14) with a depth, after the refusal")
        for src, scene in handle.items():
            assert np.array_equal(bits(scene.Volume(*tz.DEEP_CORNER)), bits(tz.restated_out(src, tz.DEEP_CORNER))), src


# ---- chains ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src, D", [("blocks_1025", 4), ("dfs_d6_a", 4), ("chain12", 4)])
def test_out_then_in_is_the_restated_identity_placement_on_the_zoo(sb, src, D):
    import torch
    S, V, _ = tz.restated_place(src, "identity", D)
    lattice = sb.lattice_of_depth(D)
    with upload(sb, src) as scene:
        res, got = sb.Scene.FromVolume(scene.Volume(*lattice), lattice[1], lattice[2], depth=D, want_octdata=True)
        with res:
            assert_same_tree(got, S, V, f"FromVolume(Volume({src})) to depth {D}")
        # ... and without the field leaving the device
        out = torch.empty(lattice[0], dtype=torch.float32, device="cuda")
        res, got = sb.Scene.FromVolume(scene.Volume(*lattice, out=out), lattice[1], lattice[2], depth=D, want_octdata=True)
        with res:
            assert_same_tree(got, S, V, f"FromVolume(Volume({src})) on the device to depth {D}")
    assert len(S) > 1000


def test_compose_prune_volume_on_returned_handles(sb, oracle_mod):
    name, depth = "csg", 5
    CS, CV, _ = tz.restated_compose(name, depth)
    PS, PV = tz.restated(("chain 3", "pruned"), lambda: pr.prune(CS, CV, 8))
    lattice = sb.lattice_of_depth(4)
    want = tz.restated(("chain 3", "out"), lambda: vr.volume_out((PS, PV), *lattice))
    assert 1 < len(PS) < len(CS)
    cam = make_camera("rotated", W, H)
    ref = tz.restated(("chain 3", "frame"), lambda: oracle_mod.render(PS, PV, cam.State, W, H)[0])
    parts = tz.compose_parts(name)
    with Uploaded(sb, [src for src, _, _ in parts]) as up:
        sources = [up.handle(src, "default") for src in dict.fromkeys(src for src, _, _ in parts)]
        before = [sc.Draw(cam, W, H) for sc in sources]
        with sb.Scene.Compose([(up.handle(src, "default"), pl, op) for src, pl, op in parts], depth) as composed:
            pruned, got = composed.Prune(8, None, want_octdata=True)
        with pruned:                                                # (the composition's handle is gone: the result stands alone)
            assert_same_tree(got, PS, PV, "compose -> prune(8)")
            assert np.array_equal(bits(pruned.Volume(*lattice)), bits(want)), "compose -> prune(8) -> volume"
            assert np.array_equal(bits(pruned.Volume(*lattice, dtype=np.float16)), bits(want.astype(np.float16)))
            assert_frames_identical(pruned.Draw(cam, W, H), ref, "compose -> prune(8)")
            assert_frames_identical(pruned.Draw(cam, W, H, sb.KERNEL_GENERIC), ref, "compose -> prune(8), the generic kernel")
        for sc, frame in zip(sources, before):
            assert_frames_identical(sc.Draw(cam, W, H), frame, "a source after the chain")

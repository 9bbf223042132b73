"""Composition on the GPU (sdfhip_scene_compose), both flavours of the library: the composed tree is the CPU restatement's
(tests/compose_restatement.py) byte for byte -- every case of tests/compose_cases.py -- its statistics are the restatement's counts,
instances of every cursor form in one call give the same bytes, its frames are the oracle's on the restated arrays, the sources are
untouched, a composition chains with the prune and the combination as the restatements do, and the errors are status codes.  The
second round's cases: depth 12 in the far corner (that its one-instance variant is the placement's tree is tests/test_compose.py's, on
the restatements) and lists of 63, 64 and 4096 instances.  Zoo trees as sources: tests/test_gpu_zoo_volumes.py."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import combine_restatement as cr
import compose_cases as cc
import compose_restatement as cpr
import edit_restatement as er
import place_restatement as plr
import prune_restatement as pr
from conftest import REPO, assert_frames_identical, make_camera
from test_gpu_prune import assert_same_tree

tree = cc.tree

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["product", "lab"])
def sb(request):
    import sdfbox_amd
    if request.param == "product":
        return sdfbox_amd
    import sdfbox_amd.lab
    return sdfbox_amd.lab.load()


class Uploaded:
    """one handle per distinct source of a list of parts, closed at the end of the `with`"""

    def __init__(self, sb, parts, **kw):
        self.sb, self.scenes = sb, {}
        for src, _, _ in parts:
            if src not in self.scenes:
                self.scenes[src] = sb.Scene(sb.OctData(*tree(src)), **kw.get(src, {}))

    def parts(self, parts):
        return [(self.scenes[src], pl, op) for src, pl, op in parts]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for s in self.scenes.values():
            s.close()


def gpu_compose(sb, up, parts, depth, **kw):
    return sb.Scene.Compose(up.parts(parts), None if depth < 0 else depth, **kw)


def check_case(sb, name):
    parts, depth = cc.case(name)
    S, V, counts = cc.restated(name)
    with Uploaded(sb, parts) as up:
        res, got, st = gpu_compose(sb, up, parts, depth, want_octdata=True, want_stats=True)
        with res:
            what = f"compose({name})"
            assert_same_tree(got, S, V, what)
            assert (st.nodes_out, st.depth_out, st.levels, st.instances) == (len(S), counts["depth_out"], counts["levels"], len(parts)), what
            assert st.samples == counts["samples"] and st.depth_out == er.tree_depth(S), what
            assert res.Length == len(S) and res.depth == st.depth_out and res.stack_kernel_ok, what


@pytest.mark.parametrize("name", cc.ONE + cc.MULTI)
def test_composed_bytes_are_the_restatements(sb, name):
    check_case(sb, name)


# the sizes the restatement gives for the cases of compose_cases.py
EIGHT_NODES, CSG_NODES, MANY_NODES, FAR_NODES = 32657, 57105, 4457, 152665


def test_the_cases_are_what_they_are_for():
    assert len(tree("nine")[0]) == 9 and len(tree("leaf")[0]) == 1
    assert [er.tree_depth(tree(s)[0]) for s in ("sphere_d4", "torus_d6")] == [4, 6]
    # one instance: the placement's own restatement (tests/test_compose.py holds every byte; here the sizes)
    for name in cc.ONE:
        (src, pl, op), = cc.case(name)[0]
        assert op == cpr.COMBINE_UNION and len(cc.restated(name)[0]) == len(plr.place(tree(src), *pl)[0])
    assert np.linalg.det(cc.ONE_PLACEMENTS["mirror"]()[0]) < 0
    # eight instances of ONE source, each turned differently, in the eight octants: the restatement's sizes are pinned
    parts, depth = cc.case("eight")
    assert len(parts) == 8 and {src for src, _, _ in parts} == {"sphere_d4"} and depth == 5
    assert len({tuple(np.round(pl[0].ravel(), 4)) for _, pl, _ in parts}) == 8 and all(float(pl[1]) == np.float32(0.4) for _, pl, _ in parts)
    lands = [float(pl[1]) * pl[0].astype(np.float64) @ np.full(3, 0.5) + pl[2] for _, pl, _ in parts]      # the source's centre
    assert len({tuple(x > 0.5) for x in lands}) == 8, "one instance in each octant"
    assert len(cc.restated("eight")[0]) == EIGHT_NODES and cc.restated("eight")[2]["depth_out"] == 5
    # a union, then a difference, then an intersection, of two sources at three placements
    parts, depth = cc.case("csg")
    assert [op for _, _, op in parts] == [cpr.COMBINE_UNION, cpr.COMBINE_SUBTRACT, cpr.COMBINE_INTERSECT] and depth == 6
    assert [src for src, _, _ in parts] == ["torus_d6", "sphere_d4", "sphere_d4"]
    assert len(cc.restated("csg")[0]) == CSG_NODES
    # each of the later instances changes the tree: the intersection its size, the difference its bytes (a solid's inside saturates
    # within the split rule's band, so carving inside a solid moves signs, not splits)
    without_cut, without_meet = (cpr.compose(cc.with_trees([p for k, p in enumerate(parts) if k != drop]), depth) for drop in (1, 2))
    assert len(without_meet[0]) != CSG_NODES and not np.array_equal(without_cut[1], cc.restated("csg")[1])
    # more instances than a wave has lanes, both ops that a small part can be joined with
    parts, depth = cc.case("many")
    assert len(parts) == 65 > 64 and depth == 4 and {op for _, _, op in parts} == {cpr.COMBINE_UNION, cpr.COMBINE_SUBTRACT}
    assert len(cc.restated("many")[0]) == MANY_NODES
    # the far instance: the torus's placement alone (tests/test_compose.py holds the bytes)
    assert len(cc.restated("far")[0]) == FAR_NODES and cc.restated("far")[2]["depth_out"] == 7
    assert len(cc.restated("depth0")[0]) == 1, "depth 0: the root alone"
    parts, depth = cc.case("deepest")
    assert depth == -1 and sorted(er.tree_depth(tree(src)[0]) for src, _, _ in parts) == [4, 6]
    assert cc.restated("deepest")[2]["depth_out"] == 6 and len(cc.restated("deepest")[0]) > 1000
    # level lists that end inside a workgroup of the first pass: four blocks of eight siblings to a workgroup
    blocks = [len(level) // 8 for level in pr.levels(cc.restated("csg")[0])]
    assert any(b > 4 and b % 4 for b in blocks), blocks
    # arrays that had to grow: they start at 1.5 times the distinct sources together
    assert FAR_NODES > 2 * ((len(tree("torus_d6")[0]) + len(tree("sphere_d4")[0])) * 3 // 2)
    # depth 12 in the far corner and the instance limit: tests/test_compose.py pins them without a GPU; here what the GPU run leans on
    assert cc.restated("corner_d12")[2]["depth_out"] == 12 and len(cc.restated("corner_d12")[0]) == cc.CORNER_D12_NODES
    assert [len(cc.case(f"limit_{n}")[0]) for n in (63, 64, cc.LIMIT)] == [63, 64, 4096] and cc.LIMIT == 4096


def test_instances_of_every_cursor_form_in_one_call(sb):
    parts, depth = cc.case("deepest")
    S, V, _ = cc.restated("deepest")
    names = [src for src, _, _ in parts]
    split_level = {src: max(er.tree_depth(tree(src)[0]) // 2, er.tree_depth(tree(src)[0]) - 6) for src in names}
    with Uploaded(sb, parts) as grid, Uploaded(sb, parts, **{src: dict(top_grid_level=0) for src in names}) as none, \
            Uploaded(sb, parts, **{src: dict(top_grid_split=split_level[src]) for src in names}) as split:
        for src in names:
            g, n, s = grid.scenes[src], none.scenes[src], split.scenes[src]
            assert g.stack_kernel_ok and g.top_grid_level >= g.depth and n.top_grid_level == 0
            assert s.top_grid_level == split_level[src] < s.depth
        # the four pairings of a source with a full-depth grid and one without
        for first in (grid, none):
            for second in (grid, none):
                handles = [(first.scenes[names[0]], parts[0][1], parts[0][2]), (second.scenes[names[1]], parts[1][1], parts[1][2])]
                res, got = sb.Scene.Compose(handles, want_octdata=True)
                with res:
                    assert_same_tree(got, S, V, f"grids: {first is grid}, {second is grid}")
        # ... and all three forms in one list: the walk along the links, the dense grid and the split grid
        for a, b in ((split, none), (grid, split), (split, split)):
            handles = [(a.scenes[names[0]], parts[0][1], parts[0][2]), (b.scenes[names[1]], parts[1][1], parts[1][2])]
            res, got = sb.Scene.Compose(handles, want_octdata=True)
            with res:
                assert_same_tree(got, S, V, "a split grid among the forms")
        three = [("sphere_d4", parts[0][1], cpr.COMBINE_UNION), ("sphere_d4", cc.ONE_PLACEMENTS["generic_half"](), cpr.COMBINE_SUBTRACT),
                 ("sphere_d4", cc.ONE_PLACEMENTS["mirror"](), cpr.COMBINE_UNION)]
        want = cpr.compose(cc.with_trees(three), 5)
        handles = [(up.scenes["sphere_d4"], pl, op) for up, (_, pl, op) in zip((grid, split, none), three)]
        res, got = sb.Scene.Compose(handles, 5, want_octdata=True)
        with res:
            assert_same_tree(got, *want, "three forms of one source in one call")


def test_composed_frames_are_the_oracles_and_the_sources_are_untouched(sb, oracle_mod):
    W, H = 64, 48
    parts, depth = cc.case("csg")
    S, V, _ = cc.restated("csg")
    cams = [make_camera(cam, W, H) for cam in ("default", "rotated")]
    with Uploaded(sb, parts) as up:
        before = {src: [scene.Draw(cam, W, H) for cam in cams] for src, scene in up.scenes.items()}
        res = gpu_compose(sb, up, parts, depth)
        for src, scene in up.scenes.items():
            for cam, frame in zip(cams, before[src]):
                assert_frames_identical(scene.Draw(cam, W, H), frame, f"{src} after the call")
    # (the sources are freed: the result stands alone)
    with res:
        for cam in cams:
            ref, _ = oracle_mod.render(S, V, cam.State, W, H)
            for flags in (sb.KERNEL_AUTO, sb.KERNEL_GENERIC):
                assert_frames_identical(res.Draw(cam, W, H, flags), ref, f"composed, flags {flags}")


def test_a_composition_beside_frames_in_flight(sb):
    import torch
    W, H = 64, 48
    cam = make_camera("rotated", W, H)
    parts, depth = cc.case("csg")
    S, V, _ = cc.restated("csg")
    with Uploaded(sb, parts) as up:
        scenes = list(up.scenes.values())
        before = [scene.Draw(cam, W, H) for scene in scenes]
        frames = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(6)]
        torch.cuda.synchronize()
        s_frames = torch.cuda.Stream()
        results = []
        for k, buf in enumerate(frames):
            scenes[k % len(scenes)].DrawDevice(cam, W, H, buf.data_ptr(), stream=s_frames.cuda_stream)
            results.append(gpu_compose(sb, up, parts, depth, want_octdata=True))
        torch.cuda.synchronize()
        for k, buf in enumerate(frames):
            assert_frames_identical(buf.cpu().numpy(), before[k % len(scenes)], "a frame in flight beside a composition")
        for res, got in results:
            assert_same_tree(got, S, V, "one of several compositions of the same sources")
            res.close()


def test_compose_then_prune_then_combine(sb):
    parts, depth = cc.case("eight")
    composed = cc.restated("eight")[:2]
    pruned = pr.prune(*composed, 0)
    united = cr.combine(pruned, tree("torus_d6"), cr.COMBINE_UNION)
    assert len(pruned[0]) < len(composed[0]) and len(united[0]) > len(pruned[0])
    with Uploaded(sb, parts) as up, sb.Scene(sb.OctData(*tree("torus_d6"))) as torus:
        with gpu_compose(sb, up, parts, depth) as c, c.Prune(0) as p:
            assert p.Length == len(pruned[0])
            res, got = p.Combine(torus, cr.COMBINE_UNION, want_octdata=True)
            with res:
                assert_same_tree(got, *united, "compose -> prune(0) -> combine")


def test_errors_are_status_codes(sb):
    L = sb._lib

    def call(items, n=None, opt=None, want_out=True, null_list=False):
        arr = (sb.Instance * max(1, len(items)))(*items)
        h = ctypes.c_void_p()
        rc = L.lib.sdfhip_scene_compose(None if null_list else arr, len(items) if n is None else n, ctypes.byref(opt) if opt is not None else None,
                                        ctypes.byref(h) if want_out else None, None, None)
        if h.value:
            L.lib.sdfhip_scene_free(h)
        assert rc == L.OK or not h.value, "*out is not null after a failure"
        return rc, L.lib.sdfhip_last_error()

    R, s, t = cc.ONE_PLACEMENTS["generic_half"]()
    with sb.Scene(sb.OctData(*tree("sphere_d4"))) as scene:
        good = lambda **kw: sb.Instance(**dict(dict(scene=scene._h, op=0, rotation=R.tolist(), scale=s, translation=t.tolist()), **kw))
        five = lambda bad: [good(), good(op=2), good(), bad, good()]
        assert call([good()])[0] == L.OK and call([good()], opt=sb.ComposeOptions(12))[0] == L.OK and call([good()], opt=sb.ComposeOptions(0))[0] == L.OK
        assert call(five(good(op=1)))[0] == L.OK
        rc, msg = call([good()], null_list=True)
        assert rc == L.ERR_ARG and b"null instance list" in msg
        for n in (0, 4097):
            rc, msg = call([good()], n=n)
            assert rc == L.ERR_ARG and b"1..4096" in msg, n
        for op in (1, 2):
            rc, msg = call([good(op=op), good()])
            assert rc == L.ERR_ARG and b"instance 0" in msg, op
        for bad, word in ((good(op=3), b"unknown op"), (good(op=-1), b"unknown op"), (good(scene=None), b"null scene"),
                          (good(rotation=((1, 0, 0), (0, 1, 0), (0, 0, 1.001))), b"orthogonal"),
                          (good(rotation=((1, 2e-4, 0), (0, 1, 0), (0, 0, 1))), b"orthogonal"),
                          (good(scale=0.0), b"scale"), (good(scale=-1.0), b"scale"), (good(scale=float("nan")), b"finite"),
                          (good(translation=(0.0, float("inf"), 0.0)), b"finite")):
            rc, msg = call(five(bad))
            assert rc == L.ERR_ARG and b"instance 3" in msg and word in msg, (word, msg)
        for depth in (13, -2):
            rc, msg = call([good()], opt=sb.ComposeOptions(depth))
            assert rc == L.ERR_ARG and b"depth" in msg, depth
        rc, msg = call([good()], want_out=False)
        assert rc == L.ERR_ARG and b"both outputs" in msg
        small = sb.ComposeOptions()
        small.size = 4
        rc, msg = call([good()], opt=small)
        assert rc == L.ERR_ARG and b"bytes" in msg

        class Newer(ctypes.Structure):
            _fields_ = sb.ComposeOptions._fields_ + [("unknown", ctypes.c_int32)]
        newer = Newer()
        newer.size, newer.depth, newer.unknown = 12, 3, 3
        as_options = ctypes.cast(ctypes.pointer(newer), ctypes.POINTER(sb.ComposeOptions)).contents
        assert call([good()], opt=as_options)[0] == L.ERR_ARG            # an unknown field that is set
        newer.unknown = -1
        assert call([good()], opt=as_options)[0] == L.OK                 # ... and one that says "default"
        # host_out alone is an output
        raw = L.COctData()
        arr = (sb.Instance * 1)(good())
        assert L.lib.sdfhip_scene_compose(arr, 1, None, None, ctypes.byref(raw), None) == L.OK
        assert raw.length == len(cc.restated("one:sphere_d4:generic_half")[0])
        L.lib.sdfhip_octdata_free(ctypes.byref(raw))
        # depth -1 with a source that has no depth to give: refused as the placement refuses it, and taken with a depth given
        S0, V0 = tree("sphere_d4")
        Sb = S0.copy()
        Sb[int(S0[0, 1]) + 3, 0] = int(S0[0, 1])
        with sb.Scene(sb.OctData(Sb, V0)) as bad:
            assert not bad.stack_kernel_ok
            rc, msg = call([good(), good(scene=bad._h)])
            assert rc == L.ERR_BAD_TREE and b"instance 1" in msg
            want = cpr.compose([((S0, V0), (R, s, t)), ((Sb, V0), (plr.IDENTITY, 1.0, (0.25, 0.0, 0.0)))], 4)
            res, got = sb.Scene.Compose([(scene, (R, s, t)), (bad, (plr.IDENTITY, 1.0, (0.25, 0.0, 0.0)))], 4, want_octdata=True)
            with res:
                assert_same_tree(got, *want, "an inconsistent source with a depth given")


def test_an_allocation_that_fails_is_nomem_and_leaves_the_sources():
    # in a fresh process of its own, so that neither the variable nor a failed call can reach the tests beside this one: every
    # allocation the call reaches fails once (k = 0, 1, ... until a call gets through), each is SDFHIP_ERR_NOMEM with no handle, and
    # afterwards the sources render as before and a plain call gives the restatement's tree (tests/compose_fault_child.py).  This is
    # the library's own host-side allocation hook: nothing on the device is provoked.
    S, V, _ = cc.restated("far")
    child = os.path.join(REPO, "tests", "compose_fault_child.py")
    out = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    report = json.loads(out.stdout.strip().splitlines()[-1])
    # the instance table, the level loop's seven buffers, and -- this result is more than twice what the arrays start with -- the
    # growth's two at least
    assert report["codes_ok"] and 10 <= report["failed"] < 64, report
    assert report["source_frames_unchanged"] and report["nodes_after"] == len(S), report
    assert report["structs_sha"] == sha(S) and report["values_sha"] == sha(V), report
    assert report["product_reads_no_variable"], report


def sha(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()

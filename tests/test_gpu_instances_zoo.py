"""The unbaked assembly calls (sdfhip_instances_*) on the tree zoo and at their own edges, both flavours of the library: every case of
tests/instances_zoo_cases.py through sample, raycast, pick and render, host and _device forms, the exact skip on and off, is the CPU
restatement's (tests/instances_restatement.py) bit for bit -- floats as their uint32 views, a NaN equal to a NaN, the rules of
tests/test_gpu_instances.py; padding is zero; a _device form writes nothing past its last record or row.  The sources are trees no
builder lays out (append order, depth-first order, the 12- and the 14-deep chain, bytes that are no distance field, a node that reads
the skip's floor exactly); the lists repeat an entry (ties keep the earlier), fold opposite zeros, and reach the instance limit; the
batches end on a workgroup's edge, the frames have fewer and one more tile than a workgroup takes; the far points overflow the
placement's arithmetic; the sources' three cursor forms give the same bytes.  tests/test_instances_zoo.py shows by the restatement
alone that each case is what it is for."""
import numpy as np
import pytest

import compose_cases as cc
import instances_zoo_cases as zc
import query_restatement as qr
import tree_zoo as tz
from conftest import assert_frames_identical
from test_gpu_zoo_volumes import forms_of, upload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["product", "lab"])
def sb(request):
    import sdfbox_amd
    if request.param == "product":
        return sdfbox_amd
    import sdfbox_amd.lab
    return sdfbox_amd.lab.load()


class Uploaded:
    """one handle per distinct source of a list of parts, a zoo tree in the cursor form asked for; closed at the end of the `with`"""

    def __init__(self, sb, parts, forms=None):
        self.scenes = {}
        for src, _, _ in parts:
            if src not in self.scenes:
                if src in tz.zoo() and src != "leaf":
                    self.scenes[src] = upload(sb, src, (forms or {}).get(src, "default"))
                else:
                    self.scenes[src] = sb.Scene(sb.OctData(*zc.tree(src)))

    def parts(self, parts):
        return [(self.scenes[src], pl, op) for src, pl, op in parts]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for s in self.scenes.values():
            s.close()


def host_answers(sb, handles, name, skip=True, kinds=None, n=None):
    """{kind: answer} of the case through the host forms; n: the first n points and rays only"""
    cam, (W, H), steps = zc.camera(name), zc.size(name), zc.max_steps(name)
    out = {}
    for kind in kinds or zc.kinds(name):
        if kind == "sample":
            out[kind] = sb.Scene.SampleParts(handles, zc.points(name)[:n], skip=skip)
        elif kind == "raycast":
            o, d = zc.rays(name)
            out[kind] = sb.Scene.RaycastParts(handles, o[:n], d[:n], cam.State.margin, cam.State.limit, max_steps=steps, skip=skip)
        elif kind == "pick":
            out[kind] = sb.Scene.PickParts(handles, cam, zc.pixels(name), max_steps=steps, skip=skip)
        else:
            out[kind] = sb.Scene.DrawParts(handles, cam, W, H, max_steps=steps, skip=skip)
    return out


def device_answers(sb, handles, name, skip=True, kinds=None, n=None):
    """{kind: answer} of the case through the _device forms (there is none of pick), on a stream of the test's own.  Every output has
    one record, or one row, more than the call is given, filled beforehand (0xEE, -1): it must come back as it was"""
    import torch
    from sdfbox_amd.renderer import _rays
    cam, (W, H), steps = zc.camera(name), zc.size(name), zc.max_steps(name)
    st = torch.cuda.Stream()
    out = {}
    for kind in kinds or zc.kinds(name):
        if kind == "sample":
            pts = np.ascontiguousarray(zc.points(name)[:n])
            d_in = torch.from_numpy(pts).cuda()
            d_out = torch.full((len(pts) + 1, 32), 0xEE, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            sb.Scene.SamplePartsDevice(handles, d_in.data_ptr(), len(pts), d_out.data_ptr(), stream=st.cuda_stream, skip=skip)
            got = d_out.cpu().numpy()
            assert (got[-1] == 0xEE).all(), (name, kind, "the record past the last is untouched")
            out[kind] = got[:-1].copy().view(np.dtype(sb.PartProbe)).reshape(-1)
        elif kind == "raycast":
            o, d = zc.rays(name)
            rays = _rays(o[:n], d[:n])
            d_in = torch.from_numpy(rays.view(np.uint8).reshape(-1, 32)).cuda()
            d_out = torch.full((len(rays) + 1, 48), 0xEE, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            sb.Scene.RaycastPartsDevice(handles, d_in.data_ptr(), len(rays), cam.State.margin, cam.State.limit, d_out.data_ptr(), max_steps=steps,
                                        stream=st.cuda_stream, skip=skip)
            got = d_out.cpu().numpy()
            assert (got[-1] == 0xEE).all(), (name, kind, "the record past the last is untouched")
            out[kind] = got[:-1].copy().view(np.dtype(sb.PartHit)).reshape(-1)
        elif kind == "frame":
            d_out = torch.full((H + 1, W, 4), -1.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            sb.Scene.DrawPartsDevice(handles, cam, W, H, d_out.data_ptr(), max_steps=steps, stream=st.cuda_stream, skip=skip)
            got = d_out.cpu().numpy()
            assert (got[H] == -1.0).all(), (name, kind, "the row past the last is untouched")
            out[kind] = got[:H]
    # (each call has waited for the stream: nothing is in flight)
    return out


def assert_restated(got, name, what, n=None):
    """tests/test_gpu_instances.py's rules: records by qr.records_differ, padding zero, frames by assert_frames_identical"""
    for kind, answer in got.items():
        if kind == "frame":
            assert_frames_identical(answer, zc.restated(name, "frame"), f"{what}: frame")
            continue
        want = zc.restated(name, kind)[:n] if kind != "pick" else zc.restated(name, kind)
        assert len(answer) == len(want), (what, kind)
        bad = qr.records_differ(answer, want)
        assert not bad, (what, kind, bad)
        assert not any(answer[f].any() for f in answer.dtype.names if f.startswith("pad")), (what, kind, "padding is zero")


def check_case(sb, handles, name, skips=(True, False), n=None, kinds=None):
    for skip in skips:
        assert_restated(host_answers(sb, handles, name, skip, kinds, n), name, f"{name}, host forms, skip {skip}, n {n}", n)
        assert_restated(device_answers(sb, handles, name, skip, kinds, n), name, f"{name}, device forms, skip {skip}, n {n}", n)


@pytest.mark.parametrize("skip", [True, False], ids=["skip", "noskip"])
@pytest.mark.parametrize("name", zc.FULL + ["corner:chain12", "corner:chain14", "far"])
def test_every_case_is_the_restatements(sb, name, skip):
    parts = zc.parts(name)
    with Uploaded(sb, parts) as up:
        if "chain14" in up.scenes:
            # the source that only the walk along the links takes; the header lists no tree that these calls refuse
            assert not up.scenes["chain14"].stack_kernel_ok and up.scenes["chain14"].depth == 14
        check_case(sb, up.parts(parts), name, skips=(skip,))


@pytest.mark.parametrize("n", zc.LIMITS)
def test_the_instance_limit_and_a_wave_of_instances(sb, n):
    name = f"limit_{n}"
    parts = zc.parts(name)
    assert len(parts) == n
    with Uploaded(sb, parts) as up:
        check_case(sb, up.parts(parts), name, skips=(True, False) if n == cc.LIMIT else (True,))


def test_batches_that_end_on_a_workgroups_edge(sb):
    parts = zc.parts("edge")
    with Uploaded(sb, parts) as up:
        handles = up.parts(parts)
        for n in zc.EDGE_COUNTS:
            check_case(sb, handles, "edge", n=n)


@pytest.mark.parametrize("frame", list(zc.EDGE_FRAMES))
def test_frames_of_fewer_tiles_than_a_workgroup_and_of_one_more(sb, frame):
    name = "edge:%dx%d" % frame
    parts = zc.parts(name)
    with Uploaded(sb, parts) as up:
        check_case(sb, up.parts(parts), name)


def test_the_sources_cursor_forms_give_the_same_bytes_on_the_zoo(sb):
    name = "keeps"
    parts = zc.parts(name)
    sources = [src for src, _, _ in parts]
    assert sources == ["chain12", "blocks_4097", "dfs_d6_a"] and all("split" in forms_of(src) for src in sources)
    mixed = {"chain12": "split", "blocks_4097": "none", "dfs_d6_a": "default"}
    for forms in [{src: form for src in sources} for form in ("default", "none", "split")] + [mixed]:
        with Uploaded(sb, parts, forms) as up:
            handles = up.parts(parts)
            for skip in (True, False):
                assert_restated(host_answers(sb, handles, name, skip), name, f"keeps in forms {forms}, skip {skip}")

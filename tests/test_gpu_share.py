"""The sparse wire shares of the N-GPU frame at their edges (sparse2_flush, the four expansion kernels of gather_kernels.h, the
float estimate and the tail resend of sdfhip_multi.hip): what the march kernel writes, checked field by field with
share_restatement.check_share; a counter that wraps; a capacity below the lit pixels; the expansion fed with arbitrary shares;
frames of more than 512 bands; bands that are not whole tile rows; the resend as the product library meets it.  RGBA32F frames
are compared with the CPU oracle, bit for bit; RGBA8 frames with the one-device Scene.DrawDisplay."""
import ctypes
import math

import numpy as np
import pytest

import share_restatement as sr
from conftest import CAMERAS, assert_frames_identical, make_camera
from tree_zoo import _random_tree

pytestmark = pytest.mark.gpu

A5 = 0xA5A5A5A5
VIEWS = dict(CAMERAS,
             sky=((0.5, 0.5, -0.5), (0.0, math.pi)),          # facing away from the cube: every pixel sky
             lit=((0.76, 0.42, 0.40), (-1.10, 5.455)),        # inside the torus' hole: every pixel a lit grey
             near=((0.3, 0.5, 0.05), (0.0, 0.3)))             # a close-up that lights about a fifth of the frame


def view(name, W, H):
    import sdfbox_amd as sb
    if name in CAMERAS:
        return make_camera(name, W, H)
    cam = sb.Logic(W, H)
    cam.Position, cam.Heading = VIEWS[name]
    return cam


@pytest.fixture(scope="module", params=["product", "lab"])
def sb(request):
    # every test of this file runs on both flavours of the library
    import sdfbox_amd
    if request.param == "product":
        return sdfbox_amd
    import sdfbox_amd.lab
    return sdfbox_amd.lab.load()


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    return torch


@pytest.fixture(scope="session")
def oracle_frame(oracle_mod, scenes):
    """(view name, W, H) -> the oracle's frame of torus_d6, rendered once for both flavours and left unchanged"""
    frames = {}

    def get(name, W, H):
        if (name, W, H) not in frames:
            od = scenes["torus_d6"]
            fr, _ = oracle_mod.render(od.Structs, od.Values, view(name, W, H).State, W, H, nthreads=8)
            fr.setflags(write=False)
            frames[name, W, H] = fr
        return frames[name, W, H]
    return get


@pytest.fixture(scope="module")
def torus(sb, scenes):
    sc = sb.Scene(scenes["torus_d6"])
    yield sc
    sc.close()


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
def new_share(torch, nbytes, count=A5, tail=0):
    share = torch.full((nbytes + tail,), 0xA5, dtype=torch.uint8, device="cuda")      # garbage: the render must define all it reads
    if count != A5:
        share[:4] = torch.from_numpy(np.array([count], dtype=np.uint32).view(np.uint8).copy()).cuda()
    return share


def render_share(sb, torch, scene, cams, W, lay, rank, share, cap, count_base):
    L = sb._lib.lib
    infos = (sb.Info * len(cams))(*[c.State for c in cams])
    blist = lay.bands_of(rank)
    bands = (ctypes.c_uint16 * len(blist))(*blist)
    sb._lib.check(L.sdfhip_render_sparse_device(scene._h, infos, len(cams), W, lay.height, lay.band_rows, bands, len(blist), lay.rows_per_rank, cap,
                                                count_base & 0xFFFFFFFF, 0, ctypes.c_void_p(share.data_ptr()),
                                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


def expand_gpu(sb, torch, shares, W, lay, cap, frames, flags=0, only_rank=-1, out=None, counts=None):
    L = sb._lib.lib
    if out is None:
        out = torch.zeros((frames, lay.height, W, 4) if flags == 0 else (frames, lay.height, W), dtype=torch.float32 if flags == 0 else torch.int32, device="cuda")
    ptrs = (ctypes.c_void_p * lay.world)(*[s.data_ptr() if s is not None else None for s in shares])
    owner = (ctypes.c_uint8 * lay.n_bands)(*lay.owner) if lay.weighted else None
    sb._lib.check(L.sdfhip_deinterleave_sparse2_device(0, ptrs, ctypes.c_void_p(out.data_ptr()), W, lay.height, lay.band_rows, lay.world,
                                                       lay.rows_per_rank, owner, cap, frames, flags, only_rank,
                                                       ctypes.c_void_p(counts.data_ptr()) if counts is not None else None,
                                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return out


def as_rgba8(t):
    """an int32 frame tensor of the display pass -> (..., 4) uint8: R, G, B, A"""
    return t.cpu().numpy().view(np.uint8).reshape(tuple(t.shape) + (4,))


def shares_against_the_oracle(sb, torch, scene, cams, refs, W, lay, caps, count=A5, tail=0):
    """One launch per rank into garbage; every share must be a share of the oracle's frames (check_share).  -> the shares (device),
    their downloads, the lit pixels of every rank"""
    wire = sr.wire_of(np.stack(refs))
    shares, host, lit = [], [], []
    for r in range(lay.world):
        cap = caps[r] if isinstance(caps, (list, tuple)) else caps
        nbytes = sb._lib.lib.sdfhip_sparse2_bytes(W, lay.rows_per_rank, len(cams), cap)
        assert nbytes == sr.layout(W, lay.rows_per_rank, len(cams), cap).bytes
        share = new_share(torch, nbytes, count, tail)
        render_share(sb, torch, scene, cams, W, lay, r, share, cap, count)
        torch.cuda.synchronize()
        h = share.cpu().numpy()
        rows = sr.rows_of_rank(wire, lay, r)
        lit.append(sr.check_share(h, rows, count, cap))
        assert lit[-1] == int((rows[0] != 0).sum())
        assert (h[sr.layout(W, lay.rows_per_rank, len(cams), cap).off_floats + 4 * cap:] == 0xA5).all(), "bytes behind the float array were written"
        shares.append(share); host.append(h)
    return shares, host, lit


def frames_against_the_oracle(sb, torch, scene, cams, refs, shares, host, W, lay, cap, what):
    """the expansion of the shares: RGBA32F against the oracle (and, bits and NaN payloads, against the restated expansion of the very
    same shares), both display modes against the one-device display pass"""
    H, G = lay.height, len(cams)
    counts = torch.zeros(lay.world, dtype=torch.int32, device="cuda")
    got = expand_gpu(sb, torch, shares, W, lay, cap, G, counts=counts).cpu().numpy()
    for f in range(G):
        assert_frames_identical(got[f], refs[f], f"{what} frame {f}")
    assert np.array_equal(got.view(np.uint32), sr.expand(host, sr.layout(W, lay.rows_per_rank, G, cap), lay, cap).view(np.uint32)), what
    assert [int(c) & 0xFFFFFFFF for c in counts.tolist()] == [sr.fields(h, sr.layout(W, lay.rows_per_rank, G, cap)).count for h in host]
    for flags in (sb.FLAG_DISPLAY, sb.FLAG_DISPLAY_DEBUG):
        got8 = as_rgba8(expand_gpu(sb, torch, shares, W, lay, cap, G, flags=flags))
        for f in range(G):
            ref8 = scene.DrawDisplay(cams[f], W, H, debug=flags == sb.FLAG_DISPLAY_DEBUG)
            assert np.array_equal(got8[f], ref8), f"{what} frame {f} flags {flags:#x}"


# ---- (a) what the march kernel writes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(333, 211), (129, 65)])
@pytest.mark.parametrize("world,weight", [(1, 1.0), (3, 1.0), (4, 0.6)])
def test_shares_of_the_march_kernel_field_by_field(sb, torch_mod, torus, oracle_frame, W, H, world, weight):
    torch = torch_mod
    lay = sb.tiles.BandLayout(H, world, 16, weight)
    for group in (("rotated", "closeup", "default"), ("sky",), ("sky", "lit", "sky"), ("closeup",)):
        cams = [view(n, W, H) for n in group]
        refs = [oracle_frame(n, W, H) for n in group]
        cap = lay.rows_per_rank * W * len(group)
        shares, host, lit = shares_against_the_oracle(sb, torch, torus, cams, refs, W, lay, cap)
        if group == ("sky",):
            # (asserted from the oracle's frame: all sky -- every mask 0, no atomic issued, the counter where it was)
            assert (sr.wire_of(refs[0])[1] > 140).all() and lit == [0] * world
            assert all(sr.fields(h, sr.layout(W, lay.rows_per_rank, 1, cap)).count == A5 for h in host)
        frames_against_the_oracle(sb, torch, torus, cams, refs, shares, host, W, lay, cap, f"{W}x{H} world {world} {group}")
    # every pixel of the frame lit (asserted from the oracle's frame), and a float array of exactly that many slots: used == capacity
    ref = oracle_frame("lit", W, H)
    a_bits, code = sr.wire_of(ref)
    assert (a_bits != 0).all() and (code <= 140).all()
    caps = [len(lay.rows_of(r)) * W for r in range(world)]
    shares, host, lit = shares_against_the_oracle(sb, torch, torus, [view("lit", W, H)], [ref], W, lay, caps, tail=4096)
    assert lit == caps
    # (expanded with the largest rank's capacity: no slot of a smaller share reaches its own)
    frames_against_the_oracle(sb, torch, torus, [view("lit", W, H)], [ref], shares, host, W, lay, max(caps),
                              f"{W}x{H} world {world}: every pixel lit, used == capacity")


def test_shares_carry_nan_greys_of_a_random_tree(sb, torch_mod, oracle_mod):
    # a random tree with random bytes under NaN-position cameras (as test_nan_coordinates_select_the_low_cells; the oracle's frames
    # of those are black, every grey +0, with no NaN in them), and under light strengths that make every lit grey a NaN, an
    # infinity, a negative number: the shares carry them.  Infinities and negative greys are held to the oracle's bits.  A NaN that
    # arithmetic made is a NaN in the march kernel's share where the oracle has one -- check_share and assert_frames_identical take
    # two NaNs for the same float, the rule of conftest.bits_equal -- and the EXPANSION is held to the payload: the frame against
    # share_restatement.expand of the very same shares, bit for bit (frames_against_the_oracle).
    torch = torch_mod
    W, H = 129, 65
    rng = np.random.default_rng(78)           # (that test's seed, 77, grows a tree that is its root alone: no grid, no sparse shares)
    s, v = _random_tree(rng, 5, p_split=0.75)
    assert len(s) > 10000 and (s[s[:, 0] >= 0][:, 0] > 0).any()                                  # five levels deep
    v = rng.integers(0, 256, size=v.shape, dtype=np.uint8)
    od = sb.OctData(s, v)
    cams = []
    for axes in ((0,), (0, 1, 2)):
        c = sb.Logic(W, H); c.Position = (0.3, 0.6, -0.2); c.Heading = (0.2, 0.4)
        for a in axes:
            c.State.position[a] = float("nan")
        cams.append(c)
    for strength in (float("nan"), float("inf"), -1.0, None):
        c = sb.Logic(W, H); c.Position = (0.3, 0.6, -0.2); c.Heading = (0.2, 0.4)
        if strength is not None:
            c.State.strength = strength
        cams.append(c)
    refs = [oracle_mod.render(s, v, c.State, W, H, nthreads=8)[0] for c in cams]
    assert np.isnan(refs[2][..., 0]).any() and np.isinf(refs[3][..., 0]).any() and (refs[4][..., 0] < 0).any()
    with sb.Scene(od) as scene:
        for world, weight in ((1, 1.0), (3, 1.0), (4, 0.6)):
            lay = sb.tiles.BandLayout(H, world, 16, weight)
            cap = lay.rows_per_rank * W * len(cams)
            shares, host, _ = shares_against_the_oracle(sb, torch, scene, cams, refs, W, lay, cap)
            frames_against_the_oracle(sb, torch, scene, cams, refs, shares, host, W, lay, cap, f"random tree, world {world}")


# ---- (b) the counter wraps -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", [0xFFFFFFFF, 0xFFFFFF00, "in the last tile"])
def test_share_counter_wraps(sb, torch_mod, torus, oracle_frame, preset):
    # header word 0 is never zeroed and runs on modulo 2^32 (one rank at 1080p wraps it every 2 000 frames): the tiles' bases, the
    # capacity test and the count must survive the wrap.  Two launches back to back on one share, the second told the first's count.
    torch = torch_mod
    W, H, world = 129, 65, 2
    group = ("rotated", "closeup", "default")
    cams = [view(n, W, H) for n in group]
    refs = [oracle_frame(n, W, H) for n in group]
    wire = sr.wire_of(np.stack(refs))
    lay = sb.tiles.BandLayout(H, world, 16)
    cap = lay.rows_per_rank * W * len(group)
    L = sr.layout(W, lay.rows_per_rank, len(group), cap)
    shares, host = [], []
    for r in range(world):
        rows = sr.rows_of_rank(wire, lay, r)
        total = int((rows[0] != 0).sum())
        assert total > 64
        first = ((1 << 32) - total + 1) if preset == "in the last tile" else preset          # (the last add of the launch crosses 2^32)
        share = new_share(torch, L.bytes, first)
        base = first
        for launch in range(2):
            render_share(sb, torch, torus, cams, W, lay, r, share, cap, base)
            torch.cuda.synchronize()
            h = share.cpu().numpy()
            assert sr.check_share(h, rows, base, cap) == total, (r, launch)
            base = (base + total) % (1 << 32)
            assert sr.fields(h, L).count == base
        assert base < first or preset == "in the last tile"                                   # it did wrap
        shares.append(share); host.append(h)
    frames_against_the_oracle(sb, torch, torus, cams, refs, shares, host, W, lay, cap, f"preset {preset}")


# ---- (c) a capacity below the lit pixels -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("cap_of", [1, 63, 64, "lit - 1", "lit", "lit + 1"])
def test_share_capacity_below_the_lit_pixels(sb, torch_mod, torus, oracle_frame, world, cap_of):
    # "slots beyond the capacity are dropped, and the count says so": nothing is written behind the float array, the header counts
    # every lit pixel, and a dropped pixel expands to a = 0 with its code kept
    torch = torch_mod
    W, H = 129, 65
    group = ("closeup", "default")
    cams = [view(n, W, H) for n in group]
    refs = [oracle_frame(n, W, H) for n in group]
    wire = sr.wire_of(np.stack(refs))
    lay = sb.tiles.BandLayout(H, world, 16)
    lit_last = int((sr.rows_of_rank(wire, lay, world - 1)[0] != 0).sum())                    # (from the oracle)
    assert lit_last > 65
    cap = cap_of if isinstance(cap_of, int) else lit_last + {"lit - 1": -1, "lit": 0, "lit + 1": 1}[cap_of]
    # (shares_against_the_oracle: 4 KiB of 0xA5 behind each share still 0xA5, floats[:min(lit, cap)] right, the count complete)
    shares, host, lit = shares_against_the_oracle(sb, torch, torus, cams, refs, W, lay, cap, tail=4096)
    assert lit[-1] == lit_last
    L = sr.layout(W, lay.rows_per_rank, len(group), cap)
    want = sr.expand([h[:L.bytes] for h in host], L, lay, cap)
    got = expand_gpu(sb, torch, shares, W, lay, cap, len(group)).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # ... which is the oracle's frame with the dropped pixels' grey at +0: step counts all there, min(lit, cap) greys per rank
    ref = np.stack(refs)
    assert np.array_equal(got[..., 3], ref[..., 3])
    kept = got.view(np.uint32)[..., 0] == ref.view(np.uint32)[..., 0]
    assert (got.view(np.uint32)[..., :3][~kept] == 0).all()
    sky = sr.wire_of(ref)[1] > 140
    assert int(((got.view(np.uint32)[..., 0] != 0) & ~sky).sum()) == sum(min(n, cap) for n in lit)
    for flags in (sb.FLAG_DISPLAY, sb.FLAG_DISPLAY_DEBUG):
        got8 = as_rgba8(expand_gpu(sb, torch, shares, W, lay, cap, len(group), flags=flags))
        for f in range(len(group)):
            ref8 = torus.DrawDisplay(cams[f], W, H, debug=flags == sb.FLAG_DISPLAY_DEBUG)
            dropped = ~kept[f]
            assert np.array_equal(got8[f][~dropped], ref8[~dropped])
            assert np.array_equal(got8[f][dropped][:, 3], ref8[dropped][:, 3])
            if flags == sb.FLAG_DISPLAY:
                assert (got8[f][dropped][:, :3] == 0).all()
            else:
                assert np.array_equal(got8[f][dropped], ref8[dropped])                       # (the heat map shows step counts only)


# ---- (d) the expansion of hand-built shares --------------------------------------------------------------------------------------
SPECIAL_BITS = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0x3F800000, 0x7FC00000, 0xFFC12345, 0x7F800001, 0xFF800000,
                         0x3F7FFFFF, 0x3F800001, 0x00800000, 0xBF800000], dtype=np.uint32)         # -0, denormals, infinities, NaNs with payloads, 1 and its neighbours


def random_share(rng, L, cap):
    ft = L.frames * L.tiles

    def r64():
        return rng.integers(0, 1 << 32, size=ft, dtype=np.uint64) << np.uint64(32) | rng.integers(0, 1 << 32, size=ft, dtype=np.uint64)

    kind = rng.integers(0, 4, size=ft)                   # an empty mask, a full one, a random one, a sparse random one
    forced = rng.permutation(ft)[:6]
    kind[forced] = 1
    masks = r64()
    masks[kind == 3] &= r64()[kind == 3] & r64()[kind == 3]
    masks[kind == 0] = 0
    masks[kind == 1] = np.uint64(0xFFFFFFFFFFFFFFFF)
    bases = rng.integers(0, cap + 100, size=ft).astype(np.uint32)
    # the edges of the float array: full tiles whose pixels take the slots capacity - 1 and capacity, that end at capacity - 1, that
    # start at the capacity and behind it, whose slots run over 2^32 into the array's first 48 (base + popcount is uint32 arithmetic),
    # and far behind it
    for t, base in zip(forced, (cap - 1, max(cap - 64, 0), cap, cap + 1, 0xFFFFFFF0, 0x7FFFFFF0)):
        bases[t] = base
    codes = rng.integers(0, 256, size=(ft, 64), dtype=np.uint8)
    floats = rng.integers(0, 1 << 32, size=cap, dtype=np.uint32)
    where = rng.random(cap) < 0.2
    floats[where] = SPECIAL_BITS[rng.integers(0, len(SPECIAL_BITS), size=int(where.sum()))]
    floats[:48] = np.resize(SPECIAL_BITS, 48)            # (the slots of the tile that wraps: every special pattern on a lit pixel)
    return sr.assemble(L, int(rng.integers(0, 1 << 32)), masks, bases, codes, floats)


@pytest.fixture(scope="module")
def sky8(torus):
    px = torus.DrawDisplay(view("sky", 16, 16), 16, 16)
    assert (px == px[0, 0]).all()
    return px[0, 0, :3].copy()


@pytest.mark.parametrize("W,H,world,band_rows,frames,deal", [
    (1, 40, 1, 8, 1, "round robin"), (7, 211, 2, 16, 8, "round robin"), (9, 130, 5, 8, 1, "owner"), (333, 211, 16, 8, 1, "round robin"),
    (333, 200, 2, 64, 8, "owner"), (9, 211, 16, 8, 8, "owner"), (333, 64, 5, 16, 1, "round robin"), (7, 100, 1, 64, 8, "round robin")])
def test_expansion_of_arbitrary_shares(sb, torch_mod, sky8, oracle_mod, W, H, world, band_rows, frames, deal):
    torch = torch_mod
    # pow(-inf, 1 / 2.2) is +inf (C and IEEE 754 pow: y > 0 and no odd integer), so the display pass of the oracle shows a grey of
    # -inf as it shows +inf; every other value <= 0, and NaN, is 0
    grey_of_minus_inf = int(oracle_mod.display(np.array([[[-np.inf, -np.inf, -np.inf, 1.0]]], dtype=np.float32))[0, 0, 0])
    assert grey_of_minus_inf == 255
    rng = np.random.default_rng(W * 1000 + H + world)
    n_bands = (H + band_rows - 1) // band_rows
    owner = None
    if deal == "owner":
        owner = np.concatenate((rng.permutation(world)[:n_bands], rng.integers(0, world, size=max(n_bands - world, 0)))).tolist() \
            if n_bands >= world else None
        assert owner is not None and set(owner) == set(range(world))
    lay = sb.tiles.BandLayout(H, world, band_rows, owner=owner)
    cap = max(200, lay.rows_per_rank * W * frames // 3)
    L = sr.layout(W, lay.rows_per_rank, frames, cap)
    host = [random_share(rng, L, cap) for _ in range(world)]
    shares = [torch.from_numpy(h).cuda() for h in host]
    want = sr.expand(host, L, lay, cap)
    for only_rank in (-1, 0, world - 1):
        mine = np.array([lay.source_of(y)[0] == only_rank or only_rank < 0 for y in range(H)])
        out = torch.full((frames, H, W, 4), float("nan"), dtype=torch.float32, device="cuda")          # the canary
        counts = torch.full((world,), 0x12345678, dtype=torch.int32, device="cuda")
        given = [s if only_rank < 0 or r == only_rank else None for r, s in enumerate(shares)]      # a null pointer for the others
        got = expand_gpu(sb, torch, given, W, lay, cap, frames, only_rank=only_rank, out=out, counts=counts).cpu().numpy()
        assert np.array_equal(got.view(np.uint32)[:, mine], want.view(np.uint32)[:, mine]), f"only_rank {only_rank}"
        assert (got.view(np.uint32)[:, ~mine] == np.array([float("nan")], dtype=np.float32).view(np.uint32)[0]).all(), "another rank's rows were written"
        for r in range(world):
            assert (int(counts[r]) & 0xFFFFFFFF) == (sr.fields(host[r], L).count if given[r] is not None else 0x12345678), (only_rank, r)
        # the display modes: what can be stated exactly without restating fp32 powf
        if not mine.any():
            continue
        wa, wc = zip(*[sr.decode(h, L) for h in host])
        src = [lay.source_of(y) for y in range(H)]
        a = np.stack([wa[r][:, l] for r, l in src], axis=1).view(np.float32)       # [frames][H][W]: the pixels' a and code
        code = np.stack([wc[r][:, l] for r, l in src], axis=1).astype(np.int64)
        steps = np.where(code > 140, 255 - code, code)
        skyc = code > 140
        if only_rank < 0:
            # the special patterns did reach lit pixels: a NaN, a -0.0, a denormal, both infinities
            lit_bits = a.view(np.uint32)[a.view(np.uint32) != 0]
            assert np.isnan(lit_bits.view(np.float32)).any() and (lit_bits == 0x80000000).any() and np.isin(lit_bits, (0x00000001, 0x807FFFFF)).any()
            assert (lit_bits == 0x7F800000).any() and (lit_bits == 0xFF800000).any()
        for flags in (sb.FLAG_DISPLAY, sb.FLAG_DISPLAY_DEBUG):
            out8 = torch.full((frames, H, W), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            got8 = as_rgba8(expand_gpu(sb, torch, given, W, lay, cap, frames, flags=flags, only_rank=only_rank, out=out8))
            assert (got8[:, ~mine] == 0x5A).all()
            g8, st, sk, av = got8[:, mine], steps[:, mine], skyc[:, mine], a[:, mine]
            assert (g8[..., 0] == g8[..., 1])[~sk].all() and (g8[..., 1] == g8[..., 2])[~sk].all()
            if flags == sb.FLAG_DISPLAY:
                assert np.array_equal(g8[..., 3] == 0xFF, st >= 1) and np.isin(g8[..., 3], (0, 0xFF)).all()
                assert (g8[sk][:, :3] == sky8).all()
                grey, av = g8[..., 0][~sk].astype(np.int64), av[~sk]
                assert (grey[np.isnan(av) | ((av <= 0) & ~np.isneginf(av))] == 0).all() and (grey[av >= 1] == 255).all()
                assert (grey[np.isneginf(av)] == grey_of_minus_inf).all()
                mid = np.isfinite(av) & (av >= 0) & (av <= 1)
                assert mid.sum() > 3 or W * H < 100
                assert (np.diff(grey[mid][np.argsort(av[mid], kind="stable")]) >= 0).all()
            else:
                # float4(1, 1, 1, 0) * steps / 140: three equal channels that never decrease with the step count, alpha 0
                assert (g8[..., 0] == g8[..., 1]).all() and (g8[..., 1] == g8[..., 2]).all() and (g8[..., 3] == 0).all()
                heat = g8[..., 0].astype(np.int64)
                assert (heat[st == 0] == 0).all() and (heat[st >= 140] == 255).all()
                assert (np.diff(heat.ravel()[np.argsort(st.ravel(), kind="stable")]) >= 0).all()
                by_steps = {int(n): set(heat[st == n].tolist()) for n in np.unique(st)}
                assert all(len(vals) == 1 for vals in by_steps.values())


# ---- (e) more than 512 bands: the per-pixel kernels ------------------------------------------------------------------------------
@pytest.mark.parametrize("H,world", [(4160, 2), (4160, 3), (4149, 2)])
def test_frames_of_more_than_512_bands(sb, torch_mod, torus, oracle_frame, H, world):
    # 24 x 4160 with 8-row bands: 520 bands (519 with a ragged last one), more than the band map holds -- the expansion falls back
    # to k_deinterleave_sparse2, the dense reorder to k_deinterleave
    torch = torch_mod
    W, band_rows = 24, 8
    group = ("default", "closeup")
    cams = [view(n, W, H) for n in group]
    refs = [oracle_frame(n, W, H) for n in group]
    lay = sb.tiles.BandLayout(H, world, band_rows)
    assert lay.n_bands > 512 and (H == 4160 or lay.n_bands == 519)
    cap = lay.rows_per_rank * W * len(group)
    shares, host, _ = shares_against_the_oracle(sb, torch, torus, cams, refs, W, lay, cap)
    frames_against_the_oracle(sb, torch, torus, cams, refs, shares, host, W, lay, cap, f"{W}x{H} over {world}")
    out = torch.full((len(group), H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    got = expand_gpu(sb, torch, [None, shares[1]] + [None] * (world - 2), W, lay, cap, len(group), only_rank=1, out=out).cpu().numpy()
    mine = np.array([lay.source_of(y)[0] == 1 for y in range(H)])
    assert np.array_equal(got.view(np.uint32)[:, mine], np.stack(refs).view(np.uint32)[:, mine]) and np.isnan(got[:, ~mine]).all()
    # the dense pair: sdfhip_render_bands_device + sdfhip_deinterleave_device
    st = torch.cuda.current_stream().cuda_stream
    for frames in (1, 2):
        for px, flags in ((16, 0), (4, sb.FLAG_DISPLAY)):
            shape = (world, frames, lay.rows_per_rank, W)
            gathered = torch.full(shape + (4,), float("nan"), dtype=torch.float32, device="cuda") if px == 16 else \
                torch.full(shape, 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            for r in range(world):
                torus.DrawBandsDevice(cams[:frames], W, H, gathered[r].data_ptr(), band_rows, lay.bands_of(r), nrows_out=lay.rows_per_rank,
                                      flags=flags, stream=st)
            frame = torch.zeros((frames, H, W, 4) if px == 16 else (frames, H, W), dtype=gathered.dtype, device="cuda")
            sb.tiles.deinterleave(0, gathered.data_ptr(), frame.data_ptr(), W, lay, stream=st, pixel_bytes=px, frames=frames)
            torch.cuda.synchronize()
            for f in range(frames):
                if px == 16:
                    assert_frames_identical(frame[f].cpu().numpy(), refs[f], f"dense {W}x{H} over {world}, frame {f} of {frames}")
                else:
                    assert np.array_equal(as_rgba8(frame[f]), torus.DrawDisplay(cams[f], W, H)), (H, world, frames, f)


# ---- (f) bands that are not whole tile rows --------------------------------------------------------------------------------------
@pytest.mark.parametrize("band_rows", [4, 12, 20])
def test_bands_that_are_not_whole_tile_rows(sb, torch_mod, torus, scenes, oracle_frame, band_rows):
    # PINNED: the direct API renders such shares correctly -- a tile of a share is 8 rows of the SHARE, which then straddle two
    # bands of the frame (the march kernel maps every local row to its frame row by itself; the expansion walks a band's rows and
    # reloads the tile's mask when it enters the next tile row).  Only sdfhip_multi_configure asks for multiples of 8.
    torch = torch_mod
    W, H, world = 333, 211, 3
    group = ("rotated", "closeup", "default")
    cams = [view(n, W, H) for n in group]
    refs = [oracle_frame(n, W, H) for n in group]
    for weight in (1.0, 0.6):
        lay = sb.tiles.BandLayout(H, world, band_rows, weight)
        cap = lay.rows_per_rank * W * len(group)
        shares, host, _ = shares_against_the_oracle(sb, torch, torus, cams, refs, W, lay, cap)
        frames_against_the_oracle(sb, torch, torus, cams, refs, shares, host, W, lay, cap, f"{band_rows}-row bands, weight {weight}")
        # the dense pair
        st = torch.cuda.current_stream().cuda_stream
        gathered = torch.full((world, len(group), lay.rows_per_rank, W, 4), float("nan"), dtype=torch.float32, device="cuda")
        for r in range(world):
            sb.tiles.render_bands_batch(torus, cams, W, lay, r, gathered[r].data_ptr(), stream=st)
        frame = torch.zeros((len(group), H, W, 4), dtype=torch.float32, device="cuda")
        sb.tiles.deinterleave(0, gathered.data_ptr(), frame.data_ptr(), W, lay, stream=st, frames=len(group))
        torch.cuda.synchronize()
        for f in range(len(group)):
            assert_frames_identical(frame[f].cpu().numpy(), refs[f], f"dense, {band_rows}-row bands, weight {weight}, frame {f}")
    with sb.MultiScene(scenes["sphere_d4"], [0, 0]) as ms:
        with pytest.raises(sb.SdfHipError) as e:
            ms.configure(band_rows=band_rows)
        assert e.value.code == sb._lib.ERR_ARG and "multiple of 8" in str(e.value)


# ---- (g) the resend as the product meets it --------------------------------------------------------------------------------------
# (The subtraction h_counts - count_base of the wait under a WRAPPED counter cannot be reached through the handle without rendering
# 2^32 floats: the kernel side of the wrap is test_share_counter_wraps above, the host side is one unsigned subtraction.)
def copy_out(torch, ptr, shape, dtype):
    frames = torch.empty(shape, dtype=dtype, device="cuda")
    hip = ctypes.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(ctypes.c_void_p(frames.data_ptr()), ctypes.c_void_p(ptr), ctypes.c_size_t(frames.numel() * frames.element_size()), 3) == 0
    return frames.cpu().numpy()


@pytest.mark.parametrize("band_rows,weight,flags", [(16, 1.0, 0), (16, 1.0, "display"), (8, 0.5, 0)])
def test_tail_resend_when_the_camera_turns_from_sky_to_object(sb, torus, scenes, oracle_frame, band_rows, weight, flags):
    W, H, world = 256, 192, 3
    flags = sb.FLAG_DISPLAY if flags == "display" else 0
    sky, near = view("sky", W, H), view("near", W, H)
    ref_sky, ref_near = oracle_frame("sky", W, H), oracle_frame("near", W, H)
    assert (sr.wire_of(ref_sky)[1] > 140).all()                                           # frame 1 is all sky
    lay = sb.tiles.BandLayout(H, world, band_rows, weight)
    wire = sr.wire_of(ref_near[None])
    lit = [int((sr.rows_of_rank(wire, lay, r)[0] != 0).sum()) for r in range(world)]
    # after an empty frame a share travels with 1024 floats (the estimate: used * 1.25 + 1024, in steps of 1024): frame 2 lights more
    assert all(n > 1024 and n > 1.25 * 0 + 2047 for n in lit[1:]), lit
    fixed = sr.layout(W, lay.rows_per_rank, 1, 0).off_floats
    full = lay.rows_per_rank * W * 4

    def same(got, ref, cam, what):
        if flags:
            assert got.dtype == np.uint8 and np.array_equal(got, torus.DrawDisplay(cam, W, H)), what
        else:
            assert_frames_identical(got, ref, what)

    with sb.MultiScene(scenes["torus_d6"], [0] * world) as ms:
        ms.configure(band_rows=band_rows, rank0_weight=weight)
        img, st = ms.Draw(sky, W, H, flags=flags, want_stats=True)
        same(img, ref_sky, sky, "the sky frame")
        assert list(st.floats_used)[:world] == [0] * world and st.resends == 0
        img, st = ms.Draw(near, W, H, flags=flags, want_stats=True)
        assert st.resends == world - 1                                                    # on both flavours: no laboratory hook
        same(img, ref_near, near, "the close-up behind a sky frame: float tails sent again")
        assert list(st.floats_used)[:world] == lit
        assert st.gathered_bytes >= sum(fixed + 4 * n for n in lit[1:])
        img, st = ms.Draw(near, W, H, flags=flags, want_stats=True)
        assert st.resends == 0 and list(st.floats_used)[:world] == lit
        same(img, ref_near, near, "the same camera again")
        assert sum(fixed + 4 * n for n in lit[1:]) <= st.gathered_bytes < (world - 1) * full


def test_tail_resend_in_four_slots_and_changing_groups(sb, torch_mod, scenes, oracle_frame):
    torch = torch_mod
    W, H, world = 256, 192, 3
    refs = {n: oracle_frame(n, W, H) for n in ("sky", "near", "closeup", "rotated")}
    cams = {n: view(n, W, H) for n in refs}
    with sb.MultiScene(scenes["torus_d6"], [0] * world) as ms:
        assert_frames_identical(ms.Draw(cams["sky"], W, H), refs["sky"], "the sky frame")
        # all four slots submitted before any is waited for: all four travel with the stale estimate
        for slot in range(4):
            ms.Submit(slot, cams["near"], W, H)
        resends = 0
        for slot in range(4):
            ptr, st = ms.Wait(slot, want_stats=True)
            resends += st.resends
            assert_frames_identical(copy_out(torch, ptr, (H, W, 4), torch.float32), refs["near"], f"slot {slot}")
        assert resends >= 2
        # one slot, groups of changing size: the share's layout changes under a counter that runs on
        groups = (("sky", "near", "closeup", "sky"), ("near",), ("sky", "closeup", "near", "rotated", "sky", "sky", "near", "closeup"),
                  ("closeup", "sky", "near"))
        for k, group in enumerate(groups):
            ms.Submit(1, [cams[n] for n in group], W, H)
            got = copy_out(torch, ms.Wait(1), (len(group), H, W, 4), torch.float32)
            for f, n in enumerate(group):
                assert_frames_identical(got[f], refs[n], f"group {k} frame {f} ({n})")

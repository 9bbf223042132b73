"""The sparse wire share's restatement (tests/share_restatement.py) held to the library's own layout, to oracle frames and to
itself: what tests/test_gpu_share.py checks the GPU's shares with must accept a correct share, give the frame back bit for bit,
and reject every kind of defect it is there to catch.  No GPU."""
import numpy as np
import pytest

import share_restatement as sr
from conftest import assert_frames_identical, make_camera


def test_layout_is_the_library_s(sb):
    L = sb._lib.lib
    for width in (1, 7, 8, 9, 333, 3840):
        for rows in (1, 8, 9, 272):
            for frames in (1, 3, 8):
                for capacity in (1, 4321, width * rows * frames):
                    lay = sr.layout(width, rows, frames, capacity)
                    assert lay.bytes == L.sdfhip_sparse2_bytes(width, rows, frames, capacity), (width, rows, frames, capacity)
                    assert lay.off_floats == L.sdfhip_sparse2_floats_offset(width, rows, frames), (width, rows, frames)
                    assert (lay.tiles_x, lay.tiles_y) == ((width + 7) // 8, (rows + 7) // 8)
                    assert 64 == lay.off_masks < lay.off_bases < lay.off_codes < lay.off_floats < lay.bytes
                    assert lay.off_codes % 64 == 0 and lay.bytes % 64 == 0 and lay.bytes - lay.off_floats >= 4 * capacity


@pytest.fixture(scope="module")
def oracle_frames(oracle_mod, scenes):
    out = {}
    for sname in ("sphere_d4", "torus_d6"):
        od = scenes[sname]
        for (W, H) in ((129, 65), (333, 211)):
            fr = np.stack([oracle_mod.render(od.Structs, od.Values, make_camera(n, W, H).State, W, H, nthreads=8)[0]
                           for n in ("rotated", "closeup", "default")])
            fr.setflags(write=False)
            out[sname, W, H] = fr
    return out


@pytest.mark.parametrize("world,weight", [(1, 1.0), (3, 1.0), (4, 0.6)])
def test_round_trip_of_oracle_frames(sb, oracle_frames, world, weight):
    rng = np.random.default_rng(11)
    for (sname, W, H), frames in oracle_frames.items():
        wire = sr.wire_of(frames)
        # wire_of and wire_expand are each other's inverse on a frame the renderer can write
        assert np.array_equal(sr.wire_expand(*wire), frames.view(np.uint32))
        lay = sb.tiles.BandLayout(H, world, 16, weight)
        cap = lay.rows_per_rank * W * len(frames)
        L = sr.layout(W, lay.rows_per_rank, len(frames), cap)
        shares, total = [], 0
        for r in range(world):
            rows = sr.rows_of_rank(wire, lay, r)
            base = int(rng.integers(0, 1 << 32))
            share = sr.encode(rows, cap, base, rng)
            assert share.size == L.bytes
            total += sr.check_share(share, rows, base, cap)
            shares.append(share)
        assert total == int((wire[0] != 0).sum())
        got = sr.expand(shares, L, lay, cap)
        for f in range(len(frames)):
            assert_frames_identical(got[f], frames[f], f"{sname} {W}x{H} world {world} frame {f}")
        assert np.array_equal(got.view(np.uint32), frames.view(np.uint32))          # (NaN payloads included)
        # one rank's rows only: the others keep what was there
        canary = np.full_like(got, np.nan)
        sr.expand([s if r == world - 1 else None for r, s in enumerate(shares)], L, lay, cap, only_rank=world - 1, out=canary)
        mine = np.array([lay.source_of(y)[0] == world - 1 for y in range(H)])
        assert np.array_equal(canary.view(np.uint32)[:, mine], frames.view(np.uint32)[:, mine]) and np.isnan(canary[:, ~mine]).all()


def test_capacity_drops_the_slots_behind_it(sb, oracle_frames):
    frames = oracle_frames["torus_d6", 129, 65][1:2]
    wire = sr.wire_of(frames)
    lay = sb.tiles.BandLayout(65, 1, 16)
    rows = sr.rows_of_rank(wire, lay, 0)
    lit = int((wire[0] != 0).sum())
    assert lit > 64
    for cap in (1, 63, lit - 1, lit, lit + 1):
        share = sr.encode(rows, cap, 0xFFFFFFF0, np.random.default_rng(cap))
        assert sr.check_share(share, rows, 0xFFFFFFF0, cap) == lit                  # (the header counts every lit pixel, and wraps)
        a, code = sr.decode(share, sr.layout(129, lay.rows_per_rank, 1, cap))
        assert np.array_equal(code, rows[1]) and int((a != 0).sum()) == min(lit, cap)
        assert ((a == rows[0]) | (a == 0)).all()


def test_check_share_rejects_what_it_is_there_to_catch(sb, oracle_frames):
    frames = oracle_frames["torus_d6", 129, 65]
    lay = sb.tiles.BandLayout(65, 2, 16)
    rows = sr.rows_of_rank(sr.wire_of(frames), lay, 1)
    cap = lay.rows_per_rank * 129 * len(frames)
    L = sr.layout(129, lay.rows_per_rank, len(frames), cap)
    base = 0xFFFFFF00
    good = sr.encode(rows, cap, base, np.random.default_rng(3))
    sr.check_share(good, rows, base, cap)
    lit_tiles = np.nonzero(sr.fields(good, L).masks)[0]
    assert lit_tiles.size >= 2

    def planted(defect):
        bad = good.copy()
        F = sr.fields(bad, L)
        if defect == "bases":                       # two tiles' bases swapped: their intervals overlap others or leave gaps
            i, j = [int(t) for t in lit_tiles[:2]]
            pi, pj = bin(int(F.masks[i])).count("1"), bin(int(F.masks[j])).count("1")
            if pi == pj:                            # (equal sizes swap harmlessly: both onto one base instead)
                F.bases[j] = F.bases[i]
            else:
                F.bases[i], F.bases[j] = F.bases[j], F.bases[i]
        elif defect == "mask":
            F.masks[int(lit_tiles[0])] ^= np.uint64(1) << np.uint64(17)
        elif defect == "code":
            F.codes[int(lit_tiles[1]), 5] ^= 1
        elif defect == "header":
            bad[:4].view(np.uint32)[0] += 1
        elif defect == "float":
            F.floats[int(F.bases[int(lit_tiles[0])])] ^= 1
        return bad

    for defect, word in (("bases", "slot intervals"), ("mask", "tile masks"), ("code", "code bytes"), ("header", "header word 0"),
                         ("float", "floats differ")):
        with pytest.raises(AssertionError, match=word):
            sr.check_share(planted(defect), rows, base, cap)
    with pytest.raises(AssertionError, match="header word 0"):
        sr.check_share(good, rows, base + 1, cap)                                    # the wrong count_base
    # and wire_of refuses a frame the wire format cannot hold
    for ch, val in ((3, 141.0), (1, 0.5)):
        f = frames[0].copy()
        grey = np.argwhere(sr.wire_of(f)[1] <= 140)[0]
        f[grey[0], grey[1], ch] = val
        with pytest.raises(AssertionError):
            sr.wire_of(f)

"""The sparse wire share in numpy, restated from the comment block "sparse wire shares" of include/sdfhip.h and from
Sparse2Layout -- not a translation of the kernels.  A plain helper module (like the other *_restatement.py files), shared by
tests/test_share.py (CPU) and tests/test_gpu_share.py.

One share holds the `frames` frames of one launch of one rank, `rows` x `width` pixels each (the rank's bands, in increasing
band order), cut into 8x8 tiles in row-major tile order; bit (y & 7) * 8 + (x & 7) of a tile is pixel (x, y):

    header   64 bytes; word 0 = float slots handed out, running on modulo 2^32 from the value the launch was told
    masks    [frames][tiles] uint64   bit set = the pixel's `a` has any bit set (it is "lit")
    bases    [frames][tiles] uint32   slot of the tile's first lit pixel; its other lit pixels follow in bit order
    codes    [frames][tiles][64] uint8   (starts on a multiple of 64 bytes)
    floats   [capacity] float32       a slot >= capacity is dropped: such a pixel reads a = +0

A pixel is (a, code): code <= 140 is the grey (a, a, a, code steps), a larger code the sky constant with 255 - code steps.
"""
from types import SimpleNamespace

import numpy as np

SKY_BITS = np.array([0.005, 0.01, 0.2], dtype=np.float32).view(np.uint32)
MAX_STEPS, MAX_SKY_STEPS = 140, 100


def layout(width, rows, frames, capacity):
    tiles_x, tiles_y = (width + 7) // 8, (rows + 7) // 8
    ft = frames * tiles_x * tiles_y
    off_masks = 64
    off_bases = off_masks + 8 * ft
    off_codes = (off_bases + 4 * ft + 63) // 64 * 64
    off_floats = off_codes + 64 * ft
    return SimpleNamespace(width=width, rows=rows, frames=frames, capacity=capacity, tiles_x=tiles_x, tiles_y=tiles_y,
                           tiles=tiles_x * tiles_y, off_masks=off_masks, off_bases=off_bases, off_codes=off_codes, off_floats=off_floats,
                           bytes=(off_floats + 4 * capacity + 63) // 64 * 64)


def wire_of(frame):
    """RGBA32F frame (..., H, W, 4) -> (a_bits uint32, code uint8) per pixel; asserts that the frame is representable."""
    bits = np.ascontiguousarray(frame, dtype=np.float32).view(np.uint32)
    steps = np.asarray(frame, dtype=np.float32)[..., 3]
    assert (steps == np.floor(steps)).all() and (steps >= 0).all() and (steps <= MAX_STEPS).all(), "step counts must be whole numbers in 0..140"
    n = steps.astype(np.int64)
    sky = (bits[..., 0] == SKY_BITS[0]) & (bits[..., 1] == SKY_BITS[1]) & (bits[..., 2] == SKY_BITS[2])
    assert (n[sky] <= MAX_SKY_STEPS).all(), "a sky pixel has at most 100 steps"
    grey = ~sky
    assert ((bits[..., 0] == bits[..., 1]) & (bits[..., 1] == bits[..., 2]))[grey].all(), "a pixel that is not sky must be a grey (r, g, b bit-equal)"
    a_bits = np.where(sky, np.uint32(0), bits[..., 0])
    code = np.where(sky, 255 - n, n).astype(np.uint8)
    return a_bits, code


def rows_of_rank(wire, band_layout, rank):
    """The wire pixels (a_bits, code) of frames [F][H][W] -> those of `rank`'s rows in share order [F][rows_per_rank][W]:
    band_layout.bands_of(rank) one after the other; rows past the frame or past the rank's bands are a = +0, code 0."""
    a_bits, code = wire
    F, H, W = a_bits.shape
    out_a = np.zeros((F, band_layout.rows_per_rank, W), dtype=np.uint32)
    out_c = np.zeros((F, band_layout.rows_per_rank, W), dtype=np.uint8)
    for lb, b in enumerate(band_layout.bands_of(rank)):
        y0 = b * band_layout.band_rows
        n = min(band_layout.band_rows, H - y0)
        out_a[:, lb * band_layout.band_rows:lb * band_layout.band_rows + n] = a_bits[:, y0:y0 + n]
        out_c[:, lb * band_layout.band_rows:lb * band_layout.band_rows + n] = code[:, y0:y0 + n]
    return out_a, out_c


def _to_tiles(x, L):
    """[F][rows][W] -> [F * tiles][64] in tile order, padded with zeros"""
    F = x.shape[0]
    p = np.zeros((F, L.tiles_y * 8, L.tiles_x * 8), dtype=x.dtype)
    p[:, :x.shape[1], :x.shape[2]] = x
    return p.reshape(F, L.tiles_y, 8, L.tiles_x, 8).transpose(0, 1, 3, 2, 4).reshape(F * L.tiles, 64)


def _from_tiles(t, L):
    """the inverse: [F * tiles][64] -> [F][rows][W]"""
    F = t.shape[0] // L.tiles
    p = t.reshape(F, L.tiles_y, L.tiles_x, 8, 8).transpose(0, 1, 3, 2, 4).reshape(F, L.tiles_y * 8, L.tiles_x * 8)
    return p[:, :L.rows, :L.width]


_BIT = np.uint64(1) << np.arange(64, dtype=np.uint64)


def _pack(lit):
    return (lit.astype(np.uint64) * _BIT).sum(axis=1, dtype=np.uint64)


def _unpack(masks):
    return ((masks[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def fields(share, L):
    """views of a share's arrays (share: uint8 array of at least L.bytes bytes)"""
    share = np.asarray(share, dtype=np.uint8)
    ft = L.frames * L.tiles
    return SimpleNamespace(count=int(share[:4].view(np.uint32)[0]),
                           masks=share[L.off_masks:L.off_masks + 8 * ft].view(np.uint64),
                           bases=share[L.off_bases:L.off_bases + 4 * ft].view(np.uint32),
                           codes=share[L.off_codes:L.off_codes + 64 * ft].reshape(ft, 64),
                           floats=share[L.off_floats:L.off_floats + 4 * L.capacity].view(np.uint32))


def assemble(L, count, masks, bases, codes, floats, fill=0xA5, tail=0):
    """a share from its arrays; every byte the format does not define (header words 1..15, padding) is `fill`, and `tail`
    more bytes of it follow the share"""
    share = np.full(L.bytes + tail, fill, dtype=np.uint8)
    F = fields(share, L)
    share[:4].view(np.uint32)[0] = count & 0xFFFFFFFF
    F.masks[:] = masks
    F.bases[:] = bases
    F.codes[:] = codes
    F.floats[:] = floats[:L.capacity]
    return share


def encode(rows, capacity, count_base, rng=None, fill=0xA5):
    """The numpy encoder: (a_bits, code) [F][rows][W] -> a share.  The tiles take their slots in the order `rng` shuffles them
    into (None: tile order), counting on from `count_base`."""
    a_bits, code = rows
    F, R, W = a_bits.shape
    L = layout(W, R, F, capacity)
    a, c = _to_tiles(a_bits, L), _to_tiles(code, L)
    lit = a != 0
    pop = lit.sum(axis=1)
    order = np.arange(len(pop)) if rng is None else rng.permutation(len(pop))
    start = np.zeros(len(pop), dtype=np.int64)
    start[order] = np.cumsum(pop[order]) - pop[order]
    total = int(pop.sum())
    floats = np.full(max(capacity, total), int(fill) * 0x01010101, dtype=np.uint32)
    slot = start[:, None] + np.cumsum(lit, axis=1) - 1
    floats[slot[lit]] = a[lit]
    return assemble(L, count_base + total, _pack(lit), np.where(pop > 0, start, 0).astype(np.uint32), c, floats, fill=fill)


def check_share(share_bytes, expected_rows, count_base, capacity):
    """Asserts that `share_bytes` is a share of the expected wire pixels (a_bits, code) [F][rows][W] -- whatever order the
    tiles took their slots in.  Two NaNs count as the same float (the rule of conftest.bits_equal: the payload of a NaN that
    arithmetic made is not the oracle's to pin); every other float is compared by its bits."""
    a_bits, code = expected_rows
    F, R, W = a_bits.shape
    L = layout(W, R, F, capacity)
    S = fields(share_bytes, L)
    a, c = _to_tiles(a_bits, L), _to_tiles(code, L)
    lit = a != 0
    want = _pack(lit)
    bad = np.nonzero(S.masks != want)[0]
    assert bad.size == 0, f"{bad.size} tile masks differ; first: frame-tile {int(bad[0])} has {int(S.masks[bad[0]]):#018x}, expected {int(want[bad[0]]):#018x}"
    bad = np.argwhere(S.codes != c)
    assert bad.size == 0, f"{len(bad)} code bytes differ; first: frame-tile {int(bad[0][0])} bit {int(bad[0][1])} has {int(S.codes[tuple(bad[0])])}, expected {int(c[tuple(bad[0])])}"
    pop = lit.sum(axis=1)
    total = int(pop.sum())
    tiles = np.nonzero(pop)[0]
    bases = S.bases.astype(np.int64)
    by_base = tiles[np.argsort(bases[tiles], kind="stable")]
    ends = np.concatenate(([0], bases[by_base] + pop[by_base]))
    gaps = np.nonzero(bases[by_base] != ends[:-1])[0]
    assert gaps.size == 0, (f"the tiles' slot intervals do not tile [0, {total}): frame-tile {int(by_base[gaps[0]])} starts at "
                            f"{int(bases[by_base[gaps[0]]])}, the interval before it ends at {int(ends[gaps[0]])}")
    assert int(ends[-1]) == total, f"the slot intervals end at {int(ends[-1])}, {total} pixels are lit"
    assert S.count == (count_base + total) % (1 << 32), f"header word 0 is {S.count:#x}, expected ({count_base:#x} + {total}) mod 2^32 = {(count_base + total) % (1 << 32):#x}"
    slot = bases[:, None] + np.cumsum(lit, axis=1) - 1
    kept = lit & (slot < capacity)
    got, exp = S.floats[slot[kept]], a[kept]
    same = (got == exp) | (np.isnan(got.view(np.float32)) & np.isnan(exp.view(np.float32)))
    assert same.all(), f"{int((~same).sum())} floats differ; first: slot {int(slot[kept][~same][0])} holds {int(got[~same][0]):#010x}, expected {int(exp[~same][0]):#010x}"
    return total


def decode(share, L):
    """a share -> the wire pixels (a_bits, code) [F][rows][W] it stands for: a = +0 where the pixel's slot >= capacity"""
    S = fields(share, L)
    lit = _unpack(S.masks)
    slot = (S.bases.astype(np.int64)[:, None] + np.cumsum(lit, axis=1) - 1) & 0xFFFFFFFF          # (uint32 arithmetic)
    kept = lit & (slot < L.capacity)
    a = np.zeros(lit.shape, dtype=np.uint32)
    a[kept] = S.floats[slot[kept]]
    return _from_tiles(a, L), _from_tiles(S.codes, L)


def wire_expand(a_bits, code):
    """(a, code) -> RGBA32F pixels, as uint32 bits (..., 4)"""
    sky = code > MAX_STEPS
    out = np.empty(a_bits.shape + (4,), dtype=np.uint32)
    for ch in range(3):
        out[..., ch] = np.where(sky, SKY_BITS[ch], a_bits)
    out[..., 3] = np.where(sky, 255 - code.astype(np.int64), code).astype(np.float32).view(np.uint32)
    return out


def expand(shares, L, band_layout, capacity, only_rank=None, out=None):
    """The ranks' shares -> frames [F][H][W][4] float32.  only_rank: that rank's rows only; the other rows keep what `out`
    holds (and the other shares may be None)."""
    assert L.capacity == capacity
    H = band_layout.height
    if out is None:
        assert only_rank is None
        out = np.zeros((L.frames, H, L.width, 4), dtype=np.float32)
    bits = out.view(np.uint32)
    src = [band_layout.source_of(y) for y in range(H)]
    for r in range(band_layout.world):
        if only_rank is not None and r != only_rank:
            continue
        ys = np.array([y for y in range(H) if src[y][0] == r], dtype=np.int64)
        if ys.size == 0:
            continue
        a, c = decode(shares[r], L)
        local = np.array([src[y][1] for y in ys], dtype=np.int64)
        bits[:, ys] = wire_expand(a[:, local], c[:, local])
    return out

"""CPU restatement of sdfhip_scene_select (include/sdfhip.h), numpy, float32 throughout, every operation an
array operation of its own in the order the header writes it.  The labelling is components_restatement.components, the source value
place_restatement.value at the identity, the bytes and the corner table trimesh_restatement's from_float and CORNER, the construct
rule and the node order place_restatement.place's: the contracts cannot drift.  Every distinct point of a level is evaluated once.

tests/test_select.py holds this file to things it did not come from (pinned counts, the identity placement, the links' invariance);
tests/test_gpu_select.py holds the GPU to this file, byte for byte."""
import numpy as np

import components_restatement as cpr
import place_restatement as plr
from edit_restatement import tree_depth
from trimesh_restatement import CORNER, from_float

f32 = np.float32
KEEP_LARGEST, DROP_SMALL, FILL_ENCLOSED, FLIP_LISTED, KEEP_LISTED = 1, 2, 4, 8, 16
ALL_RULES = 31
H = f32(2.0 ** -8)


def decide(rec, flags, lattice_depth, min_points=0, listed=()):
    """one bool per record of components_restatement's table: does the component flip?  Raises ValueError for what the call refuses
    after its labelling pass: a listed label that is no component's, a void under KEEP_LISTED."""
    flags = int(flags)
    solid = rec["flags"] == cpr.SOLID
    listed = sorted(set(int(x) for x in listed))
    labels = [int(x) for x in rec["label"]]
    for x in listed:
        if x not in labels:
            raise ValueError(f"label {x} is not the label of a component")
    is_listed = np.isin(rec["label"], np.array(listed, dtype=np.int64))
    flip = np.zeros(len(rec), bool)
    if flags & KEEP_LARGEST and solid.any():
        # most points, then the lowest label: the records are in ascending label order, and argmax takes the first
        best = np.nonzero(solid)[0][np.argmax(rec["points"][solid])]
        flip |= solid & (np.arange(len(rec)) != best)
    if flags & DROP_SMALL:
        flip |= solid & (rec["points"] < int(min_points))
    if flags & FILL_ENCLOSED:
        last = (1 << int(lattice_depth)) - 1
        flip |= ~solid & (rec["lo"] != 0).all(1) & (rec["hi"] != last).all(1)
    if flags & FLIP_LISTED:
        flip |= is_listed
    if flags & KEEP_LISTED:
        if (is_listed & ~solid).any():
            raise ValueError(f"label {int(rec['label'][is_listed & ~solid][0])} is a void")
        flip |= solid & ~is_listed
    return flip


def targets(src, flags, lattice_depth=6, origin=(0.0, 0.0, 0.0), side=1.0, min_points=0, listed=(), labelled=None):
    """(F, T, counts): (n, n, n) bool arrays indexed [z, y, x] -- the point's component flips; its target phase -- and the lattice
    side of the stats.  labelled: (records, labels) of components_restatement.components on this lattice, if the caller has them."""
    rec, lab = cpr.components(src, lattice_depth, origin, side) if labelled is None else labelled
    flip = decide(rec, flags, lattice_depth, min_points, listed)
    slot = np.searchsorted(rec["label"], lab.reshape(-1))
    F = flip[slot].reshape(lab.shape)
    phase = (rec["flags"] == cpr.SOLID)[slot].reshape(lab.shape)
    solid = rec["flags"] == cpr.SOLID
    counts = {"components": len(rec), "solids": int(solid.sum()), "flipped_solids": int((flip & solid).sum()),
              "flipped_voids": int((flip & ~solid).sum()), "points_flipped": int(rec["points"][flip].sum())}
    return F, phase ^ F, counts


def neighbours(p, lattice_depth, origin, side):
    """per axis the two candidate indices (int64 arrays) of N(p) for points p (n, 3): g = (p_a - origin_a) / pitch - 0.5f,
    f = floorf(g), {f} if g == f else {f, f + 1}, clamped into 0 .. 2^d - 1 in float"""
    p = np.asarray(p, dtype=f32).reshape(-1, 3)
    o = np.asarray(origin, dtype=f32).reshape(3)
    pitch = f32(side) * f32(2.0 ** -int(lattice_depth))
    last = f32((1 << int(lattice_depth)) - 1)
    out = []
    with np.errstate(all="ignore"):
        for a in range(3):
            g = (p[:, a] - o[a]) / pitch - f32(0.5)
            f = np.floor(g)
            c0 = np.fmin(np.fmax(f, f32(0)), last)
            c1 = np.where(g == f, c0, np.fmin(np.fmax(f + f32(1), f32(0)), last))
            assert g.dtype == f32 and c0.dtype == f32 and c1.dtype == f32
            out.append((c0.astype(np.int64), c1.astype(np.int64)))
    return out


def changed(v, p, F, T, lattice_depth, origin, side):
    """v' of the rule for the source values v (n,) at points p (n, 3)"""
    (x0, x1), (y0, y1), (z0, z1) = neighbours(p, lattice_depth, origin, side)
    any_f = np.zeros(len(v), bool)
    all_t = np.ones(len(v), bool)
    none_t = np.ones(len(v), bool)
    for z in (z0, z1):
        for y in (y0, y1):
            for x in (x0, x1):
                any_f |= F[z, y, x]
                all_t &= T[z, y, x]
                none_t &= ~T[z, y, x]
    with np.errstate(all="ignore"):
        far = np.fmax(np.abs(v), H)
    out = np.where(any_f & all_t, -far, np.where(any_f & none_t, far, v))
    assert out.dtype == f32
    return out


def select(src, flags=0, listed=(), lattice_depth=6, origin=(0.0, 0.0, 0.0), side=1.0, depth=-1, min_points=0, want_counts=False, labelled=None,
           memo=None):
    """src: (structs, values) -> (structs, values) of the selected tree (new arrays), breadth first.  depth: -1 = the source's, else
    0..12.  want_counts: also the integer fields of sdfhip_select_stats.  memo: a dict the caller keeps per source -- the source
    values of a level's distinct points, which depend on neither the rule nor the lattice."""
    if int(flags) & ~ALL_RULES or (int(flags) & FLIP_LISTED and int(flags) & KEEP_LISTED):
        raise ValueError(f"flags {flags}")
    SS = np.ascontiguousarray(src[0], dtype=np.int32).reshape(-1, 2)
    SV = np.ascontiguousarray(src[1], dtype=np.uint8).reshape(-1, 8)
    F, T, counts = targets((SS, SV), flags, lattice_depth, origin, side, min_points, listed, labelled)
    max_depth = tree_depth(SS) if depth < 0 else int(depth)
    coords = np.zeros((1, 3), dtype=np.int64)
    parent = np.full(1, -1, dtype=np.int64)
    S_out, V_out = [], []
    start, d, samples = 0, 0, 0
    while True:
        S = f32(2.0 ** -d)
        n = len(coords)
        samples += 9 if d == 0 else 35 * (n // 8)
        pts = np.concatenate([(2 * (coords[:, None, :] + CORNER[None])).reshape(-1, 3), 2 * coords + 1])     # in units of S / 2
        uniq, inv = np.unique(pts, axis=0, return_inverse=True)
        p = uniq.astype(f32) * f32(S * f32(0.5))
        key = (d, uniq.shape, hash(uniq.tobytes()))
        if memo is not None and key in memo:
            v = memo[key]
        else:
            v = plr.value((SS, SV), p, plr.IDENTITY, 1.0, (0.0, 0.0, 0.0))
            if memo is not None:
                memo[key] = v
        w = changed(v, p, F, T, lattice_depth, origin, side)[inv.reshape(-1)]
        cv, mv = w[:8 * n].reshape(n, 8), w[8 * n:]
        V_out.append(from_float(cv, S))
        links = np.full((n, 2), -1, dtype=np.int32)
        links[:, 0] = parent
        with np.errstate(all="ignore"):
            split = np.nonzero(np.abs(mv) < f32(2) * S)[0] if d < max_depth else np.zeros(0, dtype=np.int64)
        end = start + n
        links[split, 1] = end + 8 * np.arange(len(split))
        S_out.append(links)
        if not len(split):
            break
        coords = (2 * coords[split][:, None, :] + CORNER[None]).reshape(-1, 3)
        parent = np.repeat(start + split, 8)
        start = end
        d += 1
    structs, values = np.concatenate(S_out), np.concatenate(V_out)
    if want_counts:
        counts.update({"nodes_in": len(SS), "nodes_out": len(structs), "depth_out": d, "levels": d + 1, "samples": samples})
        return structs, values, counts
    return structs, values

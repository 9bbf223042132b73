"""CPU restatement of sdfhip_scene_components (include/sdfhip.h), numpy: the lattice is
clash_restatement.lattice, inside is place_restatement.value at the identity < 0, and the labels come from min-index propagation
over the six shifts -- every point takes the lowest label among itself and its face neighbours of the same phase, then the label of
its label (a label is the index of a point of the same component, so this only shortens the way) -- until nothing changes.  No
union-find, no blocks.  The records are the C dtype, in label order.

tests/test_components.py holds this file to things it did not come from (counts pinned from labellers written another way: a
breadth-first flood fill and scipy's); tests/test_gpu_components.py holds the GPU to this file, byte for byte."""
import numpy as np

import clash_restatement as clr
import place_restatement as plr

f32 = np.float32
MAX_DEPTH = 9
SOLID = 1
COMPONENT = np.dtype([("label", "<u4"), ("flags", "<u4"), ("points", "<u4"), ("reserved", "<u4"), ("lo", "<u4", (3,)), ("hi", "<u4", (3,)),
                      ("sum", "<u8", (3,))])
assert COMPONENT.itemsize == 64


def inside(src, depth, origin=(0.0, 0.0, 0.0), side=1.0):
    """(n, n, n) bool indexed [z, y, x], n = 2^depth: value(p) < 0 at the lattice's points (a NaN is outside)"""
    n = 1 << int(depth)
    p = clr.lattice(depth, origin, side)[0]
    with np.errstate(invalid="ignore"):
        return (plr.value(src, p, plr.IDENTITY, 1.0, (0.0, 0.0, 0.0)) < f32(0)).reshape(n, n, n)


def label(ins):
    """(n, n, n) int64: every point's label, the lowest linear index of its face-connected component of equal phase"""
    n = ins.shape[0]
    lab = np.arange(n ** 3, dtype=np.int64).reshape(n, n, n)
    while True:
        new = lab.copy()
        for axis in range(3):
            a = [slice(None)] * 3
            b = [slice(None)] * 3
            a[axis], b[axis] = slice(0, n - 1), slice(1, n)
            a, b = tuple(a), tuple(b)
            same = ins[a] == ins[b]
            new[a] = np.where(same, np.minimum(new[a], lab[b]), new[a])
            new[b] = np.where(same, np.minimum(new[b], lab[a]), new[b])
        new = new.reshape(-1)[new]
        if (new == lab).all():
            return lab
        lab = new


def records(ins, lab):
    """the records of a labelling, in ascending label order"""
    n = ins.shape[0]
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    labels, idx = np.unique(lab.reshape(-1), return_inverse=True)
    idx = idx.reshape(-1)
    out = np.zeros(len(labels), COMPONENT)
    out["label"] = labels
    out["flags"] = np.where(ins.reshape(-1)[labels], SOLID, 0)
    out["points"] = np.bincount(idx)
    for k, c in enumerate((x, y, z)):
        c = c.reshape(-1)
        lo, hi = np.full(len(labels), n, np.int64), np.full(len(labels), -1, np.int64)
        np.minimum.at(lo, idx, c)
        np.maximum.at(hi, idx, c)
        out["lo"][:, k], out["hi"][:, k] = lo, hi
        out["sum"][:, k] = np.bincount(idx, weights=c).astype(np.uint64)         # (below 2^53: exact)
    return out


def components(src, depth=6, origin=(0.0, 0.0, 0.0), side=1.0):
    """src: (structs, values) -> (records in label order, labels (n, n, n) uint32 indexed [z, y, x])"""
    if not 0 <= int(depth) <= MAX_DEPTH:
        raise ValueError(f"depth {depth}")
    ins = inside(src, depth, origin, side)
    lab = label(ins)
    return records(ins, lab), lab.astype(np.uint32)

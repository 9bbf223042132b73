"""The scenes that tests/test_components.py (CPU) and tests/test_gpu_components.py (GPU) share, by name, and their restatements
(tests/components_restatement.py), each made once per process and left unchanged.  A case is a tree (structs, values) and the depths
it is run at, on the unit cube unless a box is given.  Not a test module."""
import numpy as np

import clash_cases as ca
import components_restatement as cpr
import compose_cases as cc
import compose_restatement as cr
import place_restatement as plr
import query_restatement as qr
import tree_zoo as tz

UNIT = ca.UNIT
OFF_CUBE = ca.OFF_CUBE                      # a box that leaves the unit cube on one side, on "eight"
OFF_CUBE_DEPTH = 5
SOLID_BYTE, EMPTY_BYTE = 0, 200


def _hollow():
    # the source's sphere with a half-size sphere taken out of its middle: a solid with a sealed cavity
    parts = [(cc.tree("sphere_d4"), (plr.IDENTITY, 1.0, (0.0, 0.0, 0.0)), cr.COMBINE_UNION),
             (cc.tree("sphere_d4"), (plr.IDENTITY, 0.5, (0.25, 0.25, 0.25)), cr.COMBINE_SUBTRACT)]
    return cr.compose(parts, 5)


def leaf_tree(solid):
    """A full depth-3 tree of 585 nodes, breadth first, whose 512 leaves are flat: byte 0 (solid) where solid(x, y, z) of the leaf's
    coordinates, else byte 200 (empty).  Each leaf is found by sampling its centre, not by assuming the child order."""
    first = [0, 1, 9, 73, 585]
    structs = np.full((585, 2), -1, np.int32)
    for level in range(3):
        for k in range(first[level], first[level + 1]):
            child = first[level + 1] + 8 * (k - first[level])
            structs[k, 1] = child
            structs[child:child + 8, 0] = k
    values = np.full((585, 8), EMPTY_BYTE, np.uint8)
    z, y, x = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    x, y, z = x.reshape(-1), y.reshape(-1), z.reshape(-1)
    centres = ((np.stack([x, y, z], 1) + 0.5) / 8.0).astype(np.float32)
    node = qr.sample(structs, values, centres)["node"].astype(np.int64)
    assert sorted(node) == list(range(73, 585))
    values[node[solid(x, y, z)]] = SOLID_BYTE
    return structs, values


def checker_solid(x, y, z):
    return (x + y + z) % 2 == 0


def snake_solid(x, y, z):
    # one body, 148 leaves long, that visits all 64 tiles of 8 x 8 x 8 of a depth-5 lattice: rows along x on the even y of the even
    # z, joined at alternating ends
    rows = (y % 2 == 0) & (z % 2 == 0)
    turns = (y % 2 == 1) & (z % 2 == 0) & (x == np.where((y // 2) % 2 == 0, 7, 0))
    lifts = (z % 2 == 1) & (y == np.where((z // 2) % 2 == 0, 6, 0)) & (x == np.where((y // 2) % 2 == 0, 0, 7))
    return rows | turns | lifts


ZOO = ("dfs_d6_a", "dfs_d6_b", "blocks_1025", "blocks_2049", "blocks_4097", "chain12", "leaf")

# name -> (tree, depths)
CASES = {
    "sphere_d4": (lambda: cc.tree("sphere_d4"), (0, 1, 2, 3, 5)),
    "torus_d6": (lambda: cc.tree("torus_d6"), (2, 5)),
    "eight": (lambda: cc.restated("eight")[:2], (3, 5)),
    "csg": (lambda: cc.restated("csg")[:2], (5,)),
    "hollow": (_hollow, (3, 5)),
    "checker": (lambda: leaf_tree(checker_solid), (3, 5)),
    "snake": (lambda: leaf_tree(snake_solid), (3, 5, 6)),
}
CASES.update({name: ((lambda name=name: tz.zoo()[name]), (5,)) for name in ZOO})
RUNS = [(name, d, UNIT) for name, (_, depths) in CASES.items() for d in depths] + [("eight", OFF_CUBE_DEPTH, OFF_CUBE)]

_trees, _restated = {}, {}


def tree(name):
    """(structs, values) of the named case, made once, read-only"""
    if name not in _trees:
        s, v = CASES[name][0]()
        s, v = np.ascontiguousarray(s, np.int32).reshape(-1, 2), np.ascontiguousarray(v, np.uint8).reshape(-1, 8)
        _trees[name] = (s, v)
    return _trees[name]


def restated(name, depth, box=UNIT):
    """(records, labels) of the restatement of the named case at `depth` on the cube `box` = (origin, side); made once, read-only"""
    key = (name, depth, box)
    if key not in _restated:
        rec, lab = cpr.components(tree(name), depth, *box)
        rec.setflags(write=False)
        lab.setflags(write=False)
        _restated[key] = (rec, lab)
    return _restated[key]


def points_by_phase(records):
    """(the solids' points, the voids' points), each a list in descending order"""
    solid = records["flags"] == cpr.SOLID
    return sorted((int(v) for v in records["points"][solid]), reverse=True), sorted((int(v) for v in records["points"][~solid]), reverse=True)

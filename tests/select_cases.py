"""The scenes that tests/test_select.py (CPU) and tests/test_gpu_select.py (GPU) share, by name, and their restatements
(tests/select_restatement.py), each made once per process and left unchanged.  The trees are components_cases' and two of this
module's own; a run is (case, rule) on a lattice and to a result depth.  Not a test module."""
import numpy as np

import components_cases as cs
import components_restatement as cpr
import compose_cases as cc
import compose_restatement as cr
import place_restatement as plr
import select_restatement as sr

UNIT = cs.UNIT
OFF_CUBE = cs.OFF_CUBE
STRADDLE_DEPTH = 7
DROP_BELOW = 20                 # crumbs: the two crumbs (17, 1); csg: its two specks (2, 2); hollow and eight: nothing


def _union(placed, depth):
    sphere = cc.tree("sphere_d4")
    return cr.compose([(sphere, (plr.IDENTITY, s, t), cr.COMBINE_UNION) for s, t in placed], depth)


def _crumbs():
    # a body and two crumbs, the smaller a single lattice point at depth 5
    return _union([(0.6, (0.05, 0.05, 0.05)), (0.2, (0.72, 0.72, 0.72)), (0.12, (0.8, 0.1, 0.1))], 5)


# straddle: a large sphere in the corner at the origin and a small one centred on the plane x = 0.5
STRADDLE_PARTS = [(0.5, (0.0, 0.0, 0.0)), (0.1, (0.45, 0.75, 0.75))]


def _straddle():
    return _union(STRADDLE_PARTS, 5)


_own = {"crumbs": _crumbs, "straddle": _straddle}
_trees, _labelled, _memo, _restated = {}, {}, {}, {}


def tree(name):
    """(structs, values) of the named case, made once, read-only"""
    if name not in _own:
        return cs.tree(name)
    if name not in _trees:
        s, v = _own[name]()
        s, v = np.ascontiguousarray(s, np.int32).reshape(-1, 2), np.ascontiguousarray(v, np.uint8).reshape(-1, 8)
        s.setflags(write=False)
        v.setflags(write=False)
        _trees[name] = (s, v)
    return _trees[name]


def labelled(name, lattice_depth, box=UNIT):
    """(records, labels) of components_restatement on the named case's lattice; made once, read-only"""
    if name in cs.CASES:
        return cs.restated(name, lattice_depth, box)
    key = (name, lattice_depth, box)
    if key not in _labelled:
        rec, lab = cpr.components(tree(name), lattice_depth, *box)
        rec.setflags(write=False)
        lab.setflags(write=False)
        _labelled[key] = (rec, lab)
    return _labelled[key]


def solids(rec):
    """the solids' records, largest first (ties: the lowest label first)"""
    s = rec[rec["flags"] == cpr.SOLID]
    return s[np.argsort(-s["points"].astype(np.int64), kind="stable")]


def enclosed_voids(rec, lattice_depth):
    last = (1 << lattice_depth) - 1
    return rec[(rec["flags"] != cpr.SOLID) & (rec["lo"] != 0).all(1) & (rec["hi"] != last).all(1)]


# rule name -> (flags, min_points, the list as a function of the lattice's records and depth)
RULES = {
    "none": (0, 0, None),
    "keep_largest": (sr.KEEP_LARGEST, 0, None),
    "drop_small": (sr.DROP_SMALL, DROP_BELOW, None),
    "fill_enclosed": (sr.FILL_ENCLOSED, 0, None),
    # the smallest solid, twice, and every enclosed void, behind it: any order, repeats
    "flip_listed": (sr.FLIP_LISTED, 0, lambda rec, d: [int(solids(rec)[-1]["label"])] * 2 + [int(x) for x in enclosed_voids(rec, d)["label"]][::-1]),
    "keep_listed": (sr.KEEP_LISTED, 0, lambda rec, d: [int(solids(rec)[0]["label"])]),
    "keep_largest_and_fill": (sr.KEEP_LARGEST | sr.FILL_ENCLOSED, 0, None),
    "flip_the_one_solid": (sr.FLIP_LISTED, 0, lambda rec, d: [int(solids(rec)[0]["label"])]),
}


def rule(name, rule_name, lattice_depth, box=UNIT):
    """(flags, min_points, listed labels) of the named rule on the named case's lattice"""
    flags, min_points, lister = RULES[rule_name]
    return flags, min_points, ([] if lister is None else lister(labelled(name, lattice_depth, box)[0], lattice_depth))


def restated(name, rule_name, lattice_depth, depth, box=UNIT):
    """(structs, values, counts) of the restatement; made once, read-only"""
    key = (name, rule_name, lattice_depth, depth, box)
    if key not in _restated:
        flags, min_points, listed = rule(name, rule_name, lattice_depth, box)
        S, V, counts = sr.select(tree(name), flags, listed, lattice_depth, box[0], box[1], depth, min_points, want_counts=True,
                                 labelled=labelled(name, lattice_depth, box), memo=_memo.setdefault(name, {}))
        S.setflags(write=False)
        V.setflags(write=False)
        _restated[key] = (S, V, counts)
    return _restated[key]


def result_depth(name):
    return 6 if name == "csg" else 5


# straddle's reason to exist, asserted where the case is made: on the lattice of depth 7 a row of 128 points is two 64-bit words of a
# bitmap, and the small sphere has points on both sides of the boundary between them
def straddle_small():
    """the record of straddle's small solid at STRADDLE_DEPTH"""
    rec = labelled("straddle", STRADDLE_DEPTH)[0]
    s = solids(rec)
    half = 1 << (STRADDLE_DEPTH - 1)
    assert len(s) == 2 and s[1]["lo"][0] <= half - 1 and s[1]["hi"][0] >= half, s
    return s[1]

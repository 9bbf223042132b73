"""The assemblies that tests/test_clash.py (CPU) and tests/test_gpu_clash.py (GPU) share, by name, and their restatements
(tests/clash_restatement.py), each made once per process and left unchanged.  A case is a list of parts as tests/compose_cases.py
writes them -- (source name, (R, s, t), op) -- and the depths it is run at, on the unit cube unless a box is given.  Not a test module."""
import numpy as np

import clash_restatement as clr
import compose_cases as cc
import compose_restatement as cr
import instances_cases as ic
import place_restatement as plr

U = cr.COMBINE_UNION
UNIT = ((0.0, 0.0, 0.0), 1.0)
OFF_CUBE = ((-0.3, 0.1, 0.2), 0.7)          # a box that leaves the unit cube on one side, on "csg"
OFF_CUBE_DEPTH = 5


def _lens():
    # two balls of radius 0.15 (the source's sphere at half size) whose centres are 0.2 apart
    return [("sphere_d4", (plr.IDENTITY, 0.5, (0.05, 0.25, 0.25)), U), ("sphere_d4", (plr.IDENTITY, 0.5, (0.25, 0.25, 0.25)), U)]


def _chain64():
    # 64 balls of radius 0.06 in a row, 0.011 apart: each overlaps its next few neighbours
    return [("sphere_d4", (plr.IDENTITY, 0.2, (0.05 + 0.011 * k, 0.4, 0.4)), U) for k in range(64)]


def _same64():
    # ONE placement 64 times: every lane of every block is in every one of the 2016 pairs
    return [("sphere_d4", (plr.IDENTITY, 0.5, (0.25, 0.25, 0.25)), U) for _ in range(64)]


# name -> (parts, depths)
CASES = {
    "lens": (_lens, (5, 6)),
    "csg": (lambda: cc.case("csg")[0], (0, 1, 2, 5)),
    "eight": (lambda: cc.case("eight")[0], (5,)),
    "two_spheres": (lambda: ic.parts("two_spheres"), (5,)),
    "far": (lambda: ic.parts("far"), (5,)),
    "deepest": (lambda: ic.parts("deepest"), (5,)),
    "three_forms": (lambda: ic.parts("three_forms"), (5,)),
    "chain64": (_chain64, (5,)),
    "same64": (_same64, (3,)),
    "one": (lambda: [_lens()[0]], (3,)),
}
RUNS = [(name, d) for name, (_, depths) in CASES.items() for d in depths]
REFUSED = "many"                            # compose_cases.case("many"): 65 instances


def parts(name):
    return cc.case(REFUSED)[0] if name == REFUSED else CASES[name][0]()


def instances(name):
    """the case as clash_restatement takes it"""
    return cr.as_instances(cc.with_trees(parts(name)))


_restated = {}


def restated(name, depth, box=UNIT):
    """the restatement's records of the named case at `depth` on the cube `box` = (origin, side); made once, read-only"""
    key = (name, depth, box)
    if key not in _restated:
        out = clr.clash(instances(name), depth, *box)
        out.setflags(write=False)
        _restated[key] = out
    return _restated[key]


def as_dict(records, field="points"):
    """{(a, b): field} of a record array"""
    return {(int(r["a"]), int(r["b"])): (int(r[field]) if np.ndim(r[field]) == 0 else tuple(int(v) for v in r[field])) for r in records}

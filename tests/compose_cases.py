"""The compositions that tests/test_compose.py (CPU) and tests/test_gpu_compose.py (GPU) share, by name, and their restatements
(tests/compose_restatement.py), each made once per process and left unchanged.  A case is (parts, depth); a part is (source name,
(R, s, t), op), the source one of test_gpu_combine.tree's.  Not a test module."""
import numpy as np

import compose_restatement as cr
import place_restatement as plr
from test_gpu_combine import tree

U, I, S = cr.COMBINE_UNION, cr.COMBINE_INTERSECT, cr.COMBINE_SUBTRACT


def _placement(*args, **kw):
    import sdfbox_amd
    return sdfbox_amd.placement(*args, **kw)


# the placements of one instance: test_gpu_place.PLACEMENTS' identity, generic_half and mirror
ONE_PLACEMENTS = {
    "identity": lambda: (plr.IDENTITY, 1.0, (0.0, 0.0, 0.0)),
    "generic_half": lambda: _placement(30, 20, 0, 0.5),
    "mirror": lambda: (np.diag([-1.0, 1.0, 1.0]).astype(np.float32), 0.75, (0.95, 0.1, 0.2)),
}
ONE = [f"one:{src}:{name}" for src in ("leaf", "nine", "sphere_d4") for name in ONE_PLACEMENTS]


def _eight():
    # ONE handle eight times, at scale 0.4 in the eight octants' centres, each turned differently
    parts = []
    for k in range(8):
        to = (0.27 + 0.46 * (k & 1), 0.27 + 0.46 * (k >> 1 & 1), 0.27 + 0.46 * (k >> 2))
        parts.append(("sphere_d4", _placement(45.0 * k, 20.0 * k - 70.0, 13.0 * k, 0.4, to=to), U))
    return parts, 5


def _csg():
    # a union, then a difference, then an intersection: the order of the list is the order of the fold
    return [("torus_d6", _placement(20, -30, 10, 0.9), U),
            ("sphere_d4", _placement(0, 0, 0, 0.5, to=(0.72, 0.5, 0.5)), S),
            ("sphere_d4", _placement(10, 20, 30, 1.2, to=(0.45, 0.5, 0.5)), I)], 6


def _many():
    # more instances than a wave has lanes: 65 of the nine-node tree at scale 0.12 on a 5 x 5 x 3 grid, every ninth carved out
    parts = []
    for k in range(65):
        i, j, m = k % 5, k // 5 % 5, k // 25
        to = (0.1 + 0.2 * i, 0.1 + 0.2 * j, 0.2 + 0.3 * m)
        parts.append(("nine", _placement(7.0 * k, 0, 0, 0.12, to=to), S if k % 9 == 4 else U))
    return parts, 4


def _far(depth=7):
    # the torus as test_gpu_place.BIG places it, with an instance that lies three cubes away
    return [("torus_d6", _placement(30, 20, 0, 0.62), U), ("sphere_d4", (plr.IDENTITY, 1.0, (3.0, 0.0, 0.0)), U)], depth


def _deepest():
    # depth -1 with sources of depths 4 and 6
    return [("sphere_d4", _placement(0, 0, 0, 0.6, to=(0.35, 0.4, 0.5)), U), ("torus_d6", _placement(0, 90, 0, 0.7, to=(0.6, 0.55, 0.5)), U)], -1


def case(name):
    """(parts, depth) of the named case"""
    if name.startswith("one:"):
        _, src, pl = name.split(":")
        return [(src, ONE_PLACEMENTS[pl](), U)], -1
    if name == "depth0":
        return _csg()[0], 0
    return {"eight": _eight, "csg": _csg, "many": _many, "far": _far, "deepest": _deepest}[name]()


MULTI = ["eight", "csg", "many", "far", "depth0", "deepest"]
_restated = {}


def with_trees(parts):
    """the parts with the sources' arrays in place of their names: what compose_restatement.compose takes"""
    return [(tree(src), pl, op) for src, pl, op in parts]


def restated(name):
    """(structs, values, counts) of the restatement of the named case, made once and left unchanged"""
    if name not in _restated:
        parts, depth = case(name)
        _restated[name] = cr.compose(with_trees(parts), depth, want_counts=True)
    return _restated[name]

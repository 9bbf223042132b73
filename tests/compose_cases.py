"""The compositions that tests/test_compose.py (CPU) and tests/test_gpu_compose.py (GPU) share, by name, and their restatements
(tests/compose_restatement.py), each made once per process and left unchanged.  A case is (parts, depth); a part is (source name,
(R, s, t), op), the source one of tree()'s.  Not a test module."""
import numpy as np

import compose_restatement as cr
import place_restatement as plr
import tree_zoo as tz
from test_gpu_combine import tree as _builders_tree

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


def _corner_d12(instances=2):
    # depth 12 in the corner away from the origin: two small spheres (scale 2^-7: the source's leaves land on the result's level 11)
    # whose blocks have coordinates near 2^11 -- the 16 bits of a packed y, the float of 2 * bx + li, the doubling of the emit.  The
    # first is turned, the second is not and sits on the face y = 1 where x and z are small.  Its last level is past one chunk of
    # the shared scan
    sc = 2.0 ** -7
    parts = [("sphere_d4", (_placement(0, 0, 30)[0], sc, (1 - 0.9 * sc, 1 - 1.2 * sc, 1 - 1.1 * sc)), U),
             ("sphere_d4", (plr.IDENTITY, sc, (0.0, 1 - sc, 0.0)), U)]
    return parts[:instances], 12


# ---- the instance limit -------------------------------------------------------------------------------------------------------------
LIMIT = 4096
LIMIT_DEPTH = 4


def limit_pairs():
    """the 16 distinct (source, placement) pairs the long lists repeat: small trees, each at four placements"""
    pairs = []
    for j in range(16):
        src = ("leaf", "nine", "blocks_65", "blocks_65")[j % 4]
        to = (0.3 + 0.4 * (j >> 2 & 1), 0.3 + 0.4 * (j >> 3), 0.35 + 0.1 * (j % 4))
        pairs.append((src, _placement(23.0 * j, 11.0 * j - 40.0, 7.0 * j, 0.45 + 0.05 * (j % 4), to=to)))
    return pairs


def limit_parts(n):
    """the first n entries of the 4096-long list: entry k is pair k % 16, and its op is drawn anew for every k (a fixed seed), so a
    repeat of a pair meets another op and another state of the fold than the time before: later repeats still change the tree"""
    pairs = limit_pairs()
    ops = np.random.default_rng(4096).choice([U, U, S, I], size=LIMIT)
    # an intersection with a small solid leaves next to nothing: only the two largest placements (scale 0.6) are ever intersected with
    ops = [int(op) if (op != I or k % 4 == 3) else S for k, op in enumerate(ops)]
    ops[0] = U
    return [(pairs[k % 16][0], pairs[k % 16][1], ops[k]) for k in range(n)]


def folded_value(instances, p):
    """compose_restatement.value by another route: plr.value once per DISTINCT (source, placement) of the list, then the fold over
    the whole list in list order with cr.fminf / cr.fmaxf.  The same floats in the same order of operations: the same bits."""
    seen, v = {}, None
    for src, (R, s, t), op in instances:
        key = (src[0].ctypes.data, src[1].ctypes.data, R.tobytes(), s.tobytes(), t.tobytes())
        if key not in seen:
            seen[key] = plr.value(src, p, R, s, t)
        u = seen[key]
        v = u if v is None else cr.fminf(v, u) if op == U else cr.fmaxf(v, u) if op == I else cr.fmaxf(v, -u)
    return v


def case(name):
    """(parts, depth) of the named case"""
    if name.startswith("one:"):
        _, src, pl = name.split(":")
        return [(src, ONE_PLACEMENTS[pl](), U)], -1
    if name == "depth0":
        return _csg()[0], 0
    if name == "corner_d12_one":
        return _corner_d12(1)
    if name.startswith("limit_"):
        return limit_parts(int(name[len("limit_"):])), LIMIT_DEPTH
    return {"eight": _eight, "csg": _csg, "many": _many, "far": _far, "deepest": _deepest, "corner_d12": _corner_d12}[name]()


# corner_d12: see _corner_d12.  limit_N: the first N of the 4096 instances of limit_parts -- one short of a wave, a wave, and the most
# a call takes
MULTI = ["eight", "csg", "many", "far", "depth0", "deepest", "corner_d12", "corner_d12_one", "limit_63", "limit_64", f"limit_{LIMIT}"]
# the sizes the restatement gives (tests/test_compose.py pins them): corner_d12's last level has 48 120 nodes, past one chunk of the
# shared scan; it restates in 1.4 s, the long lists by the fold in 0.6 s
CORNER_D12_NODES, CORNER_D12_ONE_NODES = 63233, 33577
LIMIT_NODES = {63: 2617, 64: 1713, 130: 3753, LIMIT: 4113}
_restated = {}


def tree(name):
    """(structs, values) of a source: tests/tree_zoo.py's blocks_65, else test_gpu_combine.tree's"""
    return tz.zoo()[name] if name.startswith("blocks_") else _builders_tree(name)


def with_trees(parts):
    """the parts with the sources' arrays in place of their names: what compose_restatement.compose takes"""
    return [(tree(src), pl, op) for src, pl, op in parts]


def restated(name):
    """(structs, values, counts) of the restatement of the named case, made once and left unchanged.  The long lists go by the
    fold over their distinct pairs (folded_value): instance by instance, 4096 instances take a minute."""
    if name not in _restated:
        parts, depth = case(name)
        route = folded_value if name.startswith("limit_") else cr.value
        _restated[name] = cr.compose(with_trees(parts), depth, want_counts=True, value_of=route)
    return _restated[name]

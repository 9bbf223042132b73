"""The assemblies that tests/test_gap.py (CPU) and tests/test_gpu_gap.py (GPU) share, by name, and their restatements
(tests/gap_restatement.py), each made once per process and left unchanged: the brute force takes from a fraction of a second to a few
seconds a case.  A case is a list of parts as tests/compose_cases.py writes them -- (source name, (R, s, t), op).  Not a test module."""
import numpy as np

import clash_cases as ca
import compose_cases as cc
import compose_restatement as cr
import gap_restatement as gr
import place_restatement as plr
import tree_zoo as tz

U = cr.COMBINE_UNION
ZOO_TREE = "chain12"                 # the deepest meshable tree of the zoo: the search's stack at depth 12


def _at(src, s, t):
    return (src, (plr.IDENTITY, s, t), U)


CASES = {
    # two balls of radius 0.15 whose centres are 0.4 apart: the two directions differ in the last bit
    "apart": lambda: [_at("sphere_d4", 0.5, (0.05, 0.25, 0.25)), _at("sphere_d4", 0.5, (0.45, 0.25, 0.25))],
    # one placement twice: gap 0.0 exactly, a tie at every vertex
    "same2": lambda: [_at("sphere_d4", 1.0, (0.0, 0.0, 0.0))] * 2,
    # a quarter-size ball inside the ball: flag bit 1
    "nested": lambda: [_at("sphere_d4", 1.0, (0.0, 0.0, 0.0)), _at("sphere_d4", 0.25, (0.375, 0.375, 0.375))],
    # a turned ball, a mirrored nine-node tree, and a part without a surface
    "generic": lambda: [("sphere_d4", cc.ONE_PLACEMENTS["generic_half"](), U), ("nine", cc.ONE_PLACEMENTS["mirror"](), U), _at("leaf", 0.2, (1.5, 0.1, 0.1))],
    # 64 small parts in a row: 2016 records
    "row64": lambda: [_at("nine", 0.1, (0.02 + 0.015 * k, 0.4, 0.4)) for k in range(64)],
    "lens": lambda: ca.parts("lens"),
    "far": lambda: cc.case("far")[0],
    # a cut-cell list past one chunk of the shared scan and past many workgroups; the brute force stays cheap: 12 triangles on one side
    "big_list": lambda: [_at("torus_d6", 1.0, (0.0, 0.0, 0.0)), _at("nine", 0.3, (1.2, 0.3, 0.3))],
    "zoo": lambda: [_at(ZOO_TREE, 1.0, (0.0, 0.0, 0.0)), _at("nine", 0.5, (1.25, 0.2, 0.2))],
}
NAMES = list(CASES)
ROW64_LIMIT = 0.02                   # between two of row64's gaps (test_gap.py pins that it is)

_instances, _restated = {}, {}


def tree(name):
    """(structs, values) of a source: compose_cases.tree's (whose "leaf" is all outside: no surface), and tests/tree_zoo.py's deep trees"""
    return tz.zoo()[name] if name.startswith(("chain", "dfs_")) else cc.tree(name)


def parts(name):
    return CASES[name]()


def instances(name):
    """the case as the restatement takes it; one list per name, so that the arrays stay alive under the restatement's caches"""
    if name not in _instances:
        _instances[name] = cr.as_instances([(tree(src), pl, op) for src, pl, op in parts(name)])
    return _instances[name]


def restated(name, limit=np.inf):
    """(records, counts) of the named case at `limit`; made once, read-only.  A finite limit filters the +inf records: a pair has a
    record iff its gap is <= limit, and the record does not depend on the limit"""
    key = (name, float(limit))
    if key not in _restated:
        if np.isinf(limit):
            rec, counts = gr.gap(instances(name), want_counts=True)
        else:
            full, counts = restated(name)
            rec = full[full["gap"] <= np.float32(limit)].copy()
        rec.setflags(write=False)
        _restated[key] = (rec, counts)
    return _restated[key]

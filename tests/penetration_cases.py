"""The restatements (tests/penetration_restatement.py) of the assemblies of tests/clash_cases.py that tests/test_penetration.py (CPU)
and tests/test_gpu_penetration.py (GPU) share, each made once per process and left unchanged: the brute force takes from a fraction
of a second to a few seconds a case.  Not a test module."""
import clash_cases as ca
import compose_cases as cc
import compose_restatement as cr
import penetration_restatement as pr

UNIT, OFF_CUBE, OFF_CUBE_DEPTH = ca.UNIT, ca.OFF_CUBE, ca.OFF_CUBE_DEPTH

# (name, depth) held byte for byte on the GPU, on the unit cube
RUNS = [("lens", 5), ("lens", 6), ("csg", 5), ("chain64", 5), ("same64", 3), ("three_forms", 5), ("deepest", 5), ("one", 3), ("eight", 5)]

_instances, _restated = {}, {}


def own_sphere_three_times():
    """the source's own sphere (radius 0.3 round the cube's centre) three times over, as test_gpu_clash.py has it"""
    return [("sphere_d4", cc.ONE_PLACEMENTS["identity"](), cr.COMBINE_UNION)] * 3


def parts(name):
    return own_sphere_three_times() if name == "own3" else ca.parts(name)


def instances(name):
    """the case as the restatement takes it; one list per name, so that the arrays stay alive under the restatement's caches"""
    if name not in _instances:
        _instances[name] = cr.as_instances(cc.with_trees(parts(name)))
    return _instances[name]


def restated(name, depth, box=UNIT):
    """(records, counts) of the named case at `depth` on the cube `box` = (origin, side); made once, read-only"""
    key = (name, depth, box)
    if key not in _restated:
        rec, counts = pr.penetration(instances(name), depth, *box, want_counts=True)
        rec.setflags(write=False)
        _restated[key] = (rec, counts)
    return _restated[key]

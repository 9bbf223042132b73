"""The assemblies of hostile sources that tests/test_instances_zoo.py (CPU) and tests/test_gpu_instances_zoo.py (GPU) share, by name,
and their restatements (tests/instances_restatement.py), each made once per process and left unchanged.  What tests/instances_cases.py
is to the four friendly sources, this is to the trees of tests/tree_zoo.py -- append order, depth-first order, the 12- and the 14-deep
chain, bytes that are no distance field -- and to the edges of the calls themselves: the floor the exact skip leans on, ties, a tie of
signed zeros, the instance limit, the launch edges and points that are far but finite.  A case is a list of parts (source name,
(R, s, t), op), a camera, a frame, max_steps, the kinds of answer it is asked for ("sample", "raycast", "pick", "frame") and its points;
rays and pixels derive from the camera as in instances_cases.  Not a test module.

The cases, and the measured CPU time of their restated answers (all kinds together, the build machine's CPU; 45 s for them all, the
bases of the tie lists included):
  one:<tree>        one zoo tree under the identity: chain12 1.9 s, the others under 1 s
  corner:<chain>    sample alone, on tree_zoo.DEEP_CORNER's 9^3 points 2^-12 apart inside the chains' deepest cells: under 0.1 s
  keeps[:rotated]   tree_zoo's list of three unions -- all three win, all three statuses: 2.4 s, 2.3 s
  floor             leaf0 reads D = -0.5 exactly; its instances are skipped, looked up and lost, looked up and won: 2.9 s
  tie:*             a list whose last entry repeats the one before (BASES: the list without it): 1.6 .. 2.3 s each
  signtie           [X union, X subtract] with the points where X reads +0 in the batch -- fmaxf(+0, -0): 1.0 s
  limit_N           compose_cases.limit_parts(N) through sample and pick (20 steps), folded (ir.Folded): 0.4 s; 2 s at 4096
  edge, edge:WxH    513 points and rays, and frames of 1, 1, 2 and 5 tiles: 0.7 s; 1.0 s at most each
  far               16 finite points with a coordinate of 1e19 .. 3e38: under 0.1 s"""
import numpy as np

import compose_cases as cc
import compose_restatement as cr
import instances_cases as ic
import instances_restatement as ir
import place_restatement as plr
import query_restatement as qr
import tree_zoo as tz
import volume_restatement as vr

f32 = np.float32
U, I, S = cr.COMBINE_UNION, cr.COMBINE_INTERSECT, cr.COMBINE_SUBTRACT
KINDS = ("sample", "raycast", "pick", "frame")
ONE_NODE = {"leaf0": 0, "leaf255": 255}                       # one node, every byte the same: D = -0.5 and D = 1.5 exactly
ONE_TREES = ["chain12", "chain14", "dfs_d6_b", "blocks_257", "blocks_1017", "blocks_2049", "blocks_4097"]
LIMITS = (63, 64, cc.LIMIT)
EDGE_COUNTS = (1, 255, 256, 257, 513)                         # round the 256 threads of a workgroup, and a third workgroup's first
EDGE_FRAMES = {(1, 1): 1, (8, 8): 1, (9, 8): 2, (33, 1): 5}   # (width, height) -> tiles of 8 x 8; a workgroup takes four
ZERO_DRAW = 20000                                             # the seeded draw on the 1/256 lattice that "signtie" looks for zeros in


def tree(name):
    """(structs, values) of a source: leaf0 and leaf255; `leaf` and `nine` are the compositions' (compose_cases.tree: the long lists
    name them); else the zoo's"""
    if name in ONE_NODE:
        return tz.restated(("instances zoo tree", name), lambda: _frozen(np.array([[-1, -1]], np.int32), np.full((1, 8), ONE_NODE[name], np.uint8)))
    return cc.tree(name) if name in ("leaf", "nine") else tz.zoo()[name]


def _frozen(s, v):
    s.setflags(write=False); v.setflags(write=False)
    return s, v


IDENT = (plr.IDENTITY, 1.0, (0.0, 0.0, 0.0))


def _half():
    return cc.ONE_PLACEMENTS["generic_half"]()


def _floor():
    return [("dfs_d6_a", IDENT, U), ("leaf0", cc._placement(30, 20, 0, 0.25, to=(0.3, 0.5, 0.5)), U),
            ("leaf0", (plr.IDENTITY, 0.125, (0.6, 0.6, 0.2)), S), ("leaf255", (plr.IDENTITY, 2.0, (-0.5, -0.5, -0.5)), S)]


def _tie(op):
    return lambda: [("dfs_d6_b", IDENT, U), ("blocks_257", _half(), op), ("blocks_257", _half(), op)]


def _batch(n=333, seed=17):
    """instances_cases.points: in and round the cube, a NaN and an infinity in the middle"""
    p = np.random.default_rng(seed).uniform(-0.25, 1.25, size=(n, 3)).astype(f32)
    p[n // 2, 1] = np.nan
    p[n // 2 + 3, 2] = np.inf
    return p


def _floor_points():
    # the batch, and in its place twelve points inside each placed cube of leaf0, where e = 0 and u_k = -0.5 s_k exactly
    p = _batch()
    rng = np.random.default_rng(3)
    for k, at in ((1, 20), (2, 40)):
        _, (R, s, t), _ = _floor()[k]
        q = rng.uniform(0.2, 0.8, size=(12, 3))               # well inside the source's cube
        p[at:at + 12] = (float(s) * q @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)).astype(f32)
    return p


def zero_points():
    """the points of a seeded draw of ZERO_DRAW on the 1/256 lattice at which dfs_d6_b reads exactly 0"""
    def make():
        p = (np.random.default_rng(29).integers(0, 257, size=(ZERO_DRAW, 3)) / 256.0).astype(f32)
        return p[qr.sample(*tree("dfs_d6_b"), p)["distance"] == 0]
    return tz.restated(("instances zoo", "zero points"), make)


def _signtie_points():
    z = zero_points()
    p = _batch()
    p[10:10 + len(z)] = z                                     # in the batch's place: 333 points still
    return p


def _edge_points():
    p = np.random.default_rng(23).uniform(-0.25, 1.25, size=(EDGE_COUNTS[-1], 3)).astype(f32)
    p[255, 0] = np.nan                                        # the last lane of the first workgroup, the first of the second
    p[256, 2] = -np.inf
    return p


FAR = [1e19, -1e19, 2e19, -2e19, 3e38, -3e38]


def _far_points():
    # a far coordinate on each axis in turn, the others inside the cube; the last four have two and three far coordinates.  1e19
    # squares to 1e38 (finite), 2e19 to 4e38 (infinite); at 3e38 a product with a zero of a rotation is 0, with the rest infinite
    p = np.full((16, 3), 0.5, f32)
    for k, x in enumerate(FAR + FAR):
        p[k, (k + k // 6) % 3] = x
    p[12] = (1e19, -2e19, 0.25)
    p[13] = (3e38, 3e38, 3e38)
    p[14] = (-3e38, 3e38, -1e19)
    p[15] = (2e19, 2e19, -2e19)
    return p


def _case(parts, camera="default", size=ic.FRAME_LONG, steps=100, kinds=KINDS, points=_batch):
    return dict(parts=parts, camera=camera, size=size, steps=steps, kinds=kinds, points=points)


CASES = {f"one:{src}": _case(lambda src=src: [(src, IDENT, U)]) for src in ONE_TREES}
CASES.update({
    # every cell of blocks_2049 is flat at 63 or 64: from outside every pixel is black after one step; from inside the march goes on
    "one:blocks_2049:inside": _case(lambda: [("blocks_2049", IDENT, U)], camera="inside"),
    "corner:chain12": _case(lambda: [("chain12", IDENT, U)], kinds=("sample",), points=lambda: vr.lattice_points(*tz.DEEP_CORNER)),
    "corner:chain14": _case(lambda: [("chain14", IDENT, U)], kinds=("sample",), points=lambda: vr.lattice_points(*tz.DEEP_CORNER)),
    "keeps": _case(lambda: tz.compose_parts("keeps")),
    "keeps:rotated": _case(lambda: tz.compose_parts("keeps"), camera="rotated"),
    "floor": _case(_floor, points=_floor_points),
    "tie:xx": _case(lambda: [("dfs_d6_b", IDENT, U), ("dfs_d6_b", IDENT, U)]),
    "tie:union": _case(_tie(U)), "tie:intersect": _case(_tie(I)), "tie:subtract": _case(_tie(S)),
    "signtie": _case(lambda: [("dfs_d6_b", IDENT, U), ("dfs_d6_b", IDENT, S)], points=_signtie_points),
    "edge": _case(lambda: tz.compose_parts("keeps"), kinds=("sample", "raycast"), points=_edge_points),
    "far": _case(lambda: tz.compose_parts("keeps"), kinds=("sample",), points=_far_points),
})
# (a step of a march costs one fold of the whole list whatever the pixels: 0.07 s at 4096, so 20 steps as instances_cases' "many" has
# them; 100 took 5.2 s.  Rays still hit, escape and run out)
CASES.update({f"limit_{n}": _case(lambda n=n: cc.limit_parts(n), steps=20, kinds=("sample", "pick"), points=lambda: _batch(77)) for n in LIMITS + (130,)})
CASES.update({f"edge:{w}x{h}": _case(lambda: tz.compose_parts("keeps"), size=(w, h), kinds=("frame",)) for w, h in EDGE_FRAMES})
# a tie list without its last entry: what the CPU test compares the tie list with
BASES = {"tie:xx": "one:dfs_d6_b", "tie:union": "base:union", "tie:intersect": "base:intersect", "tie:subtract": "base:subtract"}
CASES.update({BASES[f"tie:{word}"]: _case(lambda op=op: _tie(op)()[:2]) for word, op in (("union", U), ("intersect", I), ("subtract", S))})

FULL = [name for name, c in CASES.items() if c["kinds"] == KINDS and not name.startswith("base:")]       # through all four calls
TIES = list(BASES)


def parts(name):
    return CASES[name]["parts"]()


def kinds(name):
    return CASES[name]["kinds"]


def instances(name):
    """the case as instances_restatement takes it; a long list as ir.Folded"""
    inst = cr.as_instances([(tree(src), pl, op) for src, pl, op in parts(name)])
    return ir.Folded(inst) if name.startswith("limit_") else inst


def camera(name):
    return ic.camera_named(CASES[name]["camera"], CASES[name]["size"])


def size(name):
    return CASES[name]["size"]


def max_steps(name):
    return CASES[name]["steps"]


def points(name):
    return tz.restated(("instances zoo points", name), CASES[name]["points"])


def pixels(name):
    """instances_cases' pixels of the case's frame"""
    return ic.pixels_of(size(name))


def rays(name):
    """(origins, dirs), as instances_cases.rays: the camera's rays of pixels(name) with a ray that escapes at step 0, a non-finite
    origin, a non-finite direction and a direction of all zeros in the middle.  "edge": EDGE_COUNTS[-1] rays, those of every pixel of
    a 27 x 19 frame of the default camera, the four odd ones round the workgroup's edge (253 .. 256)"""
    if name == "edge":
        W, H = 27, 19
        assert W * H == EDGE_COUNTS[-1]
        ys, xs = np.mgrid[0:H, 0:W]
        o, d = ir.camera_rays(ic.camera_named("default", (W, H)).State, np.stack([xs.ravel(), ys.ravel()], 1))
        m = 253
    else:
        o, d = ir.camera_rays(camera(name).State, pixels(name))
        m = len(o) // 2
    o, d = o.copy(), d.copy()
    o[m] = (9.0, 9.0, 9.0)
    o[m + 1, 0] = np.nan
    d[m + 2, 2] = np.inf
    d[m + 3] = 0.0
    return o, d


_restated, _visited = {}, {}


def restated(name, what):
    """the restatement's answer for the named case: what = one of kinds(name); made once, read-only"""
    assert what in kinds(name), (name, what)
    key = (name, what)
    if key not in _restated:
        inst, cam, (W, H), steps = instances(name), camera(name).State, size(name), max_steps(name)
        trace = []
        if what == "sample":
            out = ir.sample(inst, points(name))
            trace.append(points(name)[np.isfinite(points(name)).all(1)])
        elif what == "raycast":
            out = ir.raycast(inst, *rays(name), cam.margin, cam.limit, steps, trace=trace)
        elif what == "pick":
            out = ir.pick(inst, cam, pixels(name), steps, trace=trace)
        else:
            out = ir.frame(inst, cam, W, H, steps, trace=trace)
        out.setflags(write=False)
        _restated[key] = out
        _visited[key] = np.concatenate(trace) if trace else np.zeros((0, 3), f32)
    return _restated[key]


def visited(name):
    """(n, 3): every point at which the case's restatements evaluated F, the shadow rays and G's taps included"""
    return np.concatenate([(restated(name, what), _visited[(name, what)])[1] for what in kinds(name)])

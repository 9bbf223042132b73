"""The assemblies that tests/test_instances.py (CPU) and tests/test_gpu_instances.py (GPU) share, by name, and their restatements
(tests/instances_restatement.py), each made once per process and left unchanged.  A case is a list of parts as
tests/compose_cases.py writes them -- (source name, (R, s, t), op), the sources compose_cases.tree's leaf, nine, sphere_d4 and torus_d6
-- a camera, a small frame whose sides are no multiples of 8, max_steps, and the points, rays and pixels derived from them.  Not a
test module."""
import numpy as np

import compose_cases as cc
import compose_restatement as cr
import instances_restatement as ir
import place_restatement as plr
from conftest import make_camera

f32 = np.float32
U, I, S = cr.COMBINE_UNION, cr.COMBINE_INTERSECT, cr.COMBINE_SUBTRACT

FRAME, FRAME_LONG = (67, 41), (23, 17)        # (width, height): 9 x 6 and 3 x 3 tiles of 8 x 8, the last of each row and column partial


def _one(src, placement):
    return lambda: [(src, cc.ONE_PLACEMENTS[placement](), U)]


def _two_spheres():
    # two analytic spheres, disjoint: the source's sphere (centre 0.5, radius 0.3) at half size in two places
    return [("sphere_d4", (plr.IDENTITY, 0.5, (0.05, 0.25, 0.25)), U), ("sphere_d4", (plr.IDENTITY, 0.5, (0.45, 0.25, 0.25)), U)]


# name -> (parts, camera of conftest.CAMERAS, (width, height), max_steps)
CASES = {
    "one:sphere_d4:identity": (_one("sphere_d4", "identity"), "default", FRAME, 100),
    "one:sphere_d4:generic_half": (_one("sphere_d4", "generic_half"), "rotated", FRAME, 100),
    "one:sphere_d4:mirror": (_one("sphere_d4", "mirror"), "default", FRAME, 100),
    "one:leaf:generic_half": (_one("leaf", "generic_half"), "default", FRAME_LONG, 100),
    "one:nine:mirror": (_one("nine", "mirror"), "rotated", FRAME_LONG, 100),
    "eight": (lambda: cc.case("eight")[0], "rotated", FRAME, 100),
    "csg": (lambda: cc.case("csg")[0], "default", FRAME, 100),
    # (65 instances: every evaluation is 65 look-ups of the restatement; 20 steps leave rays that hit, escape and run out)
    "many": (lambda: cc.case("many")[0], "default", FRAME_LONG, 20),
    "far": (lambda: cc.case("far")[0], "rotated", FRAME, 100),
    "two_spheres": (_two_spheres, "default", FRAME, 100),
    # the camera inside the solid: the first value read is negative and the march goes backwards
    "inside": (_one("sphere_d4", "identity"), "inside", FRAME_LONG, 100),
    "steps1": (lambda: cc.case("csg")[0], "default", FRAME_LONG, 1),
    # for the test of the sources' cursor forms: two sources (depths 4 and 6), and ONE source three times
    "deepest": (lambda: cc.case("deepest")[0], "default", FRAME_LONG, 100),
    "three_forms": (lambda: [("sphere_d4", cc.case("deepest")[0][0][1], U), ("sphere_d4", cc.ONE_PLACEMENTS["generic_half"](), S),
                             ("sphere_d4", cc.ONE_PLACEMENTS["mirror"](), U)], "default", FRAME_LONG, 100),
}
NAMES = [name for name in CASES if name not in ("deepest", "three_forms")]


def parts(name):
    return CASES[name][0]()


def instances(name):
    """the case as instances_restatement takes it"""
    return cr.as_instances(cc.with_trees(parts(name)))


def camera(name):
    """the case's camera, a Logic"""
    return camera_named(CASES[name][1], CASES[name][2])


def camera_named(cam_name, size):
    """a camera of conftest.CAMERAS, or "inside", for a frame of `size` = (width, height)"""
    W, H = size
    if cam_name == "inside":
        cam = make_camera("default", W, H)
        cam.Position = (0.5, 0.5, 0.45)            # inside the sphere of radius 0.3 round the cube's centre
        return cam
    return make_camera(cam_name, W, H)


def size(name):
    return CASES[name][2]


def max_steps(name):
    return CASES[name][3]


def points(name):
    """(n, 3) float32: points in and round the cube, with a NaN and an infinity in the middle of the batch.  77: one workgroup's
    worth is 256; the long list gets fewer"""
    n = 77 if len(parts(name)) > 8 else 333
    p = np.random.default_rng(17).uniform(-0.25, 1.25, size=(n, 3)).astype(f32)
    p[n // 2, 1] = np.nan
    p[n // 2 + 3, 2] = np.inf
    return p


def pixels(name):
    """(n, 2) {x, y}: every fifth pixel of every fourth row, and the frame's corners"""
    return pixels_of(size(name))


def pixels_of(size):
    W, H = size
    xs, ys = np.meshgrid(np.arange(0, W, 5), np.arange(0, H, 4))
    px = np.stack([xs.ravel(), ys.ravel()], 1)
    return np.concatenate([px, [[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]]]).astype(np.uint32)


def rays(name):
    """(origins, dirs): the camera's rays of pixels(name), and in the middle of the batch a ray that escapes at step 0 (its origin is
    past the limit), a non-finite origin, a non-finite direction and a direction of all zeros"""
    o, d = ir.camera_rays(camera(name).State, pixels(name))
    o, d = o.copy(), d.copy()
    m = len(o) // 2
    o[m] = (9.0, 9.0, 9.0)                       # dot(pos, pos) = 243 > any camera's limit: ESCAPED with no step
    o[m + 1, 0] = np.nan
    d[m + 2, 2] = np.inf
    d[m + 3] = 0.0
    return o, d


_restated, _visited = {}, {}


def restated(name, what):
    """the restatement's answer for the named case: what = "sample", "raycast", "pick" or "frame"; made once, read-only"""
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
    """(n, 3): every point at which the case's restatements evaluated F -- the sample points and the raycast's, the pick's and the
    frame's marches, the shadow rays and G's taps included"""
    return np.concatenate([(restated(name, what), _visited[(name, what)])[1] for what in ("sample", "raycast", "pick", "frame")])

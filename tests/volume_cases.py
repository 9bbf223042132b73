"""The grids of tests/test_volume.py and tests/test_gpu_volume.py, and their restated trees, made once and left unchanged.  Every
field is an analytic distance evaluated in float64 at the lattice's vertices and rounded once to the grid's type.  Not a test
module."""
import numpy as np

import volume_restatement as vr

SPHERE = (0.5, 0.5, 0.5, 0.3)                  # sphere_d4's shape
TORUS = (0.5, 0.5, 0.5, 0.25, 0.09)            # torus_d6's shape (axis y)
TAU = 1.0 / 16                                 # the truncation of tsdf_d6


def lattice64(shape, origin, spacing):
    """the positions (nz, ny, nx, 3) of a lattice's vertices in float64"""
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    return np.stack([origin[0] + x * spacing, origin[1] + y * spacing, origin[2] + z * spacing], -1)


def sphere(p, shape=SPHERE):
    return np.sqrt(((p - np.array(shape[:3])) ** 2).sum(-1)) - shape[3]


def torus(p, shape=TORUS):
    x, y, z = p[..., 0] - shape[0], p[..., 1] - shape[1], p[..., 2] - shape[2]
    q = np.sqrt(x * x + z * z) - shape[3]
    return np.sqrt(q * q + y * y) - shape[4]


def _case(field, shape, origin, spacing, depth, dtype=np.float32, stored=1.0, clip=None):
    """stored: the grid holds distance * stored, and value_scale is 1 / stored"""
    d = field(lattice64(shape, origin, spacing))
    if clip is not None:
        d = np.clip(d, -clip, clip)
    grid = np.ascontiguousarray((d * stored).astype(dtype))
    grid.setflags(write=False)
    return dict(grid=grid, origin=tuple(origin), spacing=spacing, depth=depth, value_scale=1.0 / stored)


# Lattices the out direction is read on, (shape (nz, ny, nx), origin, spacing): a 5 x 1 x 7 lattice that sticks out of the cube on
# every side, and one element (tests/test_gpu_volume.py; tests/tree_zoo.py's out_lattices)
STICKS_OUT = ((7, 1, 5), (-0.3, 0.4, -0.45), 0.31)
ONE = ((1, 1, 1), (0.3, 0.6, 0.45), 1.0)

SP12 = 2.0 ** -11                              # corner_d12's spacing: a depth-12 tree's centres lie on it
CORNER_D12 = (1 - 11.3 * SP12, 1 - 12.1 * SP12, 1 - 11.7 * SP12, 4.4 * SP12)
HALF_EDGES = [65504.0, -65504.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -14, -2.0 ** -14, -0.0, 3 * 2.0 ** -16]


def corner_sphere(p):
    return sphere(p, CORNER_D12)


def _half_edges(stored):
    """a 9^3 float16 sphere grid with the edges of the format planted: the largest halves, the smallest subnormals, the smallest
    normals, -0.0 and a subnormal with two bits -- three of each, the small ones at the samples nearest the surface (where they
    decide bytes and splits), the large ones at the two ends of that order"""
    c = _case(sphere, (9, 9, 9), (0, 0, 0), 1.0 / 8, 3, dtype=np.float16, stored=stored)
    grid = c["grid"].copy()
    order = np.argsort(np.abs(grid.reshape(-1).astype(np.float64)), kind="stable")
    small, large = HALF_EDGES[2:], HALF_EDGES[:2]
    for k in range(3 * len(small)):
        grid.reshape(-1)[order[k]] = small[k % len(small)]
    for k in range(3):
        grid.reshape(-1)[order[20 + k]] = large[k % 2]
        grid.reshape(-1)[order[-1 - k]] = large[(k + 1) % 2]
    grid.setflags(write=False)
    return dict(c, grid=grid)


# name -> the case and the nodes of its tree.  two_d3: the smallest grid there is.  sphere17_d4: the analytic builder's own sphere.
# aniso_inset_d5: unequal n_a (nx = 9, ny = 13, nz = 21: a swapped stride reads another field), an origin inside the cube and a spacing
# that is no dyadic, so part of the cube lies in the continuation; its level 4 has 262 blocks, so the level ends inside a workgroup of
# four.  voxel_units_d5: a field in voxel units.  torus33_f16_d6: float16 samples.  tsdf_d6: the torus clipped at +-TAU, whose levels 4
# and 5 are full, and whose arrays have to grow (they start at 39 204 nodes).  outside: a grid at x = 3, the root alone.  sphere17_d7: level 6 has 38 016 nodes, past one
# chunk (32 768) of the shared scan.  The cases from corner_d12 on are the second round's (what each is for stands beside it, and
# test_volume.py's test_the_cases_are_what_they_are_for asserts it); each restates in under 0.4 s on the build machine's CPU.
_MAKERS = {
    "two_d3": (lambda: _case(sphere, (2, 2, 2), (0, 0, 0), 1.0, 3), 73),
    "sphere17_d4": (lambda: _case(sphere, (17, 17, 17), (0, 0, 0), 1.0 / 16, 4), 3465),
    "aniso_inset_d5": (lambda: _case(sphere, (21, 13, 9), (0.2, 0.15, 0.1), 0.04, 5), 10169),
    "voxel_units_d5": (lambda: _case(sphere, (33, 33, 33), (0, 0, 0), 1.0 / 32, 5, stored=32.0), 13385),
    "torus33_f16_d6": (lambda: _case(torus, (33, 33, 33), (0, 0, 0), 1.0 / 32, 6, dtype=np.float16), 39241),
    "tsdf_d6": (lambda: _case(torus, (33, 33, 33), (0, 0, 0), 1.0 / 32, 6, clip=TAU), 75657),
    "outside": (lambda: _case(sphere, (17, 17, 17), (3, 0, 0), 1.0 / 16, 4), 1),
    "sphere17_d7": (lambda: _case(sphere, (17, 17, 17), (0, 0, 0), 1.0 / 16, 7), 200905),
    # depth 12 in the corner away from the origin: block coordinates near 2^11 in the packed words, in the float of 2 * bx + li and
    # in the emit's doubling; the grid covers 1 - 20 sp .. 1 - 4 sp, so the cube's last four cells lie in the continuation
    "corner_d12": (lambda: _case(corner_sphere, (17, 17, 17), (1 - 20 * SP12,) * 3, SP12, 12), 12433),
    "corner_d12_f16": (lambda: _case(corner_sphere, (17, 17, 17), (1 - 20 * SP12,) * 3, SP12, 12, dtype=np.float16), 12433),
    # grids on the negative side.  wraps_d5: the cube strictly inside the grid's box and off its lattice (g = (p - o) * inv with o < 0
    # at every point).  inset_negative_d5: aniso_inset_d5's lattice moved to the middle of the cube along x and out of it on the
    # negative side along y, so e = (g - gc) * spacing is taken with g < 0 next to a surface inside the cube.  negative_scale_d4: a
    # field that is positive inside, sphere17_d4's grid negated with value_scale = -1
    "wraps_d5": (lambda: _case(sphere, (33, 37, 36), (-0.13, -0.21, -0.07), 0.037, 5), 13385),
    "inset_negative_d5": (lambda: _case(sphere, (21, 13, 9), (0.34, -0.17, 0.1), 0.04, 5), 4809),
    "negative_scale_d4": (lambda: _case(sphere, (17, 17, 17), (0, 0, 0), 1.0 / 16, 4, stored=-1.0), 3465),
    # 81^3 = 531 441 samples, more than the 524 288 threads k_volume_check strides with; the tree is sphere17_d4's: every point a
    # depth-4 build evaluates is a vertex of both lattices
    "sphere81_d4": (lambda: _case(sphere, (81, 81, 81), (0, 0, 0), 1.0 / 80, 4), 3465),
    # the edges of float16 among the samples, in cube units and with 2^16 to the unit
    "half_edges_d3": (lambda: _half_edges(1.0), 585),
    "half_edges_scaled_d3": (lambda: _half_edges(65536.0), 585),
}
NAMES = list(_MAKERS)
NODES = {name: nodes for name, (_, nodes) in _MAKERS.items()}
_cases, _restated = {}, {}


def case(name):
    if name not in _cases:
        _cases[name] = _MAKERS[name][0]()
    return _cases[name]


def restated(name):
    """(structs, values, counts) of the restatement, made once and left unchanged"""
    if name not in _restated:
        c = case(name)
        S, V, counts = vr.build(c["grid"], c["origin"], c["spacing"], c["depth"], c["value_scale"], want_counts=True)
        S.setflags(write=False); V.setflags(write=False)
        _restated[name] = (S, V, counts)
    return _restated[name]


def level_sizes(S):
    """the nodes of each level of a breadth-first tree"""
    sizes, level = [], np.zeros(1, dtype=np.int64)
    while len(level):
        sizes.append(len(level))
        kids = S[level, 1]
        kids = kids[kids >= 0].astype(np.int64)
        level = (kids[:, None] + np.arange(8)).reshape(-1)
    return sizes


def last_blocks(S):
    """the integer coordinates (n, 3), at their own depth, of the nodes whose children are the last level of a breadth-first tree:
    what the level builder packs into its last list of blocks"""
    level, coords, blocks = np.zeros(1, dtype=np.int64), np.zeros((1, 3), dtype=np.int64), None
    while True:
        inner = S[level, 1] >= 0
        if not inner.any():
            return blocks
        blocks = coords[inner]
        kids = S[level[inner], 1].astype(np.int64)
        level = (kids[:, None] + np.arange(8)).reshape(-1)
        coords = (2 * blocks[:, None, :] + vr.CORNER[None]).reshape(-1, 3)


def cells(S, V):
    """{(depth, x, y, z): the node's eight bytes}: a tree as its cells, whatever the order of its nodes"""
    out = {}
    level, coords, d = np.zeros(1, dtype=np.int64), np.zeros((1, 3), dtype=np.int64), 0
    while len(level):
        for n, c in zip(level, coords):
            out[(d, int(c[0]), int(c[1]), int(c[2]))] = V[n].tobytes()
        inner = S[level, 1] >= 0
        kids = S[level[inner], 1].astype(np.int64)
        level = (kids[:, None] + np.arange(8)).reshape(-1)
        coords = (2 * coords[inner][:, None, :] + vr.CORNER[None]).reshape(-1, 3)
        d += 1
    return out

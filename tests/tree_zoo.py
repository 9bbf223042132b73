"""Trees built to break a consumer, shared by the tests of the renderer, the queries, the mesh, the edit, the prune, the combination,
the placement, the measure, the volume read-out, the composition and the unbaked assembly calls.  A plain helper module
(like the *_restatement.py files): generators of consistent trees that no builder would lay out -- depth-first order, a chain along
one corner, blocks appended under randomly chosen leaves, node counts one past a kernel's chunk, row and wave -- byte fillers that are
no distance field, the named trees `zoo()` every zoo test uses, the edit cases of tests/test_tree_zoo.py and
tests/test_gpu_tree_zoo.py, the prune, combine, place and measure cases of tests/test_zoo_builders.py and
tests/test_gpu_zoo_builders.py, and the volume-out and compose cases of tests/test_zoo_volumes.py and tests/test_gpu_zoo_volumes.py,
with a cache of their restated results.  The assemblies of zoo trees that sdfhip_instances_* sample, march and draw without baking --
each tree under the identity, the list `keeps`, the skip's floor, ties, the instance limit, the launch edges -- live in
tests/instances_zoo_cases.py (tests/test_instances_zoo.py, tests/test_gpu_instances_zoo.py), which takes zoo(), compose_parts(),
DEEP_CORNER and restated() from here.

The volume-out and compose cases, and what each is for (measured CPU time of the restated answer beside it):
  out_lattices()    every tree of ALL_TREES, chain14 included, on a depth-3 tree's lattice, one that sticks out of the cube on every
                    side, one element, and DEEP_CORNER, 9^3 elements 2^-12 apart inside the chains' deepest cells (subnormal halves):
                    under 0.1 s each
  LONG_OUT          257^3 elements of blocks_1025, more than the 2^24 threads k_volume_out strides with; restated as slabs(0) and
                    slabs(254), 0.7 s each (the whole lattice: 50 s)
  COMPOSE_LISTS     csg (three ops on a depth-first tree, append order and the 12-deep chain: 0.1 s), keeps (the same as unions: the
                    arrays grow once, under 1 s at depth 5), repeated (one handle four times), leaf_blocks (one node against a tree),
                    chain14 (the walk over more than 12 levels, taken only with a depth given); each at COMPOSE_DEPTHS, 0.3 s at most
Their far-corner, long-grid, negative-side, half-precision and 4096-instance companions need no zoo tree and live in
tests/volume_cases.py and tests/compose_cases.py.

_random_tree and _chain_tree are the generators of tests/test_gpu_parity.py, moved here unchanged: their code and the order of their
RNG draws are what the parity fuzz seeds (the pinned seed 26 included) were found with."""
import numpy as np

import edit_restatement as er

LEAF_BYTES = [60, 80, 90, 120, 70, 200, 40, 255]           # the single leaf of test_degenerate_and_deep_trees
BLOCK_COUNTS = (8, 32, 127, 128, 256, 512)                  # 1 + 8k = 65, 257, 1017, 1025, 2049, 4097 nodes
NODE_CAP = 400_000                                          # no restated result (edit, prune, combine, place) may be larger


def _random_tree(rng, max_depth, p_split, max_nodes=60000):
    """A consistent octree with random splits (DFS pre-order, like SdfGen) and random bytes."""
    structs = [[-1, -1]]

    def grow(node, depth):
        if depth >= max_depth or len(structs) + 8 > max_nodes or rng.random() > p_split:
            return
        c = len(structs)
        structs[node][1] = c
        for _ in range(8):
            structs.append([node, -1])
        for k in range(8):
            grow(c + k, depth + 1)

    grow(0, 0)
    s = np.array(structs, dtype=np.int32)
    mode = rng.integers(3)
    if mode == 0:
        v = rng.integers(0, 256, size=(len(s), 8), dtype=np.uint8)
    elif mode == 1:      # mostly flat cells (exercises the flat fast path next to non-flat lanes)
        v = np.repeat(rng.integers(0, 256, size=(len(s), 1), dtype=np.uint8), 8, axis=1)
        noisy = rng.random(len(s)) < 0.2
        v[noisy] = rng.integers(0, 256, size=(int(noisy.sum()), 8), dtype=np.uint8)
    else:                # a crude distance-like field: larger values near the cube faces
        v = rng.integers(60, 200, size=(len(s), 8), dtype=np.uint8)
    return s, v


def _chain_tree(depth):
    """A consistent tree that is `depth` levels deep along the (0,0,0) corner."""
    rng = np.random.default_rng(depth)
    n = 1 + 8 * depth
    s = np.full((n, 2), -1, dtype=np.int32)
    for lvl in range(depth):
        node = 0 if lvl == 0 else 1 + 8 * (lvl - 1)       # child 0 of the previous block
        s[node, 1] = 1 + 8 * lvl
        s[1 + 8 * lvl: 9 + 8 * lvl, 0] = node
    v = rng.integers(40, 255, size=(n, 8), dtype=np.uint8)
    return s, v


# ---- byte fillers: values for any tree, none of them a distance field ------------------------------------------------------------
def fill_uniform(rng, n):
    """every byte uniform in 0..255"""
    return rng.integers(0, 256, size=(n, 8), dtype=np.uint8)


def fill_iso(rng, n):
    """only the saturated bytes and the two sides of the 63.75 iso level: 0, 63, 64, 255"""
    return np.array([0, 63, 64, 255], dtype=np.uint8)[rng.integers(0, 4, size=(n, 8))]


def fill_mostly_flat(rng, n):
    """mostly flat cells with noisy ones among them (_random_tree's mode 1)"""
    v = np.repeat(rng.integers(0, 256, size=(n, 1), dtype=np.uint8), 8, axis=1)
    noisy = rng.random(n) < 0.2
    v[noisy] = rng.integers(0, 256, size=(int(noisy.sum()), 8), dtype=np.uint8)
    return v


def fill_flat_63_64(rng, n):
    """every cell flat, all 63 or all 64: neighbouring cells disagree about inside and outside, and no cell is cut"""
    return np.repeat(np.array([63, 64], dtype=np.uint8)[rng.integers(0, 2, size=(n, 1))], 8, axis=1)


FILLERS = {"uniform": fill_uniform, "iso": fill_iso, "mostly_flat": fill_mostly_flat, "flat_63_64": fill_flat_63_64}


def tree_with_blocks(rng, k, max_depth):
    """A consistent tree of exactly 1 + 8 k nodes with random bytes: a randomly chosen leaf (of depth < max_depth) is split k times,
    each block of eight appended at the end -- blocks in the order of their making, not sorted by depth."""
    structs = [[-1, -1]]
    depth = [0]
    open_leaves = [0] if max_depth > 0 else []
    for _ in range(k):
        if not open_leaves:
            raise ValueError(f"tree_with_blocks: {k} blocks do not fit a tree of depth {max_depth}")
        at = int(rng.integers(len(open_leaves)))
        node = open_leaves[at]
        open_leaves[at] = open_leaves[-1]
        open_leaves.pop()
        c = len(structs)
        structs[node][1] = c
        for j in range(8):
            structs.append([node, -1])
            depth.append(depth[node] + 1)
            if depth[node] + 1 < max_depth:
                open_leaves.append(c + j)
    s = np.array(structs, dtype=np.int32)
    assert len(s) == 1 + 8 * k
    return s, fill_uniform(rng, len(s))


_zoo = {}


def zoo():
    """{name: (structs, values)}, made once.  Treat the arrays as read-only."""
    if _zoo:
        return _zoo
    z = {"leaf": (np.array([[-1, -1]], dtype=np.int32), np.array([LEAF_BYTES], dtype=np.uint8))}
    for d in (12, 14):
        s, _ = _chain_tree(d)
        z[f"chain{d}"] = (s, fill_uniform(np.random.default_rng(1000 + d), len(s)))
    for tag, seed, filler in (("a", 61, fill_uniform), ("b", 62, fill_iso)):
        rng = np.random.default_rng(seed)
        s, _ = _random_tree(rng, 6, 0.7, max_nodes=9000)
        z[f"dfs_d6_{tag}"] = (s, filler(rng, len(s)))
    # one node past the wave (64), the row (256) and the first, second and fourth chunk (1024) of the mesh passes, and one short of a chunk
    refill = {32: fill_iso, 127: fill_mostly_flat, 256: fill_flat_63_64}
    for k in BLOCK_COUNTS:
        rng = np.random.default_rng(2000 + k)
        s, v = tree_with_blocks(rng, k, 7)
        z[f"blocks_{1 + 8 * k}"] = (s, refill[k](rng, len(s)) if k in refill else v)
    for s, v in z.values():
        s.setflags(write=False); v.setflags(write=False)
    _zoo.update(z)
    return _zoo


MESHABLE = ["leaf", "chain12", "dfs_d6_a", "dfs_d6_b"] + [f"blocks_{1 + 8 * k}" for k in BLOCK_COUNTS]       # every tree but chain14
ALL_TREES = MESHABLE + ["chain14"]
EDITED = ["leaf", "chain12", "dfs_d6_a", "dfs_d6_b", "blocks_1025", "blocks_4097"]


def mesh_levels(depth):
    """the leaves, the root, a middle level, the tree's own depth and deeper than any tree"""
    return sorted({-1, 0, depth // 2, depth, 12})


# ---- the edit cases --------------------------------------------------------------------------------------------------------------
# On chain12 a brush may only be tiny and sit in the deep corner (a brush of r = 0.2 refined to depth 12 is tens of millions of
# nodes): centre (2^-11, 2^-11, 2^-11), r = 2^-9.  On the single leaf the brush must reach the root's corners to change a byte: r = 0.9.  Elsewhere r = 0.08 (placement below).
_CORNER = (2.0 ** -11,) * 3
_PLACE = {"leaf": ((0.45, 0.55, 0.5), 0.9), "chain12": (_CORNER, 2.0 ** -9)}


def placement(name):
    """(centre, radius) of the tree's brushes: the leaf's and chain12's are pinned above; on the other trees the centre of a leaf of
    the deepest level (where leaves of several depths meet, so that both operations find leaves to refine) and r = 0.08"""
    if name not in _PLACE:
        c, _ = er.deepest_leaf_centres(zoo()[name][0])
        _PLACE[name] = (tuple(float(x) for x in c[len(c) // 2]), 0.08)
    return _PLACE[name]


def max_depths(depth):
    """-1 (the input's depth) and two levels deeper, capped at 12"""
    return (-1, min(depth + 2, 12))


def single_edits(name):
    """[(label, (op, brush, params))]: carve and add, sphere and box, at the tree's placement"""
    c, r = placement(name)
    out = []
    for op, opname in ((er.EDIT_CARVE, "carve"), (er.EDIT_ADD, "add")):
        out.append((f"{opname} sphere", (op, er.BRUSH_SPHERE, (*c, r))))
        out.append((f"{opname} box", (op, er.BRUSH_BOX, (*c, r, 0.6 * r, 1.3 * r))))
    return out


def overlapping_chain(name, depth):
    """(A, max_depth of A, B, max_depth of B): A refines its region two levels past the input; B, the opposite operation, has its
    centre inside A's region, about A's surface, and may refine one level deeper still -- it walks, re-edits and splits the blocks A
    appended, which sit at the end of the arrays out of level order."""
    c, r = placement(name)
    r = r if name in ("leaf", "chain12") else 0.6 * r        # (A is refined three levels in the list form: a smaller brush)
    a = (er.EDIT_ADD, er.BRUSH_SPHERE, (*c, r))
    cb = (c[0] + 0.6 * r, c[1] + 0.3 * r, c[2] + 0.2 * r)
    b = (er.EDIT_CARVE, er.BRUSH_BOX, (*cb, 0.55 * r, 0.5 * r, 0.6 * r))
    return a, min(depth + 2, 12), b, min(depth + 3, 12)


_restated = {}


def restated(key, make):
    """a restatement's answer, computed once per process (the CPU tests and both library flavours of the GPU tests share it)"""
    if key not in _restated:
        _restated[key] = make()
    return _restated[key]


def walked(name):
    """mr.walk of the zoo tree `name` (every node's depth and coordinates), cached"""
    import mesh_restatement as mr
    return restated(("walk", name), lambda: mr.walk(zoo()[name][0]))


def restated_edit(name, edits, max_depth, start=None):
    """er.edit on the zoo tree `name` (or on the arrays `start` = (key, structs, values)), cached"""
    if start is None:
        s, v = zoo()[name]
        skey = None
    else:
        skey, s, v = start
    key = ("edit", name, skey, tuple((op, br, tuple(float(x) for x in p)) for op, br, p in edits), int(max_depth))
    return restated(key, lambda: er.edit(s, v, edits, max_depth))


def restated_chain(name):
    """The overlapping chain on the zoo tree `name`: ((S_A, V_A), (S_AB, V_AB)) of the two calls (A at its max_depth, then B at its
    own on A's result), and (S_L, V_L) of the list [A, B] at B's max_depth."""
    s, v = zoo()[name]
    d0 = er.tree_depth(s)
    a, md_a, b, md_b = overlapping_chain(name, d0)
    first = restated_edit(name, [a], md_a)
    second = restated_edit(name, [b], md_b, start=("after A", first[0], first[1]))
    as_list = restated_edit(name, [a, b], md_b)
    return first, second, as_list


# ---- the cases of prune, combine, place and measure (tests/test_zoo_builders.py, tests/test_gpu_zoo_builders.py) ------------------
# None of the four restatements was written with these trees in view; each answer is made once and shared, as the edits' are.
PRUNE_TOLERANCES = (0, 8, 255)
COMBINE_DEPTHS = (-1, 3)
# (a, b): two depth-first trees; append order against depth-first order; a shallow wide tree against the 12-deep chain; one node
# against a tree; one handle as both operands
COMBINE_PAIRS = [("dfs_d6_a", "dfs_d6_b"), ("blocks_4097", "dfs_d6_a"), ("blocks_1025", "chain12"), ("leaf", "blocks_257"),
                 ("chain12", "chain12")]
COMBINE_REVERSED = [("dfs_d6_a", "blocks_4097")]            # the difference is not symmetric: this pair the other way round too
# source -> the depths it is placed to.  Never the source's own: random bytes cut nearly every leaf, and a placement to depth 7 or 12
# would have millions of nodes.  The deeper ones grow the level builder's arrays (1.5 times the source at first) more than once.
PLACE_DEPTHS = {"leaf": (4,), "chain12": (4, 6), "blocks_65": (4, 5), "blocks_1025": (4,), "dfs_d6_a": (4, 6)}
PLACE_NAMES = ("identity", "dyadic_075", "generic_half")
PLACE_EXTRA = [("blocks_1025", "identity", 6)]              # 110 489 nodes from 1025


def prune_depths(depth):
    """no cut, the root alone, one level inside the tree"""
    return sorted({-1, 0, max(depth - 1, 0)})


def combine_cases():
    """[(a, b, op, max_depth)]: every pair under every operation and cut, and the reversed pair under the difference"""
    import combine_restatement as cr
    out = [(a, b, op, md) for a, b in COMBINE_PAIRS for op in cr.OPS for md in COMBINE_DEPTHS]
    return out + [(a, b, cr.COMBINE_SUBTRACT, md) for a, b in COMBINE_REVERSED for md in COMBINE_DEPTHS]


def place_cases(src=None):
    """[(source, placement, depth)] (of one source, if given)"""
    out = [(s, name, d) for s, depths in PLACE_DEPTHS.items() for name in PLACE_NAMES for d in depths] + PLACE_EXTRA
    return [c for c in out if src is None or c[0] == src]


def place_args(name):
    """(R, s, t): the identity; a dyadic scale and translation (a look-up lands on a lattice of the source four times finer than the
    result's); the generic two-axis rotation at half size about the cube's centre of tests/test_gpu_place.py"""
    import place_restatement as plr
    if name == "identity":
        return plr.IDENTITY, 1.0, (0.0, 0.0, 0.0)
    if name == "dyadic_075":
        return plr.IDENTITY, 0.75, (0.125, 0.0, 0.25)
    import sdfbox_amd
    if name == "turned_06":                                 # (the compositions' fourth: not among PLACE_NAMES)
        return sdfbox_amd.placement(70, -25, 40, 0.6, to=(0.55, 0.45, 0.5))
    assert name == "generic_half"
    return sdfbox_amd.placement(30, 20, 0, 0.5)


def restated_prune(name, tolerance, max_depth):
    import prune_restatement as pr
    return restated(("prune", name, tolerance, max_depth), lambda: pr.prune(*zoo()[name], tolerance, max_depth))


def restated_combine(a, b, op, max_depth):
    """(structs, values, counts)"""
    import combine_restatement as cr
    return restated(("combine", a, b, op, max_depth), lambda: cr.combine(zoo()[a], zoo()[b], op, max_depth, want_counts=True))


def restated_place(src, name, depth):
    """(structs, values, counts)"""
    import place_restatement as plr
    return restated(("place", src, name, depth), lambda: plr.place(zoo()[src], *place_args(name), depth, want_counts=True))


def restated_measure(name, level):
    import measure_restatement as ms
    return restated(("measure", name, level), lambda: ms.measure(*zoo()[name], level, walked=walked(name)))


# ---- the cases of volume out and compose (tests/test_zoo_volumes.py, tests/test_gpu_zoo_volumes.py) -------------------------------
# Volume out reads EVERY tree, chain14 included (the look-up is the sampler's, which walks any consistent tree), on four lattices: a
# depth-3 tree's own; one that sticks out of the cube on every side; one element; and 9^3 elements 2^-12 apart at the origin, inside the
# chains' deepest cells.  Each restates in under 0.1 s.
DEEP_CORNER = ((9, 9, 9), (0.0, 0.0, 0.0), 2.0 ** -12)
# Past k_volume_out's 2^16 workgroups of 256 threads: 257^3 = 16 974 593 elements.  Its positions are exact in float32, so three slabs
# of it are a lattice of their own, which restates in 0.7 s where the whole takes 50 s
LONG_OUT = ((257, 257, 257), (0.0, 0.0, 0.0), 2.0 ** -8)
LONG_OUT_SOURCE = "blocks_1025"


def out_lattices():
    from volume_cases import ONE, STICKS_OUT
    return [((9, 9, 9), (0, 0, 0), 0.125), STICKS_OUT, ONE, DEEP_CORNER]


def slabs(k0):
    """three slabs of LONG_OUT from slab k0 on, as a lattice of their own"""
    (nz, ny, nx), _, spacing = LONG_OUT
    return ((3, ny, nx), (0.0, 0.0, k0 * spacing), spacing)


def restated_out(name, lattice, dtype=np.float32):
    """vr.volume_out of the zoo tree `name` on `lattice`; the float16 form is the float32 form's rounding, as vr.volume_out makes it"""
    import volume_restatement as vr
    full = restated(("out", name, lattice), lambda: vr.volume_out(zoo()[name], *lattice))
    return full if np.dtype(dtype) == np.float32 else restated(("out16", name, lattice), lambda: full.astype(np.float16))


# The compositions: name -> [(source, placement name, op)], each at COMPOSE_DEPTHS.  csg: depth-first, append order and the chain
# under all three ops.  keeps: the same sources as unions, so that most of the tree stays and the result outgrows the arrays' start (1.5
# times the sources together) once.  repeated: ONE handle in four instances.  leaf_blocks: one node against a tree.  chain14: the
# 14-deep chain, which only a call with a depth given takes.
_U, _I, _S = 0, 1, 2
COMPOSE_DEPTHS = (4, 5)
COMPOSE_LISTS = {
    "csg": [("dfs_d6_a", "generic_half", _U), ("blocks_4097", "dyadic_075", _S), ("chain12", "identity", _I)],
    "keeps": [("chain12", "identity", _U), ("blocks_4097", "dyadic_075", _U), ("dfs_d6_a", "generic_half", _U)],
    "repeated": [("blocks_65", "identity", _U), ("blocks_65", "generic_half", _S), ("blocks_65", "dyadic_075", _U), ("blocks_65", "turned_06", _I)],
    "leaf_blocks": [("leaf", "identity", _U), ("blocks_257", "generic_half", _S)],
    "chain14": [("leaf", "identity", _U), ("chain14", "generic_half", _I)],
}
# the restatement's sizes at COMPOSE_DEPTHS (csg restates in 0.1 s, keeps at depth 5 in under 1 s: the build machine's CPU, as every time in this module)
COMPOSE_NODES = {"csg": (1545, 3265), "keeps": (4169, 23625), "leaf_blocks": (1937, 7161), "chain14": (1129, 2001), "repeated": (2177, 6121)}


def compose_cases():
    """[(list name, depth)]"""
    return [(name, d) for name in COMPOSE_LISTS for d in COMPOSE_DEPTHS]


def compose_parts(name):
    """[(source name, (R, s, t), op)]"""
    return [(src, place_args(pl), op) for src, pl, op in COMPOSE_LISTS[name]]


def restated_compose(name, depth):
    """(structs, values, counts)"""
    import compose_restatement as cpr
    return restated(("compose", name, depth), lambda: cpr.compose([(zoo()[src], pl, op) for src, pl, op in compose_parts(name)], depth, want_counts=True))

"""The cases of tests/instances_zoo_cases.py are what they are for, by the restatement alone (tests/instances_restatement.py): each zoo
tree under the identity shows every kind of pixel and status it was chosen for, `keeps` has three winners, `floor` reaches the
skip's floor exactly and sends its instances through all three classes of the skip, a repeated last entry never wins and changes
nothing, `signtie` folds opposite zeros, the long lists folded over their distinct pairs are the plain restatement's bits, the launch
edges are where the kernels' workgroups end, and the far points are finite.  No GPU: tests/test_gpu_instances_zoo.py holds the GPU to
these same answers, bit for bit."""
import numpy as np
import pytest

import compose_cases as cc
import compose_restatement as cr
import edit_restatement as er
import instances_cases as ic
import instances_restatement as ir
import instances_zoo_cases as zc
import query_restatement as qr
import tree_zoo as tz
from conftest import bits_equal

f32 = np.float32
ALL3 = {qr.HIT, qr.ESCAPED, qr.EXHAUSTED}


def pixel_kinds(frame):
    """(sky, lit, black) counts of a frame"""
    sky = frame[..., 2] == f32(0.2)
    return int(sky.sum()), int((~sky & (frame[..., 0] > 0)).sum()), int((~sky & (frame[..., 0] == 0)).sum())


def test_every_case_has_the_frame_and_the_batches_the_kernels_have_not_met():
    for name in zc.FULL:
        assert zc.size(name) == ic.FRAME_LONG and len(zc.points(name)) == 333 and zc.max_steps(name) == 100, name
        assert np.array_equal(zc.pixels(name), ic.pixels("inside")), name
        probes, hits = zc.restated(name, "sample"), zc.restated(name, "raycast")
        assert (probes["status"] == qr.INVALID).sum() == 2 and (hits["status"] == qr.INVALID).sum() == 3, name
    assert {f"one:{src}" for src in zc.ONE_TREES} <= set(zc.FULL) and {"keeps", "keeps:rotated", "floor", "signtie"} <= set(zc.FULL) and set(zc.TIES) <= set(zc.FULL)
    assert er.tree_depth(zc.tree("chain12")[0]) == 12 and er.tree_depth(zc.tree("chain14")[0]) == 14
    for n in zc.LIMITS:
        assert len(zc.parts(f"limit_{n}")) == n and len(zc.points(f"limit_{n}")) == 77
    assert zc.LIMITS == (63, 64, 4096)


@pytest.mark.parametrize("src", ["dfs_d6_b", "blocks_257", "blocks_1017", "blocks_4097"])
def test_a_tree_of_random_bytes_shows_every_pixel_and_every_status(src):
    name = f"one:{src}"
    sky, lit, black = pixel_kinds(zc.restated(name, "frame"))
    assert sky and lit and black and sky + lit + black == 23 * 17, (sky, lit, black)
    pick = zc.restated(name, "pick")
    assert set(pick["status"].tolist()) == ALL3 and pick["steps"].max() == 100
    assert zc.restated(name, "frame")[..., 3].max() > 100            # the shadow's steps on top of the march's
    nan_normals = int(np.isnan(pick["normal"]).any(1).sum())
    # mostly flat cells: a zero gradient, normalised, is 0 * inf
    assert nan_normals == (3 if src == "blocks_1017" else 0)
    # under the identity, inside the cube, the value is the source's own sampled distance
    p = zc.points(name)
    inside = np.isfinite(p).all(1) & ((p >= 0) & (p <= 1)).all(1)
    assert inside.sum() > 50
    assert bits_equal(zc.restated(name, "sample")["value"][inside], qr.sample(*zc.tree(src), p[inside])["distance"]).all()


def test_flat_cells_on_both_sides_of_the_iso_level_are_black_after_one_step_and_march_from_inside():
    out, inside = zc.restated("one:blocks_2049", "frame"), zc.restated("one:blocks_2049:inside", "frame")
    assert pixel_kinds(out) == (0, 0, 391) and (out[..., 3] == 1).all()
    assert pixel_kinds(inside) == (0, 0, 391) and inside[..., 3].max() == 41
    V = zc.tree("blocks_2049")[1]
    assert (V == V[:, :1]).all() and set(np.unique(V).tolist()) == {63, 64}


def test_the_chains_are_mostly_sky_and_their_corner_batch_is_the_volume_restatements():
    for src, sky in (("chain12", 343), ("chain14", 378)):
        assert pixel_kinds(zc.restated(f"one:{src}", "frame"))[0] == sky
        got = zc.restated(f"corner:{src}", "sample")
        assert len(got) == 729 and (got["status"] == qr.HIT).all() and not got["instance"].any()
        # another route to the same look-up: the volume read-out's restatement on the same lattice
        assert bits_equal(got["value"], tz.restated_out(src, tz.DEEP_CORNER).reshape(-1)).all(), src
        assert len(np.unique(got["value"])) > 100, "the deepest cells, not one flat one"


def test_keeps_has_three_winners_every_status_and_lit_pixels_from_both_cameras():
    for name, lit in (("keeps", 8), ("keeps:rotated", 58)):
        assert pixel_kinds(zc.restated(name, "frame"))[1] == lit, name
        assert set(zc.restated(name, "pick")["status"].tolist()) == ALL3, name
    winners = set(zc.restated("keeps", "sample")["instance"].tolist()) | set(zc.restated("keeps", "pick")["instance"].tolist())
    assert winners == {0, 1, 2}
    assert [src for src, _, _ in zc.parts("keeps")] == ["chain12", "blocks_4097", "dfs_d6_a"]


def skip_classes(inst, p):
    """per instance k >= 1 of a list of unions and differences: (skipped, looked up and lost, won) counts over points p, and whether
    b_k <= u_k everywhere"""
    out = {}
    for k in range(1, len(inst)):
        v = ir.value(inst[:k], p)
        b, u = ir.bound(inst[k], p)
        op = inst[k][2]
        assert op != cr.COMBINE_INTERSECT
        skipped = b > v if op == cr.COMBINE_UNION else -b < v
        won = u < v if op == cr.COMBINE_UNION else -u > v
        assert not (skipped & won).any(), "the skip would change a bit"
        out[k] = (int(skipped.sum()), int((~skipped & ~won).sum()), int(won.sum()), bool((b <= u).all()))
    return out


def test_floor_reaches_the_skips_floor_and_takes_both_branches_of_the_skip():
    inst = zc.instances("floor")
    assert np.array_equal(np.unique(zc.tree("leaf0")[1]), [0]) and np.array_equal(np.unique(zc.tree("leaf255")[1]), [255])
    classes = skip_classes(inst, zc.visited("floor"))
    print("floor: instance -> (skipped, looked up and lost, won, b <= u):", classes)
    for k in (1, 2):
        assert all(n > 0 for n in classes[k][:3]), (k, classes[k])
    assert classes[3][0] == 0 and classes[3][2] == 0 and classes[3][1] == len(zc.visited("floor"))
    assert all(c[3] for c in classes.values())
    # the floor itself: inside leaf0's placed cube e = 0 and D = -0.5 exactly, so u_k / s = -0.5 -- and nothing reads lower
    p = zc.points("floor")
    p = p[np.isfinite(p).all(1)]
    lowest = min(float((ir.bound(inst[k], p)[1] / inst[k][1][1]).min()) for k in range(len(inst)))
    assert lowest == -0.5
    for k in (1, 2):
        assert ((ir.bound(inst[k], p)[1] / inst[k][1][1]) == f32(-0.5)).sum() >= 12, k     # the twelve put there, and what the random batch adds
    assert ir.SKIP_FLOOR < -0.5
    assert set(zc.restated("floor", "pick")["status"].tolist()) == ALL3 and set(zc.restated("floor", "sample")["instance"].tolist()) == {0, 1, 2}


@pytest.mark.parametrize("name", zc.TIES)
def test_a_repeated_last_entry_never_wins_and_changes_nothing(name):
    base = zc.BASES[name]
    n = len(zc.parts(name))
    assert zc.parts(name)[-1][0] == zc.parts(name)[-2][0] and zc.parts(name)[-1][2] == zc.parts(name)[-2][2] and len(zc.parts(base)) == n - 1
    won_before = False
    for kind in ("sample", "raycast", "pick"):
        got, want = zc.restated(name, kind), zc.restated(base, kind)
        assert (got["instance"] < n - 1).all(), (kind, "ties keep the earlier instance")
        won_before |= bool((got["instance"] == n - 2).any())
        # every field, the value of the twice-subtracted list included: fmax(fmax(v, -u), -u) = fmax(v, -u)
        assert not qr.records_differ(got, want), kind
    assert won_before, "the entry that is repeated decides the value somewhere: a tie is met"
    assert bits_equal(zc.restated(name, "frame"), zc.restated(base, "frame")).all()


def test_signtie_folds_opposite_zeros():
    z = zc.zero_points()
    print("signtie:", len(z), "points of the draw read exactly 0")
    assert len(z) >= 8
    D = qr.sample(*zc.tree("dfs_d6_b"), z)["distance"]
    assert (D == 0).all() and not np.signbit(D).any(), "u = +0, so the fold is fmax(+0, -0)"
    p, got = zc.points("signtie"), zc.restated("signtie", "sample")
    at = np.nonzero((p[:, None, :] == z[None]).all(2).any(1))[0]
    assert len(at) == len(z) and (got["status"][at] == qr.HIT).all()
    # the header pins the zero C leaves open: fmaxf orders -0 below +0 (np.fmax alone returns its second operand, -0)
    assert (got["value"][at] == 0).all() and not np.signbit(got["value"][at]).any()
    with np.errstate(all="ignore"):
        pz, nz = f32(0.0) * np.ones(3, f32), f32(-0.0) * np.ones(3, f32)
    for a, b in ((pz, nz), (nz, pz)):
        assert not np.signbit(cr.fmaxf(a, b)).any() and np.signbit(cr.fminf(a, b)).all()
    assert np.signbit(cr.fmaxf(nz, nz)).all() and not np.signbit(cr.fminf(pz, pz)).any()
    x = np.array([np.nan, 1.0, -2.0, 0.0], f32)
    assert bits_equal(cr.fmaxf(x, x[::-1].copy()), np.fmax(x, x[::-1])).all() and bits_equal(cr.fminf(x, x[::-1].copy()), np.fmin(x, x[::-1])).all()
    assert [op for _, _, op in zc.parts("signtie")] == [cr.COMBINE_UNION, cr.COMBINE_SUBTRACT]


@pytest.mark.parametrize("n", [64, 130])
def test_the_fold_over_distinct_pairs_is_the_plain_restatements_bits(n):
    name = f"limit_{n}"
    folded = zc.instances(name)
    plain = list(folded)
    assert isinstance(folded, ir.Folded) and not isinstance(plain, ir.Folded)
    cam = zc.camera(name).State
    assert not qr.records_differ(zc.restated(name, "sample"), ir.sample(plain, zc.points(name)))
    assert not qr.records_differ(zc.restated(name, "pick"), ir.pick(plain, cam, zc.pixels(name), zc.max_steps(name)))
    p = zc.points(name)
    p = p[np.isfinite(p).all(1)]
    assert bits_equal(ir.value(folded, p), cc.folded_value(plain, p)).all()


def test_the_longest_list_has_late_winners():
    got = zc.restated(f"limit_{cc.LIMIT}", "sample")
    winners = set(got["instance"].tolist())
    assert len(winners) >= 10 and max(winners) == cc.LIMIT - 1
    assert len(set(zc.restated(f"limit_{cc.LIMIT}", "pick")["instance"].tolist())) >= 4
    assert len({(src, pl[0].tobytes(), pl[2].tobytes()) for src, pl, _ in zc.parts(f"limit_{cc.LIMIT}")}) == 16


def test_the_launch_edges_are_the_kernels():
    assert zc.EDGE_COUNTS == (1, 255, 256, 257, 513) and len(zc.points("edge")) == 513 == len(zc.rays("edge")[0])
    probes, hits = zc.restated("edge", "sample"), zc.restated("edge", "raycast")
    # the refused elements sit on the workgroup's edge; the rest of the batch is answered
    assert probes["status"][255] == probes["status"][256] == qr.INVALID and (probes["status"] == qr.HIT).sum() == 511
    assert hits["status"][253] == qr.ESCAPED and hits["steps"][253] == 0 and (hits["status"][254:257] == qr.INVALID).all()
    assert set(hits["status"].tolist()) == ALL3 | {qr.INVALID} and set(probes["instance"].tolist()) == {0, 1, 2}
    for (w, h), tiles in zc.EDGE_FRAMES.items():
        assert -(-w // 8) * -(-h // 8) == tiles and zc.restated(f"edge:{w}x{h}", "frame").shape == (h, w, 4)
    assert sorted(zc.EDGE_FRAMES.values()) == [1, 1, 2, 5]


def test_the_far_points_are_finite_and_their_answers_are_not():
    p, got = zc.points("far"), zc.restated("far", "sample")
    assert len(p) == 16 and np.isfinite(p).all() and (got["status"] == qr.HIT).all()
    big = np.abs(p).max(1)
    assert {1e19, 2e19, 3e38} == {float(f"{x:.0e}") for x in big.tolist()}
    with np.errstate(all="ignore"):
        assert np.isfinite(f32(1e19) * f32(1e19)) and np.isinf(f32(2e19) * f32(2e19)) and np.isnan(f32(0) * (f32(3e38) * f32(3e38)))
    print("far: values", got["value"].tolist(), "gradients with a NaN:", int(np.isnan(got["gradient"]).any(1).sum()))
    assert not np.isfinite(got["value"]).all() or np.isnan(got["gradient"]).any(), "the overflow reaches the answer"

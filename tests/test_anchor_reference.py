"""The numpy restatement tests/anchor_ref.py of the anchor-clustering rule (include/dyk_hip.h) against what the reference's
other_utils/anchor_cluster.py computed (tests/golden/anchor_cluster.npz, written by tests/golden/make_anchor_golden.py),
against hand-worked cases, and against wrong readings of the rule, each of which a NAMED case of tests/anchor_cases.py
flags.  No GPU: this file establishes the yardstick that tests/test_gpu_anchor_cluster.py holds the device entries to."""
import os
import random

import numpy as np
import pytest

import anchor_cases as C
import anchor_ref as R

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anchor_cluster.npz"))
SIZES = [int(n) for n in GOLDEN["sizes"]]
K, THR = int(GOLDEN["k"]), float(GOLDEN["thr"])


def golden_boxes(n):
    return np.exp(np.random.RandomState(0).randn(n, 2) * 0.6 + 3.3).astype(np.float32)


@pytest.mark.parametrize("n", SIZES)
def test_k_means_equals_the_reference_bit_for_bit(n):
    """the reference's arithmetic is elementwise fp32 in this order, so equality is exact; no cluster empties on these inputs"""
    np.random.seed(1)
    c, iters, empties = R.k_means(golden_boxes(n), K)
    assert c.dtype == np.float32 and np.array_equal(c, GOLDEN["centres_%d" % n])
    assert iters == int(GOLDEN["iterations_%d" % n]) and empties == []


@pytest.mark.parametrize("n", SIZES)
def test_fitness_against_the_reference(n):
    """Counts are exact.  fit_boxes: both values are fp64 sums of the same N terms in [0, 1], divided by N; the terms are
    identical (the same two divisions and minima), only the order of the additions differs (the header's order here, numpy's
    pairwise mean there).  Any order of N non-negative fp64 additions is within (N - 1) u of the exact sum relatively,
    u = 2^-53, so the two differ by at most 2 (N - 1) u S; the division by N adds u each.  Bound: 2 N 2^-53 value.
    fit_anchors is the same with K = 9 terms: the rule adds them in anchor order, numpy's mean of 9 adds them pairwise
    (eight accumulators from n = 8 on), so the two need not be equal bit for bit.  Bound: 2 K 2^-53 value."""
    wh, c = golden_boxes(n), GOLDEN["centres_%d" % n].astype(np.float64)
    f = R.fitness(wh, c, THR)
    g = float(GOLDEN["fit_boxes_%d" % n])
    print("N=%d fit_boxes %r golden %r diff %.3g bound %.3g" % (n, f["fit_boxes"], g, abs(f["fit_boxes"] - g), 2 * n * 2.0 ** -53 * g))
    assert f["hit_boxes"] == int(GOLDEN["hit_boxes_%d" % n]) and f["hit_anchors"] == int(GOLDEN["hit_anchors_%d" % n])
    assert abs(f["fit_boxes"] - g) <= 2 * n * 2.0 ** -53 * g
    ga = float(GOLDEN["fit_anchors_%d" % n])
    print("N=%d fit_anchors %r golden %r diff %.3g bound %.3g" % (n, f["fit_anchors"], ga, abs(f["fit_anchors"] - ga), 2 * K * 2.0 ** -53 * ga))
    assert abs(f["fit_anchors"] - ga) <= 2 * K * 2.0 ** -53 * ga
    assert 0.7 < f["fit_boxes"] < 0.8 < 0.96 < f["fit_anchors"]      # the swapped call scores near 1 whatever the anchors


def test_ordered_sum_is_the_exact_sum_for_exact_terms():
    """terms that are multiples of 2^-10 add without rounding in any order: the order restated must lose or repeat no box"""
    for n in (1, 63, 64, 65, 1023, 1024, 1025, 4099, C.N_FOLD_EDGE):
        t = np.random.RandomState(n).randint(0, 1024, n) / 1024.0
        assert R.ordered_sum(t) == t.sum()
    assert np.array_equal(R.draw_factors((2, 2), 0), np.empty((0, 2, 2)))


# ------------------------------------------------------------------------------------------------ hand-worked cases
@pytest.mark.parametrize("T", C.DTYPES)
def test_hand_worked_assignment_and_median(T):
    wh, c = C.named_cases(T)["even_count"]
    nearest, counts, changed = R.assign(wh, c)
    assert nearest.tolist() == [0, 0, 0, 0, 1, 1, 1] and counts.tolist() == [4, 3] and changed == 3
    # cluster 0: w 1 2 4 8 -> (2 + 4) / 2, h 5 6 7 8 -> (6 + 7) / 2; cluster 1 (odd): w 50 60 70, h 50 60 70
    assert R.median(wh, nearest, c).tolist() == [[3.0, 6.5], [60.0, 60.0]]
    wh, c = C.named_cases(T)["per_coordinate"]
    assert R.median(wh, np.zeros(3, np.int32), c).tolist() == [[5.0, 5.0]]
    # box (2,2) against (4,4): inter 4, union 4 + 16 - 4, iou 0.25, d 0.75; against (2,8): inter 4, union 16: the same
    d = R.distances(np.array([[2, 2]], T), np.array([[4, 4], [2, 8]], T))
    assert d.tolist() == [[0.75, 0.75]] and R.assign(np.array([[2, 2]], T), np.array([[4, 4], [2, 8]], T))[0].tolist() == [0]


@pytest.mark.parametrize("T", C.DTYPES)
def test_hand_worked_empty_cluster_and_early_exit(T):
    wh, c = C.named_cases(T)["equal_centres"]
    nearest, counts, _ = R.assign(wh, c)
    assert counts[2] == 0 and counts[1] > 0 and counts.sum() == len(wh)
    new = R.median(wh, nearest, c)
    assert np.array_equal(new[2], c[2]) and np.isfinite(new).all()
    out, iters, empties = R.k_means(wh, init=c)
    assert 2 in empties and np.isfinite(out).all()
    wh, c = C.named_cases(T)["all_cluster0"]
    nearest, counts, changed = R.assign(wh, c)
    assert changed == 0 and counts.tolist() == [len(wh), 0, 0]
    out, iters, _ = R.k_means(wh, init=c)
    assert iters == 1 and np.array_equal(out, c)             # the reference's quirk: the initial centres come back


def test_hand_worked_fitness():
    wh, a, thr = C.named_fitness_cases()["thr_exact"]
    f = R.fitness(wh, a[0], thr)
    # box (2,2): 0.25, not above thr; box (4,4): 0.5.  boxes: (0 + 0.5) / 2; anchors: t = 0.5
    assert f == {"fit_boxes": 0.25, "hit_boxes": 1, "fit_anchors": 0.5, "hit_anchors": 1}
    wh, a, thr = C.named_fitness_cases()["double_rounding"]
    assert R.fitness(wh, a[0], thr)["fit_boxes"] == 1.0 / (9.0 / 7.0) != 7.0 / 9.0
    # two anchors, three boxes: x = [[0.5, 0.25], [1, 0.5], [0.1, 0.2]]; b = 0.5, 1, 0.2; t = 1, 0.5
    f = R.fitness(np.array([[4, 8], [8, 8], [80, 8]], np.float32), np.array([[8, 8], [16, 16]], np.float64), 0.25)
    assert f == {"fit_boxes": 0.5, "hit_boxes": 2, "fit_anchors": 0.75, "hit_anchors": 2}


# ------------------------------------------------------------------------------------------------ wrong readings, each flagged by a named case
def _nearest(T, case, variant=None):
    wh, c = C.named_cases(T)[case]
    return R.assign(wh, c, variant=variant)[0].tolist()


@pytest.mark.parametrize("T", C.DTYPES)
def test_wrong_assignments_are_flagged(T):
    assert _nearest(T, "equal_centres") != _nearest(T, "equal_centres", "last_minimum")          # the last minimum on ties
    # argmax(iou): the two iou differ, 1 - iou is 1 for both, and that tie counts
    assert _nearest(T, "rounding_tie") == [0, 0] and _nearest(T, "rounding_tie", "argmax_iou") == [1, 1]
    assert _nearest(T, "fma_denominator") == [0] and _nearest(T, "fma_denominator", "fma_denominator") == [1]


@pytest.mark.parametrize("T", C.DTYPES)
def test_wrong_medians_are_flagged(T):
    wh, c = C.named_cases(T)["even_count"]
    nearest = R.assign(wh, c)[0]
    assert not np.array_equal(R.median(wh, nearest, c), R.median(wh, nearest, c, "lower_middle"))
    wh, c = C.named_cases(T)["per_coordinate"]
    assert not np.array_equal(R.median(wh, np.zeros(3, np.int32), c), R.median(wh, np.zeros(3, np.int32), c, "median_area_member"))
    wh, c = C.named_cases(T)["equal_centres"]
    nearest = R.assign(wh, c)[0]
    good = R.median(wh, nearest, c)
    for v in ("empty_zero", "empty_nan"):
        assert not np.array_equal(good, R.median(wh, nearest, c, v), equal_nan=True)


def test_wrong_fitness_and_acceptance_are_flagged():
    wh, a, thr = C.named_fitness_cases()["thr_exact"]
    assert R.fitness(wh, a[0], thr) != R.fitness(wh, a[0], thr, "ge_thr")
    wh, a, thr = C.named_fitness_cases()["double_rounding"]
    assert R.fitness(wh, a[0], thr)["fit_boxes"] != R.fitness(wh, a[0], thr, "a_over_w")["fit_boxes"]
    wh, a, thr = C.named_fitness_cases()["flat_fitness"]
    random.seed(5)
    np.random.seed(5)
    v = R.draw_factors(a[0].shape, 12)
    k0, f0, n0 = R.evolve(wh, a[0], thr, 12, factors=v)
    k1, f1, n1 = R.evolve(wh, a[0], thr, 12, factors=v, variant="accept_ge")
    assert (f0, n0, f1, n1) == (0.0, 0, 0.0, 12) and np.array_equal(k0, a[0]) and not np.array_equal(k1, a[0])


# ------------------------------------------------------------------------------------------------ the module's host parts
def test_seeded_draws_equal_the_restatement():
    from other_utils import anchor_cluster as A
    for shape, gen in (((9, 2), 40), ((1, 2), 25), ((32, 2), 3)):
        random.seed(11)
        np.random.seed(12)
        a = A.draw_factors(shape, gen)
        tail_a = (random.random(), np.random.random())
        random.seed(11)
        np.random.seed(12)
        b = R.draw_factors(shape, gen)
        assert a.shape == (gen,) + shape and np.array_equal(a, b) and tail_a == (random.random(), np.random.random())
        assert ((a >= 0.3) & (a <= 3.0)).all() and not (a == 1).all(axis=(1, 2)).any()


def test_wh_iou_is_the_distance_of_the_rule():
    from other_utils import anchor_cluster as A
    for T in C.DTYPES:
        wh, c = C.boxes(65, T), C.centres(C.boxes(65, T), 9)
        assert np.array_equal(T(1) - A.wh_iou(wh, c), R.distances(wh, c))

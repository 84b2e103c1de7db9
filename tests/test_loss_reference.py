"""oracle/loss.py loss_reference, the fp64 reference of the YOLO loss kernels, its input families and the bound of the per-element
GPU test (no GPU):
  * in float32 the reference is oracle.loss.compute_loss plus autograd, bit for bit, on every existing fixture case, and in
    float64 it stays within the fixtures' 1e-5 of the reference project's own outputs (loss.npz, loss_focal.npz);
  * conditioning cap: on every family the fp32 evaluation is finite and within 1e-6 (of the largest element of each head's
    box / objectness / class gradients, relative for the three scalars) of the fp64 one -- so 8 x that, the bound of
    tests/test_gpu_loss_elements.py, is a tight bound and not a licence;
  * every family provably takes the path it is named for (chunks, > 256 / > 4096 matches, chains across chunks, the v3 clamp,
    disjoint boxes, targets outside the grid);
  * the bound is not vacuous: each of eight plausible mistakes exceeds it on a named family and group."""
import os
import sys

import numpy as np
import pytest
import torch

from helpers import GOLDEN, loss_family

sys.path.insert(0, GOLDEN)
import cases  # noqa: E402

from oracle import loss as oloss  # noqa: E402

FAMILIES = list(oloss.LOSS_FAMILIES)
FID = ["%s-%d" % f for f in FAMILIES]
SCALARS = ("box_loss", "obj_loss", "class_loss")
CAP = 1e-6


def _anchor_vecs(cfg):
    anchors, strides, v4 = cases.head_geometry(cfg)
    return [torch.tensor(a, dtype=torch.float32) / s for a, s in zip(anchors, strides)], v4


def _fixture_case(case):
    av, v4 = _anchor_vecs(case["cfg"])
    hyp = cases.load_hyp(case["hyp"])
    if "fl_gamma" in case:
        hyp = dict(hyp, fl_gamma=case["fl_gamma"])
    return cases.loss_preds(case), cases.loss_targets(case), av, hyp, v4


ALL_FIXTURES = cases.loss_cases() + cases.focal_loss_cases()


# ------------------------------------------------------------------ tie to the existing oracle and the reference's fixtures
@pytest.mark.parametrize("case", ALL_FIXTURES, ids=lambda c: c["name"])
def test_fp32_reference_is_compute_loss_plus_autograd(case):
    """same operations in the same order: equal bits.  The explicit last-match-wins loop leaves what index_put_ leaves."""
    p, tg, av, hyp, v4 = _fixture_case(case)
    leaves = [t.clone().requires_grad_(True) for t in p]
    tobj = []
    out = oloss.compute_loss(leaves, tg, av, hyp, case["nc"], case["gr"], v4, tobj_out=tobj)
    (out["box_loss"] + out["obj_loss"] + out["class_loss"]).backward()
    ref = oloss.loss_reference(p, tg, av, hyp, case["nc"], case["gr"], v4, dtype=torch.float32)
    for k in SCALARS:
        assert ref[k].dtype == torch.float32 and torch.equal(ref[k], out[k].detach()[0]), k
    for h in range(3):
        assert torch.equal(ref["grads"][h], leaves[h].grad), h
        assert torch.equal(ref["tobj"][h], tobj[h]), h
        assert bool(ref["valid"][h].all())


def test_last_match_wins_is_exercised_by_the_fixtures():
    """some fixture case has a cell shared by two matches with different IoUs: there first-match-wins gives another tobj"""
    differs = 0
    for case in ALL_FIXTURES:
        p, tg, av, hyp, v4 = _fixture_case(case)
        args = (p, tg, av, hyp, case["nc"], case["gr"], v4)
        a, b = oloss.loss_reference(*args, dtype=torch.float32), oloss.loss_reference(*args, dtype=torch.float32, mistake="first_match_wins")
        differs += any(not torch.equal(x, y) for x, y in zip(a["tobj"], b["tobj"]))
    assert differs >= 2


@pytest.mark.parametrize("case", ALL_FIXTURES, ids=lambda c: c["name"])
def test_fp64_reference_stays_within_the_fixtures_tolerance(case):
    """the bounds tests/test_gpu_loss_nms.py holds the kernels to, against the reference project's own fp32 outputs"""
    gold = np.load(os.path.join(GOLDEN, "loss_focal.npz" if "fl_gamma" in case else "loss.npz"))
    p, tg, av, hyp, v4 = _fixture_case(case)
    ref = oloss.loss_reference(p, tg, av, hyp, case["nc"], case["gr"], v4)
    assert all(ref[k].dtype == torch.float64 for k in SCALARS) and all(g.dtype == torch.float64 for g in ref["grads"])
    got = np.array([float(ref[k]) for k in SCALARS])
    assert np.allclose(got, gold[case["name"] + "|losses"], rtol=1e-5, atol=1e-6), (got, gold[case["name"] + "|losses"])
    for i, g in enumerate(ref["grads"]):
        want = gold[case["name"] + "|dp%d" % i]
        err = np.abs(g.numpy() - want).max()
        assert err <= 1e-5 * max(1.0, np.abs(want).max()) + 1e-7, (i, err)


# ------------------------------------------------------------------ the families
def test_families_are_deterministic_and_cover_the_parameters():
    seen = {k: set() for k in ("cfg", "nc", "gr", "obj_pw", "cls_pw", "fl_gamma")}
    for kind, seed in FAMILIES:
        cfg, nc, over, gr, p, t = oloss.loss_input_family(kind, seed)
        cfg2, nc2, over2, gr2, p2, t2 = oloss.loss_input_family(kind, seed)
        assert (cfg, nc, over, gr) == (cfg2, nc2, over2, gr2) and torch.equal(t, t2) and all(torch.equal(a, b) for a, b in zip(p, p2))
        B = 2 if kind == "huge" else 4
        assert [tuple(x.shape) for x in p] == cases.head_shapes(cfg, B, oloss.FAMILY_H, oloss.FAMILY_W, 5 + nc)
        assert t.dtype == torch.float32 and t.shape[1] == 6 and float(t[:, 0].max()) < B and float(t[:, 1].max()) < nc
        for k, v in dict(over, cfg=cfg, nc=nc, gr=gr).items():
            seen[k].add(v)
    assert seen["cfg"] == {oloss.V3_CFG, oloss.V4_CFG} and seen["nc"] == {1, 2, 3} and seen["gr"] == {0.0, 0.5, 1.0}
    assert seen["obj_pw"] == {1.0, 1.7} and seen["cls_pw"] == {1.0, 0.6} and seen["fl_gamma"] == {0.0, 1.5}
    assert {k for k, _ in FAMILIES} == set(oloss.LOSS_KINDS)
    assert sum(k == "huge" for k, _ in FAMILIES) == 1
    assert {len(oloss.loss_input_family("chunk_edges", s)[5]) for k, s in FAMILIES if k == "chunk_edges"} == {85, 86, 171}


@pytest.mark.parametrize("kind,seed", FAMILIES, ids=FID)
def test_conditioning_cap_fp32_reference_within_1e_6_of_fp64(kind, seed):
    f = loss_family(kind, seed)
    r32, r64 = f["r32"], f["r64"]
    assert all(bool(torch.isfinite(g).all()) for g in r32["grads"] + r64["grads"] + r32["tobj"])
    err = oloss.loss_errors(r32, r64)
    worst = {k: "%.2e" % v[0] for k, v in err.items()}
    print("%s-%d fp32 vs fp64, max-normalised per group / relative per scalar: %s" % (kind, seed, worst))
    for h in range(3):
        for name, sl in oloss.channel_groups(5 + f["nc"]).items():
            key = "head%d.%s" % (h, name)
            assert err[key][0] <= CAP, (key, err[key])
            if not bool(r64["grads"][h][..., sl].any()):
                assert not bool(r32["grads"][h][..., sl].any()), key
    for k in SCALARS:
        assert err[k][0] <= CAP, (k, err[k])
        if float(r64[k]) == 0.0:
            assert float(r32[k]) == 0.0
    # the match lists and the structure of tobj do not depend on the precision
    for h in range(3):
        assert torch.equal(r32["tobj"][h] != 0, r64["tobj"][h] != 0) or f["gr"] > 0      # (gr > 0: a clamped IoU may be 0)


# ------------------------------------------------------------------ every family takes the path it is named for
def _chains(f, h):
    """{cell: [pair positions of its matches]} over the in-range matches of head h"""
    r = f["r64"]
    ok = r["valid"][h]
    b, a, gj, gi = [x[ok].tolist() for x in r["matches"][2][h]]
    out = {}
    for cell, pos in zip(zip(b, a, gj, gi), r["pairs"][h][ok].tolist()):
        out.setdefault(cell, []).append(pos)
    return out


@pytest.mark.parametrize("kind,seed", FAMILIES, ids=FID)
def test_family_reaches_its_path(kind, seed):
    f = loss_family(kind, seed)
    r = f["r64"]
    nt = f["targets"].shape[0]
    cap = 3 * nt
    counts = [len(v) for v in r["valid"]]
    valid = [int(v.sum()) for v in r["valid"]]
    assert min(valid) > 0, "a head without matches"
    if kind != "outside":
        assert counts == valid
    if kind == "chunk_edges":
        assert cap in (255, 258, 513)
        # matches on both sides of every chunk boundary the case has
        for h in range(3):
            chunks = set((r["pairs"][h] // 256).tolist())
            assert chunks == set(range((cap + 255) // 256)), (h, chunks)
    if kind in ("crowded", "dup_chain", "huge", "saturated", "outside"):
        assert cap > 256 and max(valid) > 256
    if kind == "crowded":
        assert nt == 200 and min(valid) > 256                      # every head loops over its matches more than once
    if kind == "huge":
        assert max(valid) > 4096 and min(valid) <= 4096            # the scan with and without the LDS keys
    if kind == "dup_chain":
        for h in range(3):
            spread = [sorted(set(q // 256 for q in pos)) for pos in _chains(f, h).values() if len(pos) >= 3]
            assert sum(len(s) >= 3 for s in spread) >= 2, (h, "chains of >= 3 matches in >= 3 different chunks")
            assert any(len(pos) >= 4 and len(set(q // 256 for q in pos)) >= 4 for pos in _chains(f, h).values()), h
        # centres exactly on cell borders: x * nx is an integer for the grid it was placed on
        t = f["targets"][100:112]
        assert sum(float(x * 20) == round(float(x * 20)) for x in t[:, 2]) >= 8
    if kind == "saturated":
        wh = torch.cat([pi[tuple(x[ok] for x in idx)][:, 2:4] for pi, idx, ok in zip(
            f["p"], [r["matches"][2][h] for h in range(3)], r["valid"])])
        if not f["v4"]:
            assert int((wh.exp() >= 1e3).any(1).sum()) >= 20          # the v3 clamp, gradient forced to 0
            assert int((wh.exp() < 1e3).all(1).sum()) >= 20
        obj = torch.cat([pi[..., 4:].flatten() for pi in f["p"]])
        assert float((obj > 50).float().mean()) > 0.08 and float((obj < -50).float().mean()) > 0.08
    if kind == "disjoint":
        assert "ciou" not in f["hyp"]
        n = sum(int(((i == 0) & (u < 0)).sum()) for i, u in zip(r["inter"], r["iou"]))
        assert n >= 20, n
        assert sum(int((i > 0).sum()) for i in r["inter"]) >= 20      # and the overlapping branch next to it
    if kind == "outside":
        assert all(c > v for c, v in zip(counts, valid))


def test_shared_cells_carry_several_box_gradients():
    """what the kernel adds up with atomicAdd: cells with 2 (crowded) or 3 and more matches, on every head"""
    for kind, seed in FAMILIES:
        if kind in ("crowded", "dup_chain", "huge"):
            f = loss_family(kind, seed)
            for h in range(3):
                sizes = [len(v) for v in _chains(f, h).values()]
                assert max(sizes) >= (2 if kind == "crowded" else 3), (kind, seed, h)


# ------------------------------------------------------------------ the bound is not vacuous
CAUGHT = {   # mistake -> (family, an entry of loss_errors on which it must exceed the GPU bound)
    "first_match_wins": (("dup_chain", 0), "head0.tobj"),
    "n_all_matches": (("outside", 4), "head0.box"),
    "pos_weight_factor": (("crowded", 1), "head1.obj"),
    "alpha_not_detached": (("crowded", 10), "head2.box"),
    "tobj_no_clamp": (("disjoint", 1), "head1.tobj"),
    "v3_clamp_keeps_gradient": (("saturated", 1), "head0.box"),
    "cls_mean_over_n": (("crowded", 1), "head2.cls"),
    "obj_mean_other_head": (("crowded", 2), "head0.obj"),
}


def test_every_mistake_is_listed():
    assert set(CAUGHT) == set(oloss.MISTAKES) and all(fam in FAMILIES for fam, _ in CAUGHT.values())


@pytest.mark.parametrize("mistake", oloss.MISTAKES)
def test_bound_catches_the_mistake(mistake):
    """the mistaken evaluation is fp32 like the kernel; the bound is the one of tests/test_gpu_loss_elements.py: LOSS_K times the
    error of the correct fp32 evaluation, at least LOSS_FLOOR.  The correct one passes it by construction (ratio 1 / LOSS_K)."""
    (kind, seed), key = CAUGHT[mistake]
    f = loss_family(kind, seed)
    bound = oloss.loss_bound(oloss.loss_errors(f["r32"], f["r64"]))
    bad = oloss.loss_reference(f["p"], f["targets"], f["anchor_vecs"], f["hyp"], f["nc"], f["gr"], f["v4"], dtype=torch.float32,
                               mistake=mistake)
    err = oloss.loss_errors(bad, f["r64"])
    over = {k: "%.1e > %.1e" % (err[k][0], bound[k][0]) for k in err if err[k][0] > bound[k][0] or err[k][1] > bound[k][1]}
    print(mistake, "on %s-%d:" % (kind, seed), over)
    assert err[key][0] > bound[key][0] and err[key][1] > bound[key][1], (key, err[key], bound[key])
    assert oloss.LOSS_K == 8 and oloss.LOSS_FLOOR == 4 * 2.0 ** -23


def test_group_errors_treats_all_zero_groups_exactly():
    z = torch.zeros(4)
    assert oloss.group_errors(z, z) == (0.0, 0.0)
    assert oloss.group_errors(torch.tensor([0.0, 1e-30, 0.0, 0.0]), z) == (float("inf"), float("inf"))
    e = oloss.group_errors(torch.tensor([1.0, 2.0 + 2e-6]), torch.tensor([1.0, 2.0], dtype=torch.float64))
    assert abs(e[0] - 1e-6) < 2e-7 and e[1] < e[0]

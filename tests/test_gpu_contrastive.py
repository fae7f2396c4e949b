"""GPU tests of the batch-hard contrastive loss (egonn_amd/csrc/loss.hip: contrastive_loss_kernel, contrastive_grad_kernel;
egonn_amd/loss.py) against the float64 restatement of tests/contrastive_ref.py, in the scheme of test_gpu_triplet.py, at the
sizes where the 256-strided loops wrap (n = 257, 1024) and below a wave (n = 5, d = 3).

Before the GPU is consulted each test checks in float64 (contrastive_ref.gaps) that no decision of the loss can be flipped by
fp32: the gap between the hardest and second-hardest positive (negative) of every row, |D[a][p] - pos_margin| and
|neg_margin - D[a][n]| of every triplet all exceed twice the floor 2 t distance, t = egonn_ref.triplet_tol(d).  On such inputs
the triplets, num_pairs and both above-threshold counts must EQUAL the restatement; loss, pos_loss, neg_loss, the statistics
and the gradient must lie within contrastive_ref.bounds (derivation: DESIGN.md §5; never looser than rtol 1e-3 / atol 1e-6).
The acceptance rule is contrastive_ref.accept, which test_contrastive_host.py shows to reject planted errors."""
import numpy as np
import pytest
import torch

from tests import contrastive_ref as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def loss_fn():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    g.build()
    from egonn_amd.loss import BatchHardContrastiveLossWithMasks
    return BatchHardContrastiveLossWithMasks(C.POS_MARGIN, C.NEG_MARGIN)


def _run(loss_fn, e, pm, nm, scale=1.0):
    et = torch.from_numpy(e).cuda().requires_grad_(True)
    loss, stats, (a, p, q) = loss_fn(et, torch.from_numpy(pm), torch.from_numpy(nm))
    (loss * scale).backward()
    return float(loss.detach()), stats, tuple(t.cpu().numpy() for t in (a, p, q)), et.grad.cpu().numpy()


def _check(loss_fn, case, n, d, scale=1.0, allow_ties=False):
    (e, pm, nm), (wl, ws, wt, wg, tol) = C.reference(case, n, d)
    g = C.gaps(e, pm, nm, allow_ties=allow_ties)
    print(g)
    assert min(g["pos"], g["neg"], g["pos_kink"], g["neg_kink"]) > 2.0, g
    got = _run(loss_fn, e, pm, nm, scale)
    assert got[1]["loss"] == got[0]
    C.accept(got, (wl, ws, wt, wg), tol, scale)
    return g, got, ws


def test_stats_keys_are_the_references(loss_fn):
    """models/loss.py:190-202"""
    e, pm, nm = C.HAND_E, C.HAND_POS, C.HAND_NEG
    loss, stats, trip, grad = _run(loss_fn, e, pm, nm)
    assert set(stats) == C.STATS_KEYS and stats["num_pairs"] == 6
    assert isinstance(stats["num_pairs"], int) and isinstance(stats["pos_pairs_above_threshold"], int)
    C.accept((loss, stats, trip, grad), C.loss64(e, pm, nm), C.bounds(e, pm, nm)[4])
    assert abs(loss - 0.55) < 1e-6 and np.allclose(grad, [[-1, 0], [0, 0], [1, 0], [0, 0]], atol=1e-6)   # the hand-worked case


@pytest.mark.parametrize("n,d", C.SIZES)
def test_both_hinges_active(loss_fn, n, d):
    """anchor 0 has no positive, the last anchor no negative (mean and max of the hardest-negative distances are +inf, as
    the reference averages them over ALL rows); backward scales by the incoming gradient"""
    g, got, ws = _check(loss_fn, "both_active", n, d, scale=2.5)
    assert g["pos_active"] + g["neg_active"] > 0 and ws["num_pairs"] == 2 * g["triplets"]
    if n >= 64:
        assert ws["num_pairs"] == 2 * (n - 2) and ws["mean_neg_pair_dist"] == np.inf and ws["max_neg_pair_dist"] == np.inf
        if d == 256:
            assert 0.1 <= g["pos_active"] <= 0.9 and 0.1 <= g["neg_active"] <= 0.9, g
            assert 0 < ws["pos_pairs_above_threshold"] < n - 2 and 0 < ws["neg_pairs_above_threshold"] < n - 2


@pytest.mark.parametrize("n,d", C.SIZES)
def test_no_hinge_active(loss_fn, n, d):
    g, got, ws = _check(loss_fn, "none_active", n, d)
    assert g["pos_active"] == 0.0 and g["neg_active"] == 0.0 and g["triplets"] == n
    assert got[0] == 0.0 and got[1]["pos_pairs_above_threshold"] == 0 and got[1]["neg_pairs_above_threshold"] == 0
    assert got[1]["pos_loss"] == 0.0 and got[1]["neg_loss"] == 0.0 and (got[3] == 0.0).all()         # exactly zero, not small


@pytest.mark.parametrize("n,d", C.SIZES)
def test_only_positive_hinges_active(loss_fn, n, d):
    g, got, ws = _check(loss_fn, "only_positives", n, d)
    assert g["pos_active"] > 0.5 and g["neg_active"] == 0.0
    assert got[1]["neg_loss"] == 0.0 and got[1]["neg_pairs_above_threshold"] == 0 and got[0] == got[1]["pos_loss"] > 0


@pytest.mark.parametrize("n,d", C.SIZES)
def test_exact_ties_and_zero_distances_on_integer_embeddings(loss_fn, n, d):
    """equidistant positives / negatives resolve to the first index; class 0 has every positive at distance 0 (hinge
    inactive, index 0 of the row); a negative at distance 0 is an active hinge that is counted and adds no gradient"""
    g, got, ws = _check(loss_fn, "integer_ties", n, d, allow_ties=True)
    a, p, _ = got[2]
    assert (p[np.isin(a, [0, 1, 2])] == 0).all() and ws["min_pos_pair_dist"] == 0.0
    assert np.isfinite(got[3]).all()


def test_anchors_without_positives_or_negatives(loss_fn):
    """anchors without positives, without negatives, without both; all-false masks; n = 1; a mask that names the anchor itself
    (distance 0 to its own negative: the d > 0 guard of the negative term)"""
    (e, pm, nm), _ = C.reference("both_active", 257, 256)
    pm, nm = pm.copy(), nm.copy()
    pm[[3, 40, 256]] = False
    nm[[5, 40, 255]] = False
    want = C.bounds(e, pm, nm)
    g = C.gaps(e, pm, nm)
    assert min(g["pos"], g["neg"], g["pos_kink"], g["neg_kink"]) > 2.0, g
    got = _run(loss_fn, e, pm, nm)
    C.accept(got, want[:4], want[4])
    assert want[1]["num_pairs"] == 2 * len(want[2][0]) < 2 * (257 - 2)
    none = np.zeros_like(pm)
    for masks in ((none, nm), (pm, none), (none, none)):
        got = _run(loss_fn, e, *masks)
        w = C.bounds(e, *masks)
        C.accept(got, w[:4], w[4])
        assert got[0] == 0.0 and got[1]["num_pairs"] == 0 and len(got[2][0]) == 0 and (got[3] == 0).all()
    assert got[1]["min_neg_pair_dist"] == np.inf and got[1]["max_pos_pair_dist"] == 0.0
    one = e[:1]
    for v in (False, True):
        m1 = np.full((1, 1), v)
        got = _run(loss_fn, one, m1, m1)                   # n = 1; masks set: pos 0 - 0.2 inactive, neg 0.65 - 0 active, no gradient
        w = C.bounds(one, m1, m1)
        C.accept(got, w[:4], w[4])
        assert got[1]["num_pairs"] == 2 * int(v) and got[0] == (np.float32(C.NEG_MARGIN) if v else 0.0) and (got[3] == 0).all()


def test_wrapper_conversions_and_determinism(loss_fn):
    """a second call with other data sees nothing of the first; non-contiguous, float64 and CPU-mask inputs are converted; two
    runs are bitwise equal (fixed-order reductions, no atomics on floats)"""
    (big, pmb, nmb), _ = C.reference("both_active", 257, 256)
    (small, pms, nms), _ = C.reference("both_active", 64, 3)
    first = _run(loss_fn, small, pms, nms)
    b1 = _run(loss_fn, big, pmb, nmb)
    again = _run(loss_fn, small, pms, nms)
    assert first[0] == again[0] and first[1] == again[1] and np.array_equal(first[3], again[3])
    b2 = _run(loss_fn, big, pmb, nmb)
    assert b1[0] == b2[0] and b1[1] == b2[1] and np.array_equal(b1[3], b2[3])
    et = torch.from_numpy(np.ascontiguousarray(big.T)).cuda().t().requires_grad_(True)
    assert not et.is_contiguous()
    loss, stats, _ = loss_fn(et, torch.from_numpy(pmb).cuda(), torch.from_numpy(nmb.astype(np.uint8)))
    loss.backward()
    assert float(loss.detach()) == b1[0] and stats == b1[1] and np.array_equal(et.grad.cpu().numpy(), b1[3])
    e64 = torch.from_numpy(big.astype(np.float64)).cuda().requires_grad_(True)
    loss, stats, _ = loss_fn(e64, torch.from_numpy(pmb), torch.from_numpy(nmb))
    (loss * 3.0).backward()
    assert e64.grad.dtype == torch.float64 and float(loss.detach()) == b1[0]
    assert np.array_equal(e64.grad.cpu().numpy(), (b1[3] * np.float32(3.0)).astype(np.float64))


def test_train_step_with_the_contrastive_loss():
    """one TrainStep(..., loss_fn=BatchHardContrastiveLossWithMasks(0.2, 0.65)) step on the three-scan batch of the train tests:
    finite gradients for every parameter, bitwise repeatable; the default TrainStep still carries the triplet loss"""
    import __graft_entry__ as ge
    ge.build()
    from egonn_amd import _lib
    from egonn_amd.loss import BatchHardContrastiveLossWithMasks, BatchHardTripletLossWithMasks
    from egonn_amd.train import TrainStep
    from tests import helpers as H
    from tests.test_gpu_train import _make_model, _scan_batch, _masks
    dev = _lib.require_gpu()
    case = H.load_case("egonn_train_cart03")
    coords = torch.from_numpy(case["coords"])
    pos, neg = _masks()
    runs = []
    for _ in range(2):
        model = _make_model(dev, int(case["weight_seed"]))
        step = TrainStep(model, torch.optim.SGD(model.parameters(), lr=0.0), loss_fn=BatchHardContrastiveLossWithMasks(0.2, 0.65))
        loss, stats = step(_scan_batch(dev, coords, [0, 1, 2]), pos, neg, step_optimizer=False)
        runs.append((float(loss), stats, {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}))
    assert set(runs[0][1]) == C.STATS_KEYS and runs[0][1]["num_pairs"] == 4 and np.isfinite(runs[0][0]) and runs[0][0] > 0
    global_params = {k for k, _ in model.named_parameters() if not k.startswith("local")}
    assert set(runs[0][2]) == global_params and len(global_params) > 50
    assert all(bool(torch.isfinite(g).all()) for g in runs[0][2].values())
    assert sum(float(g.abs().max()) > 0 for g in runs[0][2].values()) > 50
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    for k, g in runs[0][2].items():
        assert torch.equal(g, runs[1][2][k]), k
    assert isinstance(TrainStep(model, None).loss_fn, BatchHardTripletLossWithMasks)

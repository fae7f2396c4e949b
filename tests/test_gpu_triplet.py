"""GPU tests of the batch-hard triplet loss (egonn_amd/csrc/loss.hip, egonn_amd/loss.py) against the float64 reference
(oracle/egonn_ref.batch_hard_triplet_loss; gradient: float64 torch autograd of the same formula) at sizes where the
256-strided loops of mine_kernel / triplet_loss_kernel wrap (n > 256) and on data that reaches every branch: active and
inactive triplets together, the swap taken and not taken, no active triplet at all, anchors without positives /
negatives, exact ties and zero distances.

Before the GPU is consulted each test checks in float64 (egonn_ref.triplet_gaps) that no decision of the loss can be
flipped by fp32: the gap between the hardest and second-hardest positive (negative) of every row, |d_ap - d_an + margin|
of every triplet and |D[a][n] - D[p][n]| all exceed twice the floor  2 * triplet_tol(d) * distance,  triplet_tol(d) =
(d/2 + 2) * 2^-24 (one rounding per difference, a serial chain of d fmaf, sqrtf).  On such inputs triplet indices,
num_triplets and num_non_zero must EQUAL the reference.  Tolerances of the real-valued outputs: egonn_ref.triplet_bounds
(derived from triplet_tol and the fixed summation orders; the gradient bound is elementwise (t + (T + 4) u) * sum|terms|,
capped by the older rtol=1e-3 / atol=1e-6)."""
import numpy as np
import pytest
import torch

from tests import ends_data as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def loss_fn():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    g.build()
    from egonn_amd.loss import BatchHardTripletLossWithMasks
    return BatchHardTripletLossWithMasks(E.MARGIN)


def _run(loss_fn, e, pm, nm, scale=1.0):
    et = torch.from_numpy(e).cuda().requires_grad_(True)
    loss, stats, (a, p, q) = loss_fn(et, torch.from_numpy(pm), torch.from_numpy(nm))
    (loss * scale).backward()
    return float(loss.detach()), stats, tuple(t.cpu().numpy() for t in (a, p, q)), et.grad.cpu().numpy()


def _compare(got, e, pm, nm, scale=1.0):
    """E.triplet_accept (the rule the host suite shows to reject planted errors) against the float64 reference, whose
    gradient is first confirmed by float64 torch autograd of the same formula"""
    from oracle import egonn_ref as ref
    wl, ws, wt, wg, tol = ref.triplet_bounds(e, pm, nm, E.MARGIN)
    a_loss, a_grad = E.triplet_autograd64(e, *wt, E.MARGIN)
    assert abs(a_loss - wl) < 1e-12 and np.abs(a_grad - wg).max(initial=0.0) < 1e-12
    assert got[1]["loss"] == got[0]
    E.triplet_accept(got, (wl, ws, wt, a_grad), tol, scale)
    return ws


@pytest.mark.parametrize("n,d", [(255, 256), (256, 256), (257, 256), (300, 256), (512, 256), (1024, 256),
                                 (40, 1), (40, 33), (40, 1000), (40, 4096)])
def test_clustered_active_and_inactive_triplets(loss_fn, n, d):
    """class centres plus noise of per-class scale: at d = 256 the active and the inactive triplets, and the swapped and
    unswapped ones, are each at least a tenth; anchor 0 has no positive, the last anchor no negative (so the mean and max
    of the hardest-negative distances are +inf, as the reference averages them over ALL rows)"""
    from oracle import egonn_ref as ref
    e, pm, nm = E.triplet_clustered(n, d)
    g = ref.triplet_gaps(e, pm, nm, E.MARGIN)
    assert min(g["pos"], g["neg"], g["kink"], g["swap"]) > 2.0, g
    if d == 256:
        assert 0.1 <= g["active"] <= 0.9 and 0.1 <= g["swapped"] <= 0.9, g
    ws = _compare(_run(loss_fn, e, pm, nm, scale=2.5), e, pm, nm, scale=2.5)     # backward scales by the incoming gradient
    assert ws["num_triplets"] == n - 2 and ws["mean_neg_pair_dist"] == np.inf and ws["max_neg_pair_dist"] == np.inf
    if d == 256:
        assert 0 < ws["num_non_zero_triplets"] < ws["num_triplets"]              # AvgNonZero divides by fewer than all


@pytest.mark.parametrize("n,d", [(300, 256), (9, 5)])
def test_no_active_triplet(loss_fn, n, d):
    from oracle import egonn_ref as ref
    e, pm, nm = E.triplet_inactive(n, d)
    g = ref.triplet_gaps(e, pm, nm, E.MARGIN)
    assert min(g["pos"], g["neg"], g["kink"], g["swap"]) > 2.0 and g["active"] == 0.0 and g["triplets"] == n, g
    got = _run(loss_fn, e, pm, nm)
    _compare(got, e, pm, nm)
    assert got[0] == 0.0 and got[1]["num_non_zero_triplets"] == 0 and got[1]["num_triplets"] == n
    assert (got[3] == 0.0).all()                                                 # exactly zero, not small


def test_masks_without_positives_or_negatives(loss_fn):
    """anchors without positives, without negatives, without both; all-false masks; n = 1 and n = 2; masks that name the
    anchor itself (distance 0 to its own negative: the d > 0 guard of the negative term)"""
    from oracle import egonn_ref as ref
    e, pm, nm = E.triplet_clustered(300, 256)
    pm, nm = pm.copy(), nm.copy()
    pm[[3, 40, 299]] = False
    nm[[5, 40, 298]] = False
    ws = _compare(_run(loss_fn, e, pm, nm), e, pm, nm)
    assert ws["num_triplets"] == 300 - 6 and ws["min_pos_pair_dist"] == 0.0
    none = np.zeros_like(pm)
    for masks in ((none, nm), (pm, none), (none, none)):
        got = _run(loss_fn, e, *masks)
        _compare(got, e, *masks)
        assert got[0] == 0.0 and got[1]["num_triplets"] == 0 and len(got[2][0]) == 0 and (got[3] == 0).all()
    assert got[1]["min_neg_pair_dist"] == np.inf and got[1]["max_pos_pair_dist"] == 0.0
    one = e[:1]
    for v in (False, True):
        m1 = np.full((1, 1), v)
        got = _run(loss_fn, one, m1, m1)                                          # n = 1; with the masks set: l = 0 - 0 + margin
        _compare(got, one, m1, m1)
        assert got[1]["num_triplets"] == int(v) and got[0] == (np.float32(E.MARGIN) if v else 0.0) and (got[3] == 0).all()
    two = e[[1, 2]]
    pm2, nm2 = ~np.eye(2, dtype=bool), np.eye(2, dtype=bool)                      # n = 2: the other row is the positive,
    got = _run(loss_fn, two, pm2, nm2)                                            # the anchor its own negative
    ws = _compare(got, two, pm2, nm2)
    assert ws["num_triplets"] == 2 and ws["num_non_zero_triplets"] == 2 and np.abs(got[3]).max() > 0
    assert ref.triplet_gaps(two, pm2, nm2, E.MARGIN)["kink"] > 2.0


@pytest.mark.parametrize("n,d,flag", [(300, 8, True), (300, 8, False), (520, 16, True), (40, 3, False), (257, 1, True)])
def test_exact_ties_on_integer_embeddings(loss_fn, n, d, flag):
    """integer embeddings with duplicated rows (all distances exact): equidistant positives / negatives resolve to the
    first index for the max and the min alike; where every positive is at distance 0 the masked-out zeros tie with it and
    the index is 0 of the row, as the reference's argmax; zero distances inside active triplets leave the gradient finite
    and contribute nothing; D[p][n] == D[a][n] keeps the anchor's distance (egonn_ref.triplet_grad conventions)"""
    from oracle import egonn_ref as ref
    e, pm, nm = E.triplet_integer(n, d, row0_in_class0=flag)
    g = ref.triplet_gaps(e, pm, nm, E.MARGIN, allow_ties=True)
    assert min(g["pos"], g["neg"], g["kink"], g["swap"]) > 2.0, g                # what is not an exact tie is far from one
    got = _run(loss_fn, e, pm, nm)
    _compare(got, e, pm, nm)
    a, p, _ = got[2]
    assert (p[np.isin(a, [1, 2, 3])] == 0).all()


def test_wrapper_conversions_scratch_and_determinism(loss_fn):
    """a second call with other data sees nothing of the first; non-contiguous, float64 and CPU-mask inputs are converted;
    two runs are bitwise equal (fixed-order reductions, no atomics on floats)"""
    big, pmb, nmb = E.triplet_clustered(512, 256)
    small, pms, nms = E.triplet_clustered(40, 33)
    first = _run(loss_fn, small, pms, nms)
    _run(loss_fn, big, pmb, nmb)
    again = _run(loss_fn, small, pms, nms)                                       # after a larger problem used the allocator
    assert first[0] == again[0] and first[1] == again[1] and np.array_equal(first[3], again[3])
    assert all(np.array_equal(x, y) for x, y in zip(first[2], again[2]))
    b1, b2 = _run(loss_fn, big, pmb, nmb), _run(loss_fn, big, pmb, nmb)
    assert b1[0] == b2[0] and b1[1] == b2[1] and np.array_equal(b1[3], b2[3])
    # non-contiguous fp32 view, float64 embeddings, uint8 / CUDA masks
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

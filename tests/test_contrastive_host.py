"""Host-side tests of the batch-hard contrastive loss (no GPU): the float64 restatement (tests/contrastive_ref.py) against
values worked out by hand and against float64 autograd, and the acceptance rule of the GPU test (contrastive_ref.accept with
contrastive_ref.bounds), which must accept the float64 answer and a numpy fp32 restatement of the kernels' arithmetic on the
inputs the GPU test uses, and reject planted errors.  Also the Python surface that needs no device."""
import numpy as np
import pytest

from tests import contrastive_ref as C

HOST_SIZES = [(5, 3), (5, 256), (64, 3), (64, 256), (257, 3), (257, 256)]     # fp32 restatement: 1024 rows add nothing on the host


def test_hand_worked_four_embeddings():
    """points 0, 0.5, 0.1, 2.0 on a line, margins 0.2 / 0.65.  Anchor 0: positives {1, 2} -> p = 1 (0.5), negative 3 (2.0): positive
    hinge 0.3, negative hinge inactive.  Anchor 1: p = 0 (0.5), negatives {2, 3} -> n = 2 (0.4): hinges 0.3 and 0.25.  Anchor 2:
    p = 0 (0.1): positive hinge inactive; negatives {1, 3} -> n = 1 (0.4): 0.25.  Anchor 3 has no negative: dropped.
    pos_loss = (0.3 + 0.3) / 2, neg_loss = (0.25 + 0.25) / 2; d loss / d x = (-1, 0, +1, 0): the two positive pairs pull 0 and 1
    together with weight 1/2 each way, the two negative pairs push 1 and 2 apart."""
    loss, st, (a, p, q), g = C.loss64(C.HAND_E, C.HAND_POS, C.HAND_NEG)
    assert a.tolist() == [0, 1, 2] and p.tolist() == [1, 0, 0] and q.tolist() == [3, 2, 1]
    assert set(st) == C.STATS_KEYS
    assert st["num_pairs"] == 6 and st["pos_pairs_above_threshold"] == 2 and st["neg_pairs_above_threshold"] == 2
    for k, v in (("pos_loss", 0.3), ("neg_loss", 0.25), ("loss", 0.55), ("avg_embedding_norm", 0.65), ("mean_pos_pair_dist", 0.65),
                 ("max_pos_pair_dist", 1.5), ("min_pos_pair_dist", 0.1), ("min_neg_pair_dist", 0.4)):
        assert abs(st[k] - v) < 1e-7, (k, st[k])                      # 0.1 and 0.5 - 0.1 are fp32 values read in float64
    assert abs(loss - 0.55) < 1e-7 and st["mean_neg_pair_dist"] == np.inf and st["max_neg_pair_dist"] == np.inf
    assert np.allclose(g, [[-1, 0], [0, 0], [1, 0], [0, 0]], atol=1e-7)
    l32, s32, t32, g32 = C.loss32(C.HAND_E, C.HAND_POS, C.HAND_NEG)
    assert abs(l32 - 0.55) < 1e-6 and [v.tolist() for v in t32] == [[0, 1, 2], [1, 0, 0], [3, 2, 1]]


@pytest.mark.parametrize("case,n,d", [("both_active", 64, 256), ("both_active", 257, 3), ("only_positives", 64, 3),
                                      ("integer_ties", 64, 3)])
def test_restatement_gradient_is_the_autograd_gradient(case, n, d):
    (e, pm, nm), (wl, ws, wt, wg, tol) = C.reference(case, n, d)
    a_loss, a_grad = C.autograd64(e, *wt)
    assert abs(a_loss - wl) < 1e-12 and np.abs(a_grad - wg).max(initial=0.0) < 1e-12


@pytest.mark.parametrize("n,d", HOST_SIZES)
@pytest.mark.parametrize("case", ["both_active", "none_active", "only_positives"])
def test_checker_accepts_float64_and_fp32_restatement(case, n, d):
    (e, pm, nm), (wl, ws, wt, wg, tol) = C.reference(case, n, d)
    g = C.gaps(e, pm, nm)
    assert min(g["pos"], g["neg"], g["pos_kink"], g["neg_kink"]) > 2.0, g
    if case == "both_active":
        assert g["pos_active"] + g["neg_active"] > 0, g
        if n >= 64 and d == 256:          # a share of each hinge active and a share inactive
            assert 0.1 <= g["pos_active"] <= 0.9 and 0.1 <= g["neg_active"] <= 0.9, g
    if case == "none_active":
        assert g["pos_active"] == 0.0 and g["neg_active"] == 0.0 and wl == 0.0 and not wg.any()
    if case == "only_positives":
        assert g["pos_active"] > 0.5 and g["neg_active"] == 0.0 and ws["neg_loss"] == 0.0 and wl > 0
    assert tol["loss"] <= 1e-6 + 1e-3 * wl and (tol["grad"] <= 1e-6 + 1e-3 * np.abs(wg)).all()      # never looser than the older cap
    C.accept((wl, ws, wt, wg), (wl, ws, wt, wg), tol)
    C.accept(C.loss32(e, pm, nm), (wl, ws, wt, wg), tol)


@pytest.mark.parametrize("n,d", C.SIZES)
def test_gpu_inputs_have_the_properties_the_gpu_tests_state(n, d):
    """what test_gpu_contrastive.py asserts of its inputs alone, at every size it runs, the 1024 rows included: only anchor 0
    (no positive) and the last (no negative) are dropped from both_active, none from the other two cases"""
    for case, dropped in (("both_active", 2 if n >= 3 else 0), ("none_active", 0), ("only_positives", 0)):
        e, pm, nm = getattr(C, case)(n, d)
        keep = pm.any(1) & nm.any(1)
        assert int(keep.sum()) == n - dropped, (case, np.flatnonzero(~keep))
        if dropped:
            assert not keep[0] and not keep[n - 1] and not pm[0].any() and not nm[n - 1].any()
    (e, pm, nm), (wl, ws, wt, wg, tol) = C.reference("both_active", n, d)
    g = C.gaps(e, pm, nm)
    assert min(g["pos"], g["neg"], g["pos_kink"], g["neg_kink"]) > 2.0, g
    assert ws["num_pairs"] == 2 * (n - 2) and ws["mean_neg_pair_dist"] == np.inf and ws["max_neg_pair_dist"] == np.inf
    if n >= 64 and d == 256:
        assert 0.1 <= g["pos_active"] <= 0.9 and 0.1 <= g["neg_active"] <= 0.9, g
        assert 0 < ws["pos_pairs_above_threshold"] < n - 2 and 0 < ws["neg_pairs_above_threshold"] < n - 2


@pytest.mark.parametrize("n,d", [(5, 3), (64, 3), (257, 3), (64, 256)])
def test_checker_accepts_fp32_on_integer_ties(n, d):
    (e, pm, nm), (wl, ws, wt, wg, tol) = C.reference("integer_ties", n, d)
    g = C.gaps(e, pm, nm, allow_ties=True)
    assert min(g["pos"], g["neg"], g["pos_kink"], g["neg_kink"]) > 2.0, g
    a, p, q = wt
    D = np.linalg.norm(e[a].astype(np.float64) - e[p], axis=1), np.linalg.norm(e[a].astype(np.float64) - e[q], axis=1)
    assert (D[0] == 0).any() and ((D[1] == 0).any() or n == 5)        # zero positive and zero negative distances are present
    C.accept(C.loss32(e, pm, nm), (wl, ws, wt, wg), tol)


def test_checker_rejects_planted_errors():
    (e, pm, nm), (wl, ws, wt, wg, tol) = C.reference("both_active", 64, 256)
    want = (wl, ws, wt, wg)
    good = C.loss32(e, pm, nm)
    C.accept(good, want, tol)
    a, p, q = wt
    # the second-hardest positive of one anchor
    D = np.linalg.norm(e[:, None, :].astype(np.float64) - e[None], axis=2)
    i = int(np.flatnonzero(pm[a].sum(1) >= 2)[0])
    second = int(np.argsort(-np.where(pm[a[i]], D[a[i]], -np.inf))[1])
    p2 = p.copy()
    p2[i] = second
    with pytest.raises(AssertionError):
        C.accept((good[0], good[1], (a, p2, q), good[3]), want, tol)
    # a count off by one, each of the three
    for k, dv in (("pos_pairs_above_threshold", 1), ("neg_pairs_above_threshold", -1), ("num_pairs", 2)):
        st = dict(good[1])
        st[k] += dv
        with pytest.raises(AssertionError):
            C.accept((good[0], st, good[2], good[3]), want, tol)
    # the loss, and each part, off by ten tolerances
    with pytest.raises(AssertionError):
        C.accept((good[0] + 10 * tol["loss"], good[1], good[2], good[3]), want, tol)
    for k in ("pos_loss", "neg_loss", "loss"):
        st = dict(good[1])
        st[k] -= 10 * tol[k]
        with pytest.raises(AssertionError):
            C.accept((good[0], st, good[2], good[3]), want, tol)
    # one gradient entry off by ten of its tolerances; a dropped stats key
    g2 = good[3].copy()
    r, c = np.unravel_index(np.argmax(tol["grad"]), g2.shape)
    g2[r, c] += 10 * tol["grad"][r, c]
    with pytest.raises(AssertionError):
        C.accept((good[0], good[1], good[2], g2), want, tol)
    st = dict(good[1])
    del st["neg_loss"]
    with pytest.raises(AssertionError):
        C.accept((good[0], st, good[2], good[3]), want, tol)


def test_python_surface_without_a_device():
    """make_losses keeps today's call and accepts the reference's loss names and margins (models/loss.py:12-21)"""
    import inspect
    from egonn_amd import loss as L
    from egonn_amd.train import TrainStep
    assert isinstance(L.make_losses(), L.BatchHardTripletLossWithMasks) and L.make_losses(0.4).margin == 0.4
    c = L.make_losses(loss="BatchHardContrastiveLoss")
    assert isinstance(c, L.BatchHardContrastiveLossWithMasks) and (c.pos_margin, c.neg_margin) == (0.2, 0.65)
    c = L.make_losses(loss="BatchHardContrastiveLoss", pos_margin=0.1, neg_margin=0.5)
    assert (c.pos_margin, c.neg_margin) == (0.1, 0.5)
    with pytest.raises(NotImplementedError):
        L.make_losses(loss="SomethingElse")
    sig = inspect.signature(TrainStep.__init__)
    assert list(sig.parameters)[1:] == ["model", "optimizer", "margin", "loss_fn"]
    assert sig.parameters["margin"].default == 0.2 and sig.parameters["loss_fn"].default is None
    sentinel = object()
    assert TrainStep(None, None, loss_fn=sentinel).loss_fn is sentinel
    assert isinstance(TrainStep(None, None).loss_fn, L.BatchHardTripletLossWithMasks)

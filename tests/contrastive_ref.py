"""float64 restatement of the batch-hard contrastive loss (egonn_amd/csrc/loss.hip: contrastive_loss_kernel /
contrastive_grad_kernel; reference models/loss.py:175-204) with its gradient, the error bounds allowed to the fp32 kernel,
the seeded inputs of the GPU tests (test_gpu_contrastive.py) and THE acceptance rule those tests use, which
test_contrastive_host.py shows on the CPU to accept a float32 restatement and to reject planted errors.

The loss class the reference calls, pytorch_metric_learning.losses.ContrastiveLoss, is absent from the image and restated
from its documentation [recall]: on the triplets (a, p, n) of the in-tree miner (models/loss.py:114-143) read as the pairs
(a, p) and (a, n), with D the plain Euclidean distance (LpDistance(p=2, power=1), not squared),
    pos_i = relu(D[a][p] - pos_margin)        neg_i = relu(neg_margin - D[a][n])
    loss  = mean of the pos_i > 0 (0 if none) + mean of the neg_i > 0 (0 if none)          (AvgNonZeroReducer per pair set)
There is no swap.  Gradient conventions: those of the triplet kernel (a zero distance contributes nothing)."""
import functools

import numpy as np

from oracle import egonn_ref as ref

POS_MARGIN, NEG_MARGIN = 0.2, 0.65          # the reference's defaults (misc/utils.py:158-160)
U32 = ref.U32
DIST_KEYS = ("mean_pos_pair_dist", "max_pos_pair_dist", "min_pos_pair_dist", "mean_neg_pair_dist", "max_neg_pair_dist",
             "min_neg_pair_dist")
STATS_KEYS = {"loss", "avg_embedding_norm", "pos_pairs_above_threshold", "neg_pairs_above_threshold", "pos_loss", "neg_loss",
              "num_pairs"} | set(DIST_KEYS)                                        # models/loss.py:190-202


def mine(D, pm, nm):
    """models/loss.py:114-143: positives masked to 0 then row max, negatives masked to +inf then row min (first index on
    ties), anchors kept if they have both.  -> (a, p, n), hardest positive / negative distance of every row"""
    mp, mn = np.where(pm, D, D.dtype.type(0)), np.where(nm, D, D.dtype.type(np.inf))
    keep = pm.any(1) & nm.any(1)
    a = np.arange(len(D))[keep]
    return (a, mp.argmax(1)[keep], mn.argmin(1)[keep]), mp.max(1), mn.min(1)


def _avg_non_zero(v, dtype=np.float64):
    nz = int((v > 0).sum())
    return (dtype(v[v > 0].sum(dtype=dtype)) / dtype(nz) if nz else dtype(0)), nz


def _stats(loss, pl, nl, cp, cn, n_trip, norms, hp, hn, dtype=np.float64):
    with np.errstate(invalid="ignore"):
        return {"loss": float(loss), "avg_embedding_norm": float(norms.mean(dtype=dtype)), "pos_pairs_above_threshold": cp,
                "neg_pairs_above_threshold": cn, "pos_loss": float(pl), "neg_loss": float(nl), "num_pairs": 2 * n_trip,
                "mean_pos_pair_dist": float(hp.mean(dtype=dtype)), "max_pos_pair_dist": float(hp.max()),
                "min_pos_pair_dist": float(hp.min()), "mean_neg_pair_dist": float(hn.mean(dtype=dtype)),
                "max_neg_pair_dist": float(hn.max()), "min_neg_pair_dist": float(hn.min())}


def grad(emb, D, a, p, q, pos_margin, neg_margin, dtype=np.float64):
    """dLoss/dE for given triplets in `dtype`: + d(a,p) / #pos for every pos_i > 0, - d(a,n) / #neg for every neg_i > 0; a zero
    distance contributes nothing.  Returns (grad, S, T): S[r][c] = sum of the |terms| landing on grad[r][c], T[r] their
    number (for the bound of the fp32 kernel, as egonn_ref.triplet_grad)."""
    e, D = np.asarray(emb, dtype), np.asarray(D, dtype)
    n, d = e.shape
    g, S, T = np.zeros((n, d), dtype), np.zeros((n, d), np.float64), np.zeros(n, np.int64)
    a, p, q = (np.asarray(v, np.int64) for v in (a, p, q))
    if len(a) == 0:
        return g, S, T
    pos = np.maximum(D[a, p] - dtype(pos_margin), dtype(0)) > 0
    neg = np.maximum(dtype(neg_margin) - D[a, q], dtype(0)) > 0
    for act, other, sign in ((pos, p, 1.0), (neg, q, -1.0)):
        if not act.any():
            continue
        w = dtype(1) / dtype(act.sum())
        x, y = a[act], other[act]
        dist = D[x, y]
        ok = dist > 0
        term = (dtype(sign) * w * (e[x] - e[y])[ok] / dist[ok][:, None]).astype(dtype)
        np.add.at(g, x[ok], term)
        np.add.at(g, y[ok], -term)
        for rows in (x[ok], y[ok]):
            np.add.at(S, rows, np.abs(term).astype(np.float64))
            np.add.at(T, rows, 1)
    return g, S, T


def loss64(emb, pos_mask, neg_mask, pos_margin=POS_MARGIN, neg_margin=NEG_MARGIN):
    """float64: (loss, stats with the reference's keys, (a, p, n), grad)"""
    e = np.asarray(emb, np.float64)
    pm, nm = np.asarray(pos_mask, bool), np.asarray(neg_mask, bool)
    D = ref.pdist64(e)
    (a, p, q), hp, hn = mine(D, pm, nm)
    pl, cp = _avg_non_zero(np.maximum(D[a, p] - pos_margin, 0.0))
    nl, cn = _avg_non_zero(np.maximum(neg_margin - D[a, q], 0.0))
    stats = _stats(pl + nl, pl, nl, cp, cn, len(a), np.linalg.norm(e, axis=1), hp, hn)
    return float(pl + nl), stats, (a, p, q), grad(e, D, a, p, q, pos_margin, neg_margin)[0]


def loss32(emb, pos_mask, neg_mask, pos_margin=POS_MARGIN, neg_margin=NEG_MARGIN):
    """numpy fp32 restatement of the kernels' arithmetic (D by a serial fmaf chain over the columns and sqrtf, as
    egonn_ref.triplet_fp32; hinges, means and gradient terms in float32; numpy's summation order, not the kernel's)"""
    f = np.float32
    e = np.asarray(emb, f)
    n, d = e.shape
    s = np.zeros((n, n), f)
    for c in range(d):
        df = e[:, None, c] - e[None, :, c]
        s = (df.astype(np.float64) * df.astype(np.float64) + s.astype(np.float64)).astype(f)      # fmaf
    D = np.sqrt(s)
    pm, nm = np.asarray(pos_mask, bool), np.asarray(neg_mask, bool)
    (a, p, q), hp, hn = mine(D, pm, nm)
    pl, cp = _avg_non_zero(np.maximum(D[a, p] - f(pos_margin), f(0)), f)
    nl, cn = _avg_non_zero(np.maximum(f(neg_margin) - D[a, q], f(0)), f)
    stats = _stats(f(pl + nl), pl, nl, cp, cn, len(a), np.sqrt((e * e).sum(1, dtype=f)), hp, hn, f)
    return float(f(pl + nl)), stats, (a, p, q), grad(e, D, a, p, q, pos_margin, neg_margin, dtype=f)[0]


def gaps(emb, pos_mask, neg_mask, pos_margin=POS_MARGIN, neg_margin=NEG_MARGIN, allow_ties=False):
    """How far the input is from every decision fp32 could flip, each as a multiple of its floor (> 1: fp32 cannot flip it),
    in float64 with t = egonn_ref.triplet_tol(d), over the kept anchors, in the convention of egonn_ref.triplet_gaps:
      pos / neg   hardest vs second-hardest positive / negative of a row:  gap / (2 t larger distance)
      pos_kink    |D[a][p] - pos_margin| / (2 t (D[a][p] + pos_margin))          (relu, the > 0 count, the gradient filter)
      neg_kink    |neg_margin - D[a][n]| / (2 t (D[a][n] + neg_margin))
    allow_ties: mining gaps that are exactly 0 are left out (there the first-index rule decides, not the arithmetic).
    Also the shares of active positive / negative hinges."""
    e = np.asarray(emb, np.float64)
    t = ref.triplet_tol(e.shape[1])
    D = ref.pdist64(e)
    pm, nm = np.asarray(pos_mask, bool), np.asarray(neg_mask, bool)
    keep = pm.any(1) & nm.any(1)
    out = {"pos": np.inf, "neg": np.inf, "pos_kink": np.inf, "neg_kink": np.inf, "pos_active": 0.0, "neg_active": 0.0,
           "triplets": int(keep.sum())}
    if not keep.any():
        return out

    def ratio(gap, floor):
        sel = gap > 0 if allow_ties else np.ones(gap.shape, bool)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = gap[sel] / floor[sel]
        return float(np.nan_to_num(r, nan=0.0).min(initial=np.inf))

    rows = keep & (pm.sum(1) >= 2)
    if rows.any():
        top = -np.sort(-np.where(pm, D, -np.inf)[rows], axis=1)[:, :2]
        out["pos"] = ratio(top[:, 0] - top[:, 1], 2 * t * top[:, 0])
    rows = keep & (nm.sum(1) >= 2)
    if rows.any():
        low = np.sort(np.where(nm, D, np.inf)[rows], axis=1)[:, :2]
        out["neg"] = ratio(low[:, 1] - low[:, 0], 2 * t * low[:, 1])
    (a, p, q), _, _ = mine(D, pm, nm)
    out["pos_kink"] = float((np.abs(D[a, p] - pos_margin) / (2 * t * (D[a, p] + pos_margin))).min())
    out["neg_kink"] = float((np.abs(neg_margin - D[a, q]) / (2 * t * (D[a, q] + neg_margin))).min())
    out["pos_active"] = float((D[a, p] > pos_margin).mean())
    out["neg_active"] = float((D[a, q] < neg_margin).mean())
    return out


def bounds(emb, pos_mask, neg_mask, pos_margin=POS_MARGIN, neg_margin=NEG_MARGIN):
    """loss64 plus the absolute error allowed to the fp32 kernel per quantity (derivation: DESIGN.md §5), with t =
    triplet_tol(d) the relative error of one D entry, u = 2^-24 and s = ceil(n / 256) + 9 roundings of a strided partial sum,
    the 8-level tree and one division:
      pos_loss   (t + 2u) max(D[a][p] + pos_margin) + s u pos_loss      a hinge: one D entry, the margin's rounding to fp32 and
      neg_loss   (t + 2u) max(D[a][n] + neg_margin) + s u neg_loss      the subtraction's; then the mean of the hinges
      loss       the two above + u loss                                  one addition
      mean_*_dist, avg_embedding_norm (t + s u) value;  max_* / min_* t value;  counts and indices 0
      grad[r][c] (t + (T[r] + 4) u) S[r][c], the triplet gradient's rule (egonn_ref.triplet_bounds)
    and none looser than the older cap 1e-6 + 1e-3 |value|.  Returns (loss, stats, (a, p, n), grad, tol)."""
    e = np.asarray(emb, np.float64)
    n, d = e.shape
    t = ref.triplet_tol(d)
    s = -(-n // 256) + 9
    loss, stats, (a, p, q), _ = loss64(e, pos_mask, neg_mask, pos_margin, neg_margin)
    D = ref.pdist64(e)
    g, S, T = grad(e, D, a, p, q, pos_margin, neg_margin)
    cap = lambda v: 1e-6 + 1e-3 * abs(v)
    tol = {}
    tp = (t + 2 * U32) * (D[a, p] + pos_margin).max(initial=0.0) + s * U32 * stats["pos_loss"]
    tn = (t + 2 * U32) * (D[a, q] + neg_margin).max(initial=0.0) + s * U32 * stats["neg_loss"]
    tol["pos_loss"], tol["neg_loss"] = min(tp, cap(stats["pos_loss"])), min(tn, cap(stats["neg_loss"]))
    tol["loss"] = min(tp + tn + U32 * loss, cap(loss))
    for k, v in stats.items():
        if k.startswith("mean_") or k == "avg_embedding_norm":
            tol[k] = (t + s * U32) * abs(v) if np.isfinite(v) else 0.0
        elif k.startswith(("max_", "min_")):
            tol[k] = t * abs(v) if np.isfinite(v) else 0.0
        elif k not in tol:
            tol[k] = 0.0
    tol["grad"] = np.minimum((t + (T[:, None] + 4) * U32) * S, 1e-6 + 1e-3 * np.abs(g))
    return loss, stats, (a, p, q), g, tol


def autograd64(e, a, p, q, pos_margin=POS_MARGIN, neg_margin=NEG_MARGIN):
    """float64 torch autograd of the loss formula for fixed pairs (zero distances contribute no gradient) -> (loss, grad)"""
    import torch
    x = torch.from_numpy(np.asarray(e, np.float64)).requires_grad_(True)
    a, p, q = (torch.from_numpy(np.asarray(v, np.int64)) for v in (a, p, q))
    if len(a) == 0:
        return 0.0, np.zeros(x.shape)

    def dist(i, j):
        d2 = ((x[i] - x[j]) ** 2).sum(1)
        return torch.where(d2 > 0, torch.sqrt(torch.where(d2 > 0, d2, torch.ones_like(d2))), torch.zeros_like(d2))

    lp, ln = torch.relu(dist(a, p) - pos_margin), torch.relu(neg_margin - dist(a, q))
    loss = sum((l[l > 0].mean() if (l > 0).any() else l.sum() * 0) for l in (lp, ln))
    loss.backward()
    return float(loss.detach()), x.grad.numpy()


def accept(got, want, tol, scale=1.0):
    """THE acceptance rule of the contrastive tests, host and GPU alike: got = (loss, stats, (a, p, n), grad) of the code under
    test, want the same in float64, tol from bounds().  Triplets, num_pairs and both above-threshold counts EQUAL; loss, its
    two parts, the statistics and the gradient (divided by `scale`, the incoming gradient of backward) within their bounds;
    non-finite statistics equal.  Every figure is printed before it is asserted."""
    loss, stats, trip, g = got
    wl, ws, wt, wg = want
    assert set(stats) == STATS_KEYS, set(stats) ^ STATS_KEYS
    for x, y, name in zip(trip, wt, "apn"):
        assert np.array_equal(x, y), name
    for k in ("num_pairs", "pos_pairs_above_threshold", "neg_pairs_above_threshold"):
        print(f"{k} {stats[k]!r} want {ws[k]!r}")
        assert stats[k] == ws[k], (k, stats[k], ws[k])
    print(f"loss {loss!r} want {wl!r} allowed {tol['loss']:.3g}")
    assert abs(loss - wl) <= tol["loss"], (loss, wl, tol["loss"])
    for k, v in ws.items():
        print(f"{k} {stats[k]!r} want {v!r} allowed {tol[k]:.3g}")
        assert (stats[k] == v) if not np.isfinite(v) else (abs(stats[k] - v) <= tol[k]), (k, stats[k], v, tol[k])
    err = np.abs(np.asarray(g, np.float64) / scale - wg)
    print(f"grad max err {err.max(initial=0.0):.3g}, max allowed {tol['grad'].max(initial=0.0):.3g}")
    assert np.isfinite(g).all() and (err <= tol["grad"]).all()


# ------------------------------------------------------------------------------------------------ seeded inputs
def masks_from_labels(lab):
    lab = np.asarray(lab)
    pm = (lab[:, None] == lab[None, :]) & ~np.eye(len(lab), dtype=bool)
    return pm, lab[:, None] != lab[None, :]


def _settle(e, pm, nm, draw, rng):
    """draw single rows again until every decision is at least 2 floors (4 t, the factor 2 of gaps() included) from flipping"""
    e = e.astype(np.float32)
    n, d = e.shape
    t = ref.triplet_tol(d)
    for _ in range(200):
        # Gram form in float64: its error, 1e-16 |e|^2 on D^2, is far below the 1e-5 relative gaps looked for here (the tests
        # confirm the settled input with gaps(), on the exact difference form)
        x = e.astype(np.float64)
        sq = (x * x).sum(1)
        D = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2.0 * (x @ x.T), 0.0))
        keep = pm.any(1) & nm.any(1)
        bad = np.zeros(n, bool)
        if n >= 2:
            top = -np.sort(-np.where(pm, D, -np.inf), axis=1)[:, :2]
            low = np.sort(np.where(nm, D, np.inf), axis=1)[:, :2]
            with np.errstate(invalid="ignore"):
                tie_p = keep & (pm.sum(1) >= 2) & (top[:, 0] - top[:, 1] <= 5 * t * top[:, 0])
                tie_n = keep & (nm.sum(1) >= 2) & (low[:, 1] - low[:, 0] <= 5 * t * low[:, 1])
            # a near tie is a property of the two tied rows as much as of the anchor: draw the hardest one again as well
            bad |= tie_p | tie_n
            bad[np.where(pm, D, 0.0).argmax(1)[tie_p]] = True
            bad[np.where(nm, D, np.inf).argmin(1)[tie_n]] = True
        (a, p, q), _, _ = mine(D, pm, nm)
        bad[a] |= np.abs(D[a, p] - POS_MARGIN) <= 5 * t * (D[a, p] + POS_MARGIN)
        bad[a] |= np.abs(NEG_MARGIN - D[a, q]) <= 5 * t * (D[a, q] + NEG_MARGIN)
        if not bad.any():
            return e
        for i in np.flatnonzero(bad):
            e[i] = draw(i, rng)
    raise AssertionError("the contrastive input did not settle")


def _classes(n, d, seed, cen_scale, sig_lo, sig_hi, drop=True, lattice=0.0):
    """class centres plus noise of per-class norm in sig_lo .. sig_hi.  Centres: Gaussian of norm ~ cen_scale, or (lattice > 0)
    the points of a cubic lattice of that spacing in the first three coordinates, jittered, so that classes stay apart in
    3-D as well.  Every class has at least two members, so every row has a positive.  drop: anchor 0 has no positive, the last anchor no negative (n >= 3)."""
    rng = np.random.default_rng(seed)
    ncls = max(2, n // 8)
    lab = np.arange(n) % ncls if n < 16 else rng.integers(0, ncls, n)
    # a class drawn with a single member would leave its anchor without a positive: that row joins the class of the next row
    # of a larger class (no random number is spent, so inputs without such a class are what they were)
    cnt = np.bincount(lab, minlength=ncls)
    for i in np.flatnonzero(cnt[lab] == 1):
        lab[i] = next(lab[j % n] for j in range(i + 1, i + n) if cnt[lab[j % n]] >= 2)
    cen = rng.standard_normal((ncls, d)) * (cen_scale / np.sqrt(d))
    if lattice:
        m = int(np.ceil(ncls ** (1.0 / 3.0)))
        k = np.arange(ncls)
        cen[:, :3] += lattice * np.stack([k % m, (k // m) % m, k // (m * m)], axis=1)[:, :min(3, d)]
    sig = rng.uniform(sig_lo, sig_hi, ncls) / np.sqrt(d)

    def draw(i, rng):
        return cen[lab[i]] + sig[lab[i]] * rng.standard_normal(d)

    e = np.stack([draw(i, rng) for i in range(n)])
    pm, nm = masks_from_labels(lab)
    if drop and n >= 3:
        pm[0] = False
        nm[n - 1] = False
    return _settle(e, pm, nm, draw, rng), pm, nm


SIZES = [(n, d) for n in (5, 64, 257, 1024) for d in (3, 256)]      # the 256-strided loops at their wrap; d below a wave


@functools.lru_cache(maxsize=None)
def both_active(n, d):
    """loose and tight classes around close centres: positive hinges (D[a][p] > 0.2) and negative hinges (D[a][n] < 0.65) are
    each active for a share of the anchors and inactive for another"""
    return _classes(n, d, 11000 + 7 * n + d, 0.45, 0.03, 0.35)


@functools.lru_cache(maxsize=None)
def none_active(n, d):
    """tight classes well apart: every D[a][p] < 0.2 and every D[a][n] > 0.65 -> loss 0, gradient 0"""
    return _classes(n, d, 12000 + 7 * n + d, 0.2, 0.02, 0.05, drop=False, lattice=2.0)


@functools.lru_cache(maxsize=None)
def only_positives(n, d):
    """loose classes far apart: positive hinges active, no negative hinge"""
    return _classes(n, d, 13000 + 7 * n + d, 0.2, 0.3, 0.6, drop=False, lattice=5.0)


@functools.lru_cache(maxsize=None)
def integer_ties(n, d):
    """small-integer embeddings drawn from a small pool of points whatever the class (the recipe of
    tests/ends_data.triplet_integer, for any n >= 5): every squared distance is an exact small integer, so exact ties between
    positives and between negatives are plentiful and resolve to the first index.  Class 0 is one point repeated: its
    positives are at distance 0 (hinge inactive, 0 - 0.2 < 0; the masked-out zeros tie with them, index 0 of the row); one
    row of another class repeats that point: a negative at distance 0 (hinge active and counted, no gradient).  Every
    distance is 0 or at least 1, far from both margins."""
    rng = np.random.default_rng(14000 + 7 * n + d)
    ncls = max(3, n // 10)
    lab = rng.integers(1, ncls, n)
    lab[:3] = 0
    twin = min(5, n - 1)
    lab[twin] = 2
    pts = rng.integers(-3, 4, (max(4, n // 3), d))
    e = pts[rng.integers(0, len(pts), n)].astype(np.float32)
    e[lab == 0] = pts[0]
    e[twin] = pts[0]
    pm, nm = masks_from_labels(lab)
    return e, pm, nm


@functools.lru_cache(maxsize=None)
def reference(case, n, d):
    """(inputs, bounds) of a named case, computed once per process and shared by the tests that need it"""
    e, pm, nm = globals()[case](n, d)
    return (e, pm, nm), bounds(e, pm, nm)


# the 4-embedding case worked out by hand (test_contrastive_host.py): points on a line, D = |x_i - x_j|
HAND_E = np.array([[0.0, 0.0], [0.5, 0.0], [0.1, 0.0], [2.0, 0.0]], np.float32)
HAND_POS = np.array([[0, 1, 1, 0], [1, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0]], bool)
HAND_NEG = np.array([[0, 0, 0, 1], [0, 0, 1, 1], [0, 1, 0, 1], [0, 0, 0, 0]], bool)

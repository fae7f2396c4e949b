"""Seeded inputs shared by the GPU tests of the two ends of the pipeline and of the global loss (test_gpu_retrieval.py,
test_gpu_triplet.py) and by the CPU tests of their checkers (test_ends_host.py): the checkers are shown on the CPU to
accept a float32 restatement of the kernels' arithmetic on exactly the inputs the GPU tests use."""
import numpy as np

from oracle import egonn_ref as ref
from oracle import retrieval_ref as R

MARGIN = 0.2


# ------------------------------------------------------------------------------------------------ kNN, real-valued
def knn_parity():
    """the recipe of test_gpu_parity.test_knn_and_recall_match_oracle: Gaussian database with exact duplicates"""
    rng = np.random.default_rng(7)
    m, nq, d, k = 5000, 300, 256, 25
    db = rng.standard_normal((m, d)).astype(np.float32)
    db[100] = db[7]
    db[4000] = db[7]
    qs = (db[rng.integers(0, m, nq)] + 0.05 * rng.standard_normal((nq, d))).astype(np.float32)
    qs[0] = db[7]
    return qs, db, k


def knn_unit():
    """unit-normalised 256-d descriptors, what the model emits; queries are noisy revisits of database rows"""
    rng = np.random.default_rng(17)
    db = rng.standard_normal((3001, 256))
    db /= np.linalg.norm(db, axis=1, keepdims=True)
    qs = db[rng.integers(0, len(db), 203)] + 0.02 * rng.standard_normal((203, 256))
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    db = db.astype(np.float32)
    db[2999] = db[3]                                                   # a duplicate in another wave's stride
    return qs.astype(np.float32), db, 25


def knn_clustered():
    """20 tight clusters, d = 100 (ragged lanes): within a cluster the distances to a query nearly coincide"""
    rng = np.random.default_rng(27)
    cen = rng.standard_normal((20, 100))
    db = (cen[rng.integers(0, 20, 2002)] + 1e-3 * rng.standard_normal((2002, 100))).astype(np.float32)
    qs = (cen[rng.integers(0, 20, 129)] + 1e-2 * rng.standard_normal((129, 100))).astype(np.float32)
    return qs, db, 150


def knn_ragged():
    """d = 37 < 64 with k = m: the whole database sorted"""
    rng = np.random.default_rng(37)
    db = rng.standard_normal((1000, 37)).astype(np.float32)
    qs = rng.standard_normal((9, 37)).astype(np.float32)
    return qs, db, 1000


KNN_REAL = {"parity": knn_parity, "unit": knn_unit, "clustered": knn_clustered, "ragged": knn_ragged}


# ------------------------------------------------------------------------------------------------ recall
RADII = (1e-3, 5.0, 20.0, 25.0, 1e7)          # nothing meets the first (the floor keeps every pair away), all meet the last
ROOM = 4.0                                    # inputs are built this many floors away from every decision


# (position_dim, queries, seed, map rows) of every recall input of the GPU tests; nq = 203 is the recall_at_k wrapper's
RECALL_SETS = [(pd, nq, 100 + 10 * pd + nq % 7, 700) for pd in (2, 3) for nq in (0, 1, 127, 128, 129, 1000)] + \
              [(2, 203, 302, 700), (3, 203, 303, 700)]


def recall_utm(seed, m, nq, pd, radius=RADII):
    """UTM-scale float64 positions (around 4e6 m) with metre-scale structure: a random-walk trajectory as the map,
    queries a few metres off map poses.  Queries closer than ROOM floors to any radius are drawn again, so that the
    float64 reference and an fp32 evaluation of the origin-shifted positions must give the same counts."""
    rng = np.random.default_rng(seed)
    base = np.array([4.05e6, 3.96e6, 120.0])[:pd]
    step = rng.normal(0, 1.5, (m, pd)) + np.array([2.0, 0.5, 0.0])[:pd]
    mpos = base + np.cumsum(step, axis=0)
    qpos = mpos[rng.integers(0, m, nq)] + rng.normal(0, 8.0, (nq, pd)) if nq else np.zeros((0, pd))
    if pd == 3:
        qpos[:, 2] = base[2] + rng.normal(0, 2.0, nq)
    for _ in range(50):
        bad = np.flatnonzero(R.recall_margin_rows(qpos, mpos, radius) <= ROOM)
        if not len(bad):
            break
        qpos[bad] = mpos[rng.integers(0, m, len(bad))] + rng.normal(0, 8.0, (len(bad), pd))
    return qpos, mpos


# ------------------------------------------------------------------------------------------------ triplet loss
def masks_from_labels(lab):
    lab = np.asarray(lab)
    pm = (lab[:, None] == lab[None, :]) & ~np.eye(len(lab), dtype=bool)
    return pm, lab[:, None] != lab[None, :]


def _settle(e, pm, nm, draw, rng, allow_ties=False):
    """Draw single rows again until every decision of the loss is at least 2 floors from flipping (triplet_gaps), so
    that triplet indices and counts are determined whatever the fp32 rounding.  Returns float32 embeddings."""
    e = e.astype(np.float32)
    n, d = e.shape
    t = ref.triplet_tol(d)
    for _ in range(200):
        D = ref.pdist64(e)
        keep = pm.any(1) & nm.any(1)
        bad = np.zeros(n, bool)
        P, N = np.where(pm, D, -np.inf), np.where(nm, D, np.inf)
        top, low = -np.sort(-P, axis=1)[:, :2], np.sort(N, axis=1)[:, :2]
        if n >= 2:
            with np.errstate(invalid="ignore"):
                bad |= keep & (pm.sum(1) >= 2) & (top[:, 0] - top[:, 1] <= 4 * t * top[:, 0])
                bad |= keep & (nm.sum(1) >= 2) & (low[:, 1] - low[:, 0] <= 4 * t * low[:, 1])
        a = np.flatnonzero(keep)
        p, q = np.where(pm, D, 0.0).argmax(1)[a], np.where(nm, D, np.inf).argmin(1)[a]
        d_ap, d_an = D[a, p], np.minimum(D[a, q], D[p, q])
        bad[a] |= np.abs(d_ap - d_an + MARGIN) <= 4 * t * (d_ap + d_an + MARGIN)
        bad[a] |= np.abs(D[a, q] - D[p, q]) <= 4 * t * np.maximum(D[a, q], D[p, q])
        if not bad.any():
            return e
        for i in np.flatnonzero(bad):
            e[i] = draw(i, rng)
    raise AssertionError("the triplet input did not settle")


def triplet_clustered(n, d, seed=0):
    """Class centres plus noise whose scale differs per class: tight classes give inactive triplets (d_ap + margin < d_an),
    loose ones active triplets; both shares and both outcomes of the swap test are at least a tenth (asserted by the
    tests from triplet_gaps).  Anchor 0 has no positive, the last anchor no negative."""
    rng = np.random.default_rng(1000 * seed + 7 * n + d)
    ncls = max(2, n // 8)
    lab = rng.integers(0, ncls, n)
    cen = rng.standard_normal((ncls, d)) * (0.5 / np.sqrt(d))
    sig = rng.uniform(0.05, 0.8, ncls) / np.sqrt(d)

    def draw(i, rng):
        return cen[lab[i]] + sig[lab[i]] * rng.standard_normal(d)

    e = np.stack([draw(i, rng) for i in range(n)])
    pm, nm = masks_from_labels(lab)
    pm[0] = False
    nm[n - 1] = False
    return _settle(e, pm, nm, draw, rng), pm, nm


def triplet_inactive(n, d, seed=0):
    """well separated tight classes: d_ap + margin < d_an for every triplet -> loss 0, gradient 0, num_non_zero 0"""
    rng = np.random.default_rng(2000 * seed + 7 * n + d)
    ncls = max(2, n // 8)
    lab = np.arange(n) % ncls
    cen = rng.standard_normal((ncls, d)) * (3.0 / np.sqrt(d))

    def draw(i, rng):
        return cen[lab[i]] + 0.15 / np.sqrt(d) * rng.standard_normal(d)

    e = np.stack([draw(i, rng) for i in range(n)])
    pm, nm = masks_from_labels(lab)
    return _settle(e, pm, nm, draw, rng), pm, nm


def triplet_integer(n, d, seed=0, row0_in_class0=True):
    """Small-integer embeddings (every squared distance an exact integer below 2^20, so fp32 and float64 agree on every
    comparison of two distances) drawn from a small pool of points, whatever the class: equidistant positives and
    negatives and zero distances to both are plentiful.  Class 0 is one point repeated, so every positive of its anchors
    is at distance 0 and ties with the masked-out zeros: the reference's argmax then returns index 0 of the row, which
    is a row of class 0 (the anchor itself for anchor 0) or, with row0_in_class0=False, a row of another class.  Row 5
    repeats the point of class 0 from another class: l = 0 - 0 + margin, an active triplet with both distances zero."""
    rng = np.random.default_rng(3000 * seed + 7 * n + d)
    ncls = max(3, n // 10)
    lab = rng.integers(1, ncls, n)
    lab[1:4] = 0
    lab[0] = 0 if row0_in_class0 else 1
    lab[5] = 2
    pts = rng.integers(-3, 4, (max(4, n // 3), d))
    e = pts[rng.integers(0, len(pts), n)].astype(np.float32)
    e[lab == 0] = pts[0]
    e[5] = pts[0]
    pm, nm = masks_from_labels(lab)
    return e, pm, nm


def triplet_autograd64(e, a, p, q, margin):
    """float64 torch autograd of the loss formula for fixed triplets; a zero distance contributes no gradient and the
    swap picks D[p][n] only where it is strictly smaller (the kernel's conventions).  Returns (loss, grad)."""
    import torch
    x = torch.from_numpy(np.asarray(e, np.float64)).requires_grad_(True)
    a, p, q = (torch.from_numpy(np.asarray(v, np.int64)) for v in (a, p, q))

    def dist(i, j):
        d2 = ((x[i] - x[j]) ** 2).sum(1)
        return torch.where(d2 > 0, torch.sqrt(torch.where(d2 > 0, d2, torch.ones_like(d2))), torch.zeros_like(d2))

    if len(a) == 0:
        return 0.0, np.zeros(x.shape)
    d_an, d_pn = dist(a, q), dist(p, q)
    li = torch.relu(dist(a, p) - torch.where(d_pn < d_an, d_pn, d_an) + margin)
    loss = li[li > 0].mean() if (li > 0).any() else li.sum() * 0
    loss.backward()
    return float(loss.detach()), x.grad.numpy()


# ------------------------------------------------------------------------------------------------ recall, ingest
def recall_indices(qpos, mpos, k, seed):
    """retrieved-neighbour lists for egonn_recall_counts called on its own: half the entries among the 30 map rows
    nearest in position, half anywhere, a -1 tail of random length on a third of the queries (k > m style), one query
    with nothing retrieved"""
    rng = np.random.default_rng(seed)
    nq, m = len(qpos), len(mpos)
    idx = rng.integers(0, m, (nq, k))
    if nq:
        near = np.argsort(np.linalg.norm(qpos[:, None, :] - mpos[None, :, :], axis=2), axis=1)[:, :30]
        pick = np.take_along_axis(near, rng.integers(0, near.shape[1], (nq, k)), 1)
        idx = np.where(rng.random((nq, k)) < 0.5, pick, idx)
    idx = idx.astype(np.int32)
    for i in range(0, nq, 3):
        idx[i, rng.integers(1, k + 1):] = -1
    if nq > 2:
        idx[2] = -1
    return idx


def ingest_batch(total, nscans, seed, extra=0, stride=4, offsets=None):
    """raw (total + extra, stride) float32 rows and scan offsets: z around the ground levels, a tenth of the rows
    all-zero, a few NaN, so the keep mask is irregular and a lost or doubled block carry moves every later row.  The
    `extra` rows behind the batch end hold points every filter setting would keep."""
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal((total + extra, stride), dtype=np.float32)
    raw[:, 2] -= np.float32(1.2)
    raw[rng.random(total + extra) < 0.1, :3] = 0.0
    raw[rng.integers(0, max(total, 1), min(total, 7)), 2] = np.nan
    raw[total:, :3] = np.float32(5.0)
    if offsets is None:
        cuts = np.sort(rng.integers(0, total + 1, nscans - 1)) if nscans > 1 else np.zeros(0, np.int64)
        offsets = [0] + [int(c) for c in cuts] + [total]
    assert offsets[0] == 0 and offsets[-1] == total
    return np.ascontiguousarray(raw), list(offsets)


def threshold_scan(dataset_type):
    """One small scan with values placed by hand next to the two thresholds: every (x, y, z) combination of a set around
    |v| <= 1e-8, and z at float32(ground level) and its two neighbours, +-inf and NaN, beside fine, zero and NaN x / y."""
    from oracle.ingest_ref import GROUND_PLANE_LEVEL
    f = np.float32
    t = f(1e-8)
    tiny = [f(0.0), f(-0.0), t, -t, np.nextafter(t, f(0)), np.nextafter(t, f(1)), -np.nextafter(t, f(1)),
            -np.nextafter(t, f(0)), f(1e-45), f(-1e-39), f(1.0), f(np.nan), f(np.inf)]
    rows = [(x, y, z) for x in tiny for y in tiny for z in tiny]
    lv = f(GROUND_PLANE_LEVEL[dataset_type])
    zs = [lv, np.nextafter(lv, f(0)), np.nextafter(lv, f(-10)), f(np.nan), f(np.inf), f(-np.inf), f(0.0), f(-0.0)]
    rows += [(x, y, z) for z in zs for x, y in ((f(1), f(1)), (f(0), f(0)), (f(np.nan), f(2)), (f(2), f(np.nan)),
                                                (f(0), f(np.nan)), (t, f(0)))]
    raw = np.zeros((len(rows), 4), np.float32)
    raw[:, :3] = np.array(rows, np.float32)
    raw[:, 3] = 7.0
    return raw


def triplet_accept(got, want, tol, scale=1.0):
    """THE acceptance rule of the triplet tests, host and GPU alike: got = (loss, stats, (a, p, n), grad) of the code under
    test, want the same from the float64 reference, tol from egonn_ref.triplet_bounds.  Indices and counts equal, loss /
    statistics / gradient (divided by `scale`, the incoming gradient of backward) within their bounds, non-finite
    statistics equal.  Raises AssertionError."""
    loss, stats, trip, grad = got
    wl, ws, wt, wg = want
    for x, y, name in zip(trip, wt, "apn"):
        assert np.array_equal(x, y), name
    assert stats["num_triplets"] == ws["num_triplets"] and stats["num_non_zero_triplets"] == ws["num_non_zero_triplets"]
    print(f"loss {loss!r} want {wl!r} allowed {tol['loss']:.3g}")
    assert abs(loss - wl) <= tol["loss"], (loss, wl, tol["loss"])
    for k, v in ws.items():
        print(f"{k} {stats[k]!r} want {v!r} allowed {tol[k]:.3g}")
        assert (stats[k] == v) if not np.isfinite(v) else (abs(stats[k] - v) <= tol[k]), (k, stats[k], v, tol[k])
    err = np.abs(np.asarray(grad, np.float64) / scale - wg)
    print(f"grad max err {err.max(initial=0.0):.3g}, max allowed {tol['grad'].max(initial=0.0):.3g}")
    assert np.isfinite(grad).all() and (err <= tol["grad"]).all()

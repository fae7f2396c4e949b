"""CPU tests of the checkers behind test_gpu_ingest.py, test_gpu_retrieval.py and test_gpu_triplet.py (no GPU needed).
A checker that accepts everything tests nothing, so for each of them: (a) the float64 reference's own answer passes,
(b) a numpy float32 restatement of the kernel's arithmetic passes with the DERIVED tolerance on every real-valued input
the GPU tests use, (c) planted errors are rejected."""
import numpy as np
import pytest

from oracle import egonn_ref as ref
from oracle import ingest_ref as I
from oracle import retrieval_ref as R
from tests import ends_data as E


# ------------------------------------------------------------------------------------------------ ingest
def test_ingest_reference_equals_row_loop_on_threshold_scan():
    for ds in I.GROUND_PLANE_LEVEL:
        pc = E.threshold_scan(ds)[:, :3]
        for rz in (True, False):
            for rg in (True, False):
                keep = I.keep_loop(pc, ds, rz, rg)
                want = I.preprocess(pc, ds, rz, rg)
                assert np.array_equal(pc[keep], want, equal_nan=True), (ds, rz, rg)
                assert 0 < keep.sum() <= len(pc)
        both = I.keep_loop(pc, ds, True, True)
        assert both.sum() < I.keep_loop(pc, ds, True, False).sum() < len(pc)     # each switch drops rows of its own
        assert both.sum() < I.keep_loop(pc, ds, False, True).sum() < len(pc)


def test_ingest_batch_reference_ignores_rows_behind_the_end():
    raw, off = E.ingest_batch(5000, 3, seed=1, extra=100)
    pts, noff = I.filter_batch(raw, off, "kitti")
    assert noff[-1] == len(pts) < off[-1] and len(noff) == len(off)
    pts2, noff2 = I.filter_batch(raw[:off[-1]], off, "kitti")
    assert np.array_equal(pts, pts2, equal_nan=True) and noff == noff2
    keep = I.keep_loop(raw[:off[-1]], "kitti")
    assert np.array_equal(raw[:off[-1], :3][keep], pts, equal_nan=True)
    assert 0.2 < keep.mean() < 0.8                                                # an irregular mask, not all or nothing


# ------------------------------------------------------------------------------------------------ kNN certificate
@pytest.mark.parametrize("name", sorted(E.KNN_REAL))
def test_knn_certificate_accepts_float64_and_fp32_restatement(name):
    qs, db, k = E.KNN_REAL[name]()
    tol = R.knn_tol(db.shape[1])
    idx, dist = R.knn(qs, db, k)                                                  # (a) float64 argsort, fp32 inputs
    assert R.knn_certificate(qs, db, idx, dist, tol) == []
    idx32, dist32 = R.knn_fp32(qs, db, k)                                         # (b) the kernel's arithmetic in numpy
    assert R.knn_certificate(qs, db, idx32, dist32, tol) == []
    D = R.dist64(qs, db)
    err = np.abs(dist32[:, :min(k, len(db))] - np.take_along_axis(D, idx32[:, :min(k, len(db))].astype(np.int64), 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.nan_to_num(err / np.take_along_axis(D, idx32[:, :min(k, len(db))].astype(np.int64), 1)).max()
    assert rel <= tol, (rel, tol)                                                 # the bound holds; how closely is printed
    print(f"{name}: fp32 restatement max rel distance error {rel:.3g}, bound {tol:.3g}, "
          f"{(idx32 != idx).sum()} of {idx.size} indices differ from the float64 argsort")


def test_knn_tol_value():
    assert R.knn_tol(256) == pytest.approx(7 * 2.0 ** -24) and R.knn_tol(1) == R.knn_tol(64) < R.knn_tol(65)


def _small_knn():
    rng = np.random.default_rng(3)
    db = rng.standard_normal((50, 20)).astype(np.float32)
    db[30] = db[4]                                                                # an exact tie for every query
    qs = rng.standard_normal((6, 20)).astype(np.float32)
    qs[0] = db[4]
    return qs, db


def test_knn_certificate_rejects_planted_errors():
    qs, db = _small_knn()
    k, tol = 8, R.knn_tol(20)
    idx, dist = R.knn(qs, db, k)
    assert idx[0, :2].tolist() == [4, 30]
    assert R.knn_certificate(qs, db, idx, dist, tol) == []
    full, fdist = R.knn(qs, db, 50)

    def viol(i=idx, d=dist, q=qs, b=db):
        return R.knn_certificate(q, b, i, d, tol)

    i2, d2 = idx.copy(), dist.copy()                                              # two neighbours swapped across a real gap
    i2[1, [2, 5]], d2[1, [2, 5]] = i2[1, [5, 2]], d2[1, [5, 2]]
    assert any("order" in v for v in viol(i2, d2))
    i2, d2 = idx.copy(), dist.copy()                                              # one neighbour replaced by the (k+1)-th
    i2[2, 3], d2[2, 3] = full[2, k], fdist[2, k]
    assert any("left out" in v or "order" in v for v in viol(i2, d2))
    i2, d2 = idx.copy(), dist.copy()                                              # the last replaced by the (k+1)-th
    i2[2, k - 1], d2[2, k - 1] = full[2, k], fdist[2, k]
    assert any("left out" in v for v in viol(i2, d2))
    i2, d2 = idx.copy(), dist.copy()                                              # a duplicate index
    i2[3, 4], d2[3, 4] = i2[3, 3], d2[3, 3]
    assert any("duplicate" in v for v in viol(i2, d2))
    i2, d2 = idx.copy(), dist.copy()                                              # a tie in the wrong index order
    i2[0, :2] = [30, 4]
    assert any("tie" in v for v in viol(i2, d2))
    i2, d2 = idx.copy(), dist.copy()                                              # a distance off by 10 tolerances
    d2[4, 2] *= np.float32(1 + 10 * tol)
    assert any("distance" in v for v in viol(i2, d2))
    i2, d2 = idx.copy(), dist.copy()                                              # an index out of range
    i2[5, 0] = 50
    assert any("range" in v for v in viol(i2, d2))
    # k > m: the -1 tail is exactly the positions >= m
    i3, d3 = R.knn(qs, db[:5], 8)
    assert (i3[:, 5:] == -1).all() and viol(i3, d3, b=db[:5]) == []
    i4, d4 = i3.copy(), d3.copy()
    i4[0, 4], d4[0, 4] = -1, np.inf                                               # a -1 one position early
    assert any("range" in v for v in viol(i4, d4, b=db[:5]))
    i4, d4 = i3.copy(), d3.copy()
    i4[0, 5], d4[0, 5] = 0, 1.0                                                   # an index where the tail must be
    assert any("tail" in v for v in viol(i4, d4, b=db[:5]))
    # the tie rule at the cut: k = 1 for the query that equals rows 4 and 30
    assert any("tie at the cut" in v for v in viol(np.array([[30]]), np.array([[0.0]], np.float32), q=qs[:1]))
    assert viol(np.array([[4]]), np.array([[0.0]], np.float32), q=qs[:1]) == []


def test_knn_exact_reference_and_fp32_restatement_agree_on_integers():
    rng = np.random.default_rng(5)
    for d, m in ((1, 5), (65, 257), (100, 31)):
        db = rng.integers(-7, 8, (m, d)).astype(np.float32)
        qs = rng.integers(-7, 8, (4, d)).astype(np.float32)
        qs[0] = db[m // 2]
        for k in (1, m, m + 2):
            want = R.knn_exact_int(qs, db, k)
            got = R.knn_fp32(qs, db, k)
            assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])
            assert R.knn_certificate(qs, db, *want, tol=0.5 * 2.0 ** -23) == []    # exact sums: only sqrtf rounds


def test_knn_fp32_restatement_non_finite_contract():
    """+inf distances are neighbours like any other (after every finite one, in index order); NaN distances never are."""
    db = np.array([[0.0], [np.inf], [3e38], [-3e38], [np.nan], [1.0]], np.float32)
    qs = np.array([[0.5], [3e38], [np.nan]], np.float32)
    idx, dist = R.knn_fp32(qs, db, 6)
    assert idx[0].tolist() == [0, 5, 1, 2, 3, -1] and np.isinf(dist[0, 2:]).all()      # 3e38^2 overflows to +inf
    assert idx[1].tolist() == [2, 0, 1, 3, 5, -1] and dist[1, 0] == 0.0
    assert (idx[2] == -1).all() and np.isinf(dist[2]).all()


# ------------------------------------------------------------------------------------------------ recall
def test_recall_floor_needs_the_origin_shift():
    qpos, mpos = E.recall_utm(11, 2000, 1000, 2)
    assert R.recall_floor(qpos, mpos, 20.0) < 2e-3                                # shifted: offsets of a few km
    assert R.recall_margin(qpos, mpos, E.RADII) > E.ROOM
    assert R.recall_floor(qpos, mpos, 20.0, origin=np.zeros(2)) > 1.0             # the same data cast to fp32 as it is
    assert R.recall_margin(qpos, mpos, E.RADII, origin=np.zeros(2)) < 1.0         # ... is not decidable
    # and it really is not: fp32 without the shift changes counts, with the shift it does not
    idx = E.recall_indices(qpos, mpos, 10, seed=0)
    idx[idx < 0] = 0
    want = R.recall_counts(idx, qpos, mpos, E.RADII, 10)
    origin = mpos.mean(0)
    q32, m32 = (qpos - origin).astype(np.float32), (mpos - origin).astype(np.float32)
    assert np.array_equal(R.recall_counts(idx, q32, m32, np.float32(E.RADII), 10), want)
    assert not np.array_equal(R.recall_counts(idx, qpos.astype(np.float32), mpos.astype(np.float32),
                                              np.float32(E.RADII), 10), want)
    assert (want[0] == 0).all() and (want[-1] == len(qpos)).all() and 0 < want[1, 0] < want[2, -1] < len(qpos)


@pytest.mark.parametrize("pd,nq,seed,m", E.RECALL_SETS)
def test_recall_inputs_keep_the_floor_and_fp32_agrees(pd, nq, seed, m):
    """every recall input of the GPU tests: the floor holds with room, and an fp32 evaluation of the origin-shifted
    positions (what recall_kernel is given) counts exactly what float64 counts on the UTM-scale positions"""
    qpos, mpos = E.recall_utm(seed, m, nq, pd)
    assert R.recall_margin(qpos, mpos, E.RADII) > E.ROOM
    for s in (nq + pd, 999):                                                      # the GPU tests' neighbour lists
        idx = E.recall_indices(qpos, mpos, 12, seed=s)
        want = R.recall_counts(idx, qpos, mpos, E.RADII, 12)
        origin = mpos.mean(0)
        got = R.recall_counts(idx, (qpos - origin).astype(np.float32), (mpos - origin).astype(np.float32),
                              np.float32(E.RADII), 12)
        assert np.array_equal(got, want)
        assert (np.diff(want, axis=1) >= 0).all()                                 # monotone in nn
        ratios = R.recall(idx, qpos, mpos, list(E.RADII), 12)                    # the ratios are these counts / n
        for ri, r in enumerate(E.RADII):
            assert ratios[r] == [c / max(nq, 1) for c in want[ri]]


def test_recall_counts_boundary_and_tail():
    mpos = np.array([[3.0, 4.0], [30.0, 40.0], [0.0, 6.0]])
    qpos = np.zeros((2, 2))
    idx = np.array([[1, 0, -1], [-1, -1, -1]])
    tp = R.recall_counts(idx, qpos, mpos, [np.nextafter(5.0, 0), 5.0, 50.0], 3)
    assert tp.tolist() == [[0, 0, 0], [0, 1, 1], [1, 1, 1]]                       # distance exactly 5 at radius 5 counts


# ------------------------------------------------------------------------------------------------ triplet loss
TRIPLET_SETS = [("clustered", 255, 256), ("clustered", 256, 256), ("clustered", 257, 256), ("clustered", 300, 256),
                ("clustered", 512, 256), ("clustered", 1024, 256), ("clustered", 40, 1), ("clustered", 40, 33),
                ("clustered", 40, 1000), ("clustered", 40, 4096), ("inactive", 300, 256), ("inactive", 9, 5)]


_within = E.triplet_accept


@pytest.mark.parametrize("kind,n,d", TRIPLET_SETS)
def test_triplet_inputs_unambiguous_and_fp32_restatement_within_bounds(kind, n, d):
    e, pm, nm = getattr(E, "triplet_" + kind)(n, d)
    g = ref.triplet_gaps(e, pm, nm, E.MARGIN)
    assert min(g["pos"], g["neg"], g["kink"], g["swap"]) > 2.0, g                 # built with room: 2 floors
    if kind == "clustered" and d == 256:
        assert 0.1 <= g["active"] <= 0.9 and 0.1 <= g["swapped"] <= 0.9, g
    if kind == "inactive":
        assert g["active"] == 0.0 and g["triplets"] == n
    wl, ws, wt, wg, tol = ref.triplet_bounds(e, pm, nm, E.MARGIN)                 # (a) float64 against itself
    _within((wl, ws, wt, wg), (wl, ws, wt, wg), tol)
    got = ref.triplet_fp32(e, pm, nm, E.MARGIN)                                   # (b) the kernel's arithmetic in numpy
    _within(got, (wl, ws, wt, wg), tol)
    # the derived gradient bound is no looser than the older rtol=1e-3, atol=1e-6
    assert (tol["grad"] <= 1e-6 + 1e-3 * np.abs(wg)).all()
    print(f"{kind} n={n} d={d}: grad err {np.abs(got[3] - wg).max():.3g} (allowed up to {tol['grad'].max():.3g}), "
          f"loss err {abs(got[0] - wl):.3g} (allowed {tol['loss']:.3g})")


def test_triplet_checks_reject_planted_errors():
    e, pm, nm = E.triplet_clustered(300, 256)
    wl, ws, (a, p, q), wg, tol = ref.triplet_bounds(e, pm, nm, E.MARGIN)
    D = ref.pdist64(e)
    # a hardest positive replaced by the second hardest: index equality sees it, and so does the loss bound somewhere
    i = int(np.flatnonzero(pm[a].sum(1) >= 2)[0])
    second = int(np.argsort(-np.where(pm[a[i]], D[a[i]], -1.0))[1])
    p2 = p.copy()
    p2[i] = second
    assert not np.array_equal(p2, p)
    with pytest.raises(AssertionError):
        _within((wl, ws, (a, p2, q), wg), (wl, ws, (a, p, q), wg), tol)
    s2 = dict(ws, num_non_zero_triplets=ws["num_non_zero_triplets"] + 1)          # num_non_zero off by one
    with pytest.raises(AssertionError):
        _within((wl, s2, (a, p, q), wg), (wl, ws, (a, p, q), wg), tol)
    nz = ws["num_non_zero_triplets"]                                              # ... and what it does to the loss
    with pytest.raises(AssertionError):
        _within((wl * nz / (nz + 1), ws, (a, p, q), wg), (wl, ws, (a, p, q), wg), tol)
    g2 = wg.copy()                                                                # an inactive triplet fed to the gradient
    li = D[a, p] - np.minimum(D[a, q], D[p, q]) + E.MARGIN
    j = int(np.flatnonzero(li <= 0)[0])
    g2[a[j]] += (e[a[j]] - e[p[j]]) / D[a[j], p[j]] / nz
    with pytest.raises(AssertionError):
        _within((wl, ws, (a, p, q), g2), (wl, ws, (a, p, q), wg), tol)
    # an ambiguous input is reported as such: two positives of one anchor at (nearly) the same distance
    e2 = e.copy()
    r = int(a[i])
    j1, j2 = np.argsort(-np.where(pm[r], D[r], -1.0))[:2]
    e2[j2] = e2[r] + (e2[j1] - e2[r]) * np.float32(1 - 1e-7)
    assert ref.triplet_gaps(e2, pm, nm, E.MARGIN)["pos"] < 1.0


def test_triplet_gradient_reference_equals_float64_autograd():
    import torch
    for e, pm, nm in (E.triplet_clustered(300, 256), E.triplet_integer(300, 8), E.triplet_integer(40, 3, row0_in_class0=False)):
        wl, ws, (a, p, q), wg, _ = ref.triplet_bounds(e, pm, nm, E.MARGIN)
        loss, grad = E.triplet_autograd64(e, a, p, q, E.MARGIN)
        assert abs(loss - wl) < 1e-12 and np.isfinite(grad).all()
        assert np.abs(grad - wg).max() < 1e-12


def test_triplet_integer_sets_hit_the_ties_and_zero_distances():
    for flag in (True, False):
        e, pm, nm = E.triplet_integer(300, 8, row0_in_class0=flag)
        assert (e == np.round(e)).all()
        D = ref.pdist64(e)
        _, st, (a, p, q) = ref.batch_hard_triplet_loss(e, pm, nm, E.MARGIN)
        cls0 = np.flatnonzero(pm[:, 1] | (np.arange(len(e)) == 1))                # the repeated point's class
        assert (p[np.isin(a, cls0)] == 0).all()                                   # all-zero row: argmax is index 0
        assert pm[1, 0] == flag
        both = (D[a, p] == 0) & (D[a, q] == 0)                                    # both gradient guards, in an active triplet
        assert both.any() if flag else (D[a, p][np.isin(a, cls0)] > 0).all()      # (index 0 of another class is no duplicate)
        assert (D[a, q] == D[p, q]).any() or not flag                             # the swap comparison on a tie
        top = np.sort(np.where(nm, D, np.inf), axis=1)
        assert (top[:, 0] == top[:, 1]).any()                                     # equidistant negatives
        g = ref.triplet_gaps(e, pm, nm, E.MARGIN, allow_ties=True)
        assert min(g["pos"], g["neg"], g["kink"], g["swap"]) > 2.0, g             # whatever is not a tie is far from one

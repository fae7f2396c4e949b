"""GPU tests of the loop-closure layer (run with -m gpu on an MI355X): the windowed kNN against the parent's `retrieval.knn` per
query (indices equal, distances bit-equal) and against the float64 restatement on exactly representable inputs; the time
windows on Unix-scale float64 stamps; the radius counts on a lattice; the precision/recall arrays and scalars against
tests/loop_closure_ref.py; and LoopDetector on a planted trajectory, batched pushes against one offline detect."""
import math

import numpy as np
import pytest
import torch

from tests import loop_closure_ref as ref
from tests.test_registration_host import metrics_f64, planted_pair
from tests.test_relocalize_host import NO_CANDIDATE, PLANTED_H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    g.build()
    import egonn_amd
    return egonn_amd


def _np(t):
    return t.detach().cpu().numpy()


def _cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _i32(a):
    return _cu(np.asarray(a, np.int32))


def _bits(t):
    return _np(t.contiguous().view(torch.int32))


# ------------------------------------------------------------------ 1. knn_window against the parent's egonn_knn, per query
def _check_vs_parent(gpu, q, db, k, lo, hi, rows=None):
    """`knn_window` of all queries in one call == `retrieval.knn(q[i:i+1], db[lo:hi], k)` with lo added, for every i (or `rows`):
    indices equal, distances equal as int32 bit patterns.  -> (idx, dist) of the one call as numpy."""
    from egonn_amd import retrieval
    M = db.shape[0]
    idx, dist = gpu.knn_window(q, db, k, _i32(hi), None if lo is None else _i32(lo))
    assert idx.shape == (q.shape[0], k) and idx.dtype == torch.int32 and dist.dtype == torch.float32
    for i in (range(q.shape[0]) if rows is None else rows):
        a = 0 if lo is None else max(int(lo[i]), 0)
        b = min(int(hi[i]), M)
        if b <= a:                                            # the parent refuses an empty database: the contract is all (-1, +inf)
            want_i = torch.full((1, k), -1, dtype=torch.int32, device="cuda")
            want_d = torch.full((1, k), math.inf, device="cuda")
        else:
            want_i, want_d = retrieval.knn(q[i:i + 1], db[a:b], k)
            want_i = torch.where(want_i >= 0, want_i + a, want_i)
        assert torch.equal(idx[i:i + 1], want_i), (i, a, b, idx[i], want_i)
        assert np.array_equal(_bits(dist[i:i + 1]), _bits(want_d)), (i, a, b)
    return _np(idx), _np(dist)


def _randn(rng, *shape):
    return _cu(rng.standard_normal(shape).astype(np.float32))


@pytest.mark.parametrize("d", [1, 63, 64, 65, 256, 257])
def test_knn_window_equals_parent_over_descriptor_widths(gpu, d):
    rng = np.random.default_rng(d)
    M, k = 300, 20
    db, q = _randn(rng, M, d), _randn(rng, 6, d)
    _check_vs_parent(gpu, q, db, k, [0, 3, 100, 299, 17, 250], [300, 40, 299, 300, 18, 290])


@pytest.mark.parametrize("k", [1, 20, 63, 64])
def test_knn_window_equals_parent_over_window_lengths(gpu, k):
    """every length at which the list, the four waves, the four-row step or the segments of a window change behaviour; the few
    queries of the call put every window on 16 segments"""
    rng = np.random.default_rng(100 + k)
    M, d = 1200, 64
    lengths = sorted({0, 1, 3, 4, 5, max(k - 1, 0), k, k + 1, 15, 16, 17, 255, 256, 257, 1025})
    lo = [7 * j for j in range(len(lengths))]
    hi = [a + n for a, n in zip(lo, lengths)]
    assert max(hi) <= M
    db, q = _randn(rng, M, d), _randn(rng, len(lengths), d)
    idx, _ = _check_vs_parent(gpu, q, db, k, lo, hi)
    for j, n in enumerate(lengths):
        assert (idx[j] >= 0).sum() == min(n, k)


def test_knn_window_bounds_are_clamped(gpu):
    rng = np.random.default_rng(5)
    M, d, k = 90, 33, 20
    db, q = _randn(rng, M, d), _randn(rng, 8, d)
    #     lo > 0    lo = hi   lo > hi   lo < 0    hi > M    both      hi = 0   hi < 0
    lo = [30,       40,       50,       -5,       80,       -1000,    0,       0]
    hi = [60,       40,       10,       12,       M + 7,    10 ** 9,  0,       -3]
    idx, dist = _check_vs_parent(gpu, q, db, k, lo, hi)
    assert (idx[1] == -1).all() and (idx[2] == -1).all() and (idx[6] == -1).all() and (idx[7] == -1).all() and np.isinf(dist[1]).all()
    assert idx[0].min() >= 30 and idx[0].max() < 60 and idx[4][idx[4] >= 0].min() >= 80 and (idx[4] >= 0).sum() == 10
    _check_vs_parent(gpu, q, db, k, None, hi)                 # win_lo = None is lo = 0


def test_knn_window_empty_sides(gpu):
    q = torch.ones((3, 16), device="cuda")
    idx, dist = gpu.knn_window(q, torch.zeros((0, 16), device="cuda"), 5, _i32([0, 4, -1]))
    assert (_np(idx) == -1).all() and np.isinf(_np(dist)).all() and (_np(dist) > 0).all()
    idx, dist = gpu.knn_window(torch.zeros((0, 16), device="cuda"), torch.ones((7, 16), device="cuda"), 5, _i32([]))
    assert idx.shape == (0, 5) and dist.shape == (0, 5)


def test_knn_window_ties_go_to_the_lower_index(gpu):
    """copies of one row dealt to different waves (index mod 4) and to different segments of the window: the lower index wins,
    as in the parent; then a database of equal rows"""
    rng = np.random.default_rng(6)
    M, d = 1200, 48
    base = rng.standard_normal((M, d)).astype(np.float32)
    qv = rng.standard_normal(d).astype(np.float32)
    copies = [1101, 10, 7, 613, 5, 1028]                      # 5 -> wave 1, 7 -> wave 3, 10 -> wave 2 (lo = 0); far ones: other segments
    near = qv + 0.001 * rng.standard_normal(d).astype(np.float32)
    base[copies] = near
    db, q = _cu(base), _cu(np.stack([qv, qv, qv]))
    idx, dist = _check_vs_parent(gpu, q, db, 4, [0, 6, 0], [M, M, 1028])
    assert idx[0].tolist() == [5, 7, 10, 613] and idx[1].tolist() == [7, 10, 613, 1028] and idx[2].tolist() == [5, 7, 10, 613]
    assert len(set(dist[0].tolist())) == 1
    same = torch.ones((700, 20), device="cuda") * 0.5
    q2 = torch.zeros((2, 20), device="cuda")
    idx, dist = _check_vs_parent(gpu, q2, same, 64, [0, 101], [700, 650])
    assert idx[0].tolist() == list(range(64)) and idx[1].tolist() == list(range(101, 165)) and len(set(dist.reshape(-1).tolist())) == 1


def test_knn_window_infinite_and_nan_rows(gpu):
    rng = np.random.default_rng(7)
    M, d, k = 40, 70, 20
    base = rng.standard_normal((M, d)).astype(np.float32)
    base[3, 65] = np.inf                                       # +inf distances: after every finite one, in index order
    base[9, 0] = -np.inf
    base[5, 2] = np.nan                                        # never a neighbour
    base[6, :] = np.nan
    base[11, 1] = 3e38                                         # overflows to +inf in the squared sum
    db, q = _cu(base), _randn(rng, 3, d)
    idx, dist = _check_vs_parent(gpu, q, db, k, [0, 2, 4], [16, 14, 8])
    # 16 rows, two of them NaN: 11 finite distances, the three +inf ones in index order, six empty places
    assert idx[0].tolist()[11:] == [3, 9, 11] + [-1] * 6 and np.isinf(dist[0][11:]).all() and np.isfinite(dist[0][:11]).all()
    assert idx[1].tolist()[7:] == [3, 9, 11] + [-1] * 10
    assert set(idx[2][:2].tolist()) == {4, 7} and (idx[2][2:] == -1).all()
    assert 5 not in idx and 6 not in idx


def test_knn_window_is_batch_invariant(gpu):
    """the same queries in one call (520 queries: one workgroup per window) and split over calls of 130, 7 and 1 queries (8 and
    16 segments per window) give the same bits; a sample of them is held to the parent"""
    rng = np.random.default_rng(8)
    M, d, k, Q = 900, 40, 20, 520
    base = rng.standard_normal((M, d)).astype(np.float32)
    base[200:260] = base[100:160]                             # ties across the split points too
    db, q = _cu(base), _randn(rng, Q, d)
    hi = rng.integers(0, M + 1, Q).astype(np.int32)
    lo = (hi * rng.uniform(0, 1.1, Q)).astype(np.int32)
    lo[::3] = 0
    q[5] = db[130]                                            # an exact duplicate pair at distance 0
    lo[5], hi[5] = 0, M
    whole_i, whole_d = gpu.knn_window(q, db, k, _i32(hi), _i32(lo))
    for step, starts in ((130, range(0, Q, 130)), (7, range(0, 140, 7)), (1, range(0, 24))):
        for a in starts:
            b = min(Q, a + step)
            i2, d2 = gpu.knn_window(q[a:b], db, k, _i32(hi[a:b]), _i32(lo[a:b]))
            assert torch.equal(i2, whole_i[a:b]) and np.array_equal(_bits(d2), _bits(whole_d[a:b])), (step, a)
    assert _np(whole_i)[5, :2].tolist() == [130, 230]
    _check_vs_parent(gpu, q, db, k, lo, hi, rows=range(0, 40))


def test_knn_window_equals_float64_on_exact_inputs(gpu):
    """small-integer descriptors: every squared distance is an integer below 2^24, exact in fp32 in any summation order, and
    sqrtf is correctly rounded, so indices and distances equal the restatement exactly"""
    rng = np.random.default_rng(9)
    M, d, k, Q = 150, 33, 20, 12
    base = rng.integers(-8, 9, (M, d)).astype(np.float32)      # squared distance <= 33 * 16^2 = 8448
    base[40:60] = base[20:40]                                  # exact ties
    qs = rng.integers(-8, 9, (Q, d)).astype(np.float32)
    hi = np.array([150, 10, 19, 20, 21, 60, 0, 200, 149, 75, 33, 150], np.int32)
    lo = np.array([0, 0, 0, 0, 0, 20, 0, -3, 140, 80, 30, 1], np.int32)
    idx, dist = gpu.knn_window(_cu(qs), _cu(base), k, _i32(hi), _i32(lo))
    want_i, want_d = ref.knn_window(qs, base, k, lo, hi)
    assert np.array_equal(_np(idx), want_i)
    assert np.array_equal(_np(dist).view(np.int32), want_d.view(np.int32))


# ------------------------------------------------------------------ 2. time windows
def _unix_stamps(n, seed=1):
    """about 10 Hz at Unix scale, every stamp a multiple of 2^-10 s (so t + 30 and t - 30 are exact in float64), with repeats"""
    rng = np.random.default_rng(seed)
    step = np.round((0.1 + 0.004 * rng.standard_normal(n)) * 1024) / 1024
    step[rng.integers(0, n, n // 10)] = 0.0                    # duplicate stamps
    return 1.7e9 + np.cumsum(step)


def test_time_windows_on_unix_scale_stamps(gpu):
    from egonn_amd import loop_closure
    t = _unix_stamps(800)
    assert (np.diff(t) >= 0).all() and (np.diff(t) == 0).sum() > 20
    tq = np.concatenate([t[::7], t[[310, 311, 500]] + 30.0, [t[0] - 5.0, t[-1] + 1e4, t[400] + 30.0 - 2.0 ** -10]])
    for min_gap, max_gap in ((30.0, math.inf), (30.0, 60.0), (0.5, 0.5), (12.25, 40.0)):
        lo, hi = gpu.time_windows(t, tq, min_gap, max_gap)
        want_lo, want_hi = ref.windows(t, tq, min_gap, max_gap)
        assert lo.dtype == torch.int32 and np.array_equal(_np(lo), want_lo) and np.array_equal(_np(hi), want_hi), (min_gap, max_gap)
    lo, hi = gpu.time_windows(_cu(t), _cu(tq), 30.0)          # device tensors in, the same out
    want_lo, want_hi = ref.windows(t, tq, 30.0)
    assert np.array_equal(_np(hi), want_hi) and (_np(lo) == 0).all()
    # a stamp exactly at t_q - min_gap is admissible (with its duplicates), one 2^-10 s short of it is not
    n = len(t[::7])
    for j, e in ((n, 310), (n + 1, 311), (n + 2, 500)):
        assert tq[j] - 30.0 == t[e] and want_hi[j] == np.searchsorted(t, t[e], side="right") > e
    assert want_hi[-1] == np.searchsorted(t, t[400], side="left") and want_hi[-3] == 0 and want_hi[-2] == len(t)
    # fp32 cannot hold these stamps (its spacing at 1.7e9 is 128 s): the restatement in single precision gives other windows
    lo32, hi32 = ref.windows(t, tq, 30.0, 60.0, dtype=np.float32)
    lo64, hi64 = ref.windows(t, tq, 30.0, 60.0)
    assert (hi32 != hi64).mean() > 0.5 and (lo32 != lo64).any()
    # an empty database
    lo, hi = gpu.time_windows(np.zeros(0), tq, 30.0, 60.0)
    assert (_np(lo) == 0).all() and (_np(hi) == 0).all() and lo.shape == (len(tq),)
    lo, hi = gpu.time_windows(t, np.zeros(0), 30.0)
    assert lo.shape == (0,) and hi.shape == (0,)
    # an unsorted database sets the status bit; the windows stay in range
    bad = t.copy()
    bad[[100, 101]] = bad[[101, 100]]
    assert bad[100] > bad[101]
    with pytest.raises(ValueError, match="non-decreasing"):
        gpu.time_windows(bad, tq, 30.0)
    lo, hi, status = loop_closure._time_windows(_cu(bad), _cu(tq), 30.0, 60.0)
    assert int(status.item()) == 1 and 0 <= int(lo.min()) and int(hi.max()) <= len(t) and 0 <= int(hi.min()) and int(lo.max()) <= len(t)
    nan = t.copy()
    nan[-1] = np.nan
    with pytest.raises(ValueError, match="non-decreasing"):
        gpu.time_windows(nan, tq, 30.0)
    _, _, status = loop_closure._time_windows(_cu(t), _cu(tq), 30.0, 60.0)
    assert int(status.item()) == 0


# ------------------------------------------------------------------ 3. radius counts
def _window_radius(qpos, dbpos, lo, hi, radius, pred):
    from egonn_amd import _lib
    import ctypes
    lib = _lib.load()
    Q, M = len(qpos), len(dbpos)
    qp, dp = _cu(np.asarray(qpos, np.float32)), _cu(np.asarray(dbpos, np.float32))
    count = torch.full((Q,), -7, dtype=torch.int32, device="cuda")
    pdist = None if pred is None else torch.full((Q,), -7.0, device="cuda")
    lo_t, hi_t, pr_t = (None if lo is None else _i32(lo)), _i32(hi), (None if pred is None else _i32(pred))
    _lib.call(qp.device, lib.egonn_window_radius, qp.data_ptr(), Q, dp.data_ptr(), M, qp.shape[1], _lib._ptr(lo_t), hi_t.data_ptr(),
              ctypes.c_float(radius), _lib._ptr(pr_t), count.data_ptr(), _lib._ptr(pdist))
    torch.cuda.synchronize()
    return _np(count), None if pdist is None else _np(pdist)


@pytest.mark.parametrize("pd", [2, 3])
def test_window_radius_on_a_lattice(gpu, pd):
    """positions on a 0.25 m lattice: squared distances are multiples of 1/16, exact in fp32, sqrtf is correctly rounded, so
    counts and distances equal the restatement exactly, also for radii that are lattice distances themselves"""
    rng = np.random.default_rng(20 + pd)
    M, Q = 333, 70
    dbpos = rng.integers(-12, 13, (M, pd)).astype(np.float64) * 0.25
    qpos = rng.integers(-12, 13, (Q, pd)).astype(np.float64) * 0.25
    hi = rng.integers(0, M + 1, Q)
    lo = (hi * rng.uniform(0, 1.05, Q)).astype(np.int64)
    lo[:5], hi[:5] = [-4, 0, 100, 200, 0], [M + 9, M, 100, 150, 0]
    pred = rng.integers(0, M, Q)
    pred[:6] = [-1, M, M + 5, -7, 0, M - 1]
    for radius in (0.0, 0.25, 0.75, 0.9, 1.0, 1.25, 1.3, 2.5, 2.6, 100.0):          # 1.25 = |(0.75, 1.0)|: on the lattice
        count, pdist = _window_radius(qpos, dbpos, lo, hi, radius, pred)
        want_c, want_d = ref.window_radius(qpos, dbpos, lo, hi, radius, pred)
        assert np.array_equal(count, want_c), radius
        assert np.array_equal(pdist.view(np.int32), want_d.view(np.int32))
    assert np.isinf(pdist[:4]).all() and np.isfinite(pdist[4:]).all()
    assert count[2] == 0 and count[3] == 0 and count[4] == 0 and count[0] == M
    c2, none = _window_radius(qpos, dbpos, None, hi, 1.25, None)                      # no pred, win_lo = NULL
    assert none is None and np.array_equal(c2, ref.window_radius(qpos, dbpos, None, hi, 1.25)[0])
    on = ref.window_radius(qpos, dbpos, lo, hi, 1.25)[0] - ref.window_radius(qpos, dbpos, lo, hi, 1.2)[0]
    assert on.sum() > 0                                                               # rows exactly at the radius exist and count


# ------------------------------------------------------------------ 4. precision/recall
def _pr_curve(score, correct, revisit):
    from egonn_amd import _lib
    lib = _lib.load()
    n = len(score)
    sc, co, rv = _cu(np.asarray(score, np.float32)), _i32(correct), _i32(revisit)
    outs = [torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda") for _ in range(4)]
    end = torch.full((max(n, 1),), 9, dtype=torch.uint8, device="cuda")
    totals = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    nb = lib.egonn_pr_curve_scratch_bytes(n)
    assert nb > 0
    buf = torch.empty(nb + 256, dtype=torch.uint8, device="cuda")
    off = (-buf.data_ptr()) % 256
    _lib.call(sc.device, lib.egonn_pr_curve, sc.data_ptr(), co.data_ptr(), rv.data_ptr(), n, *[o.data_ptr() for o in outs], end.data_ptr(),
              totals.data_ptr(), buf.data_ptr() + off, nb)
    torch.cuda.synchronize()
    o = [_np(x)[:n] for x in outs]
    return dict(order=o[0], cum_tp=o[1], cum_fp=o[2], cum_rev=o[3], group_end=_np(end)[:n], n_predicted=int(totals[0]),
                n_revisit=int(totals[1]))


def _scores(rng, n, kind):
    if kind == "groups":            # nine distinct values, negative ones and both zeros among them: runs of equal scores far longer
        s = rng.integers(-3, 6, n).astype(np.float32) / 2          # than a workgroup's 256 or a tile's 1024 positions
        s[(s == 0) & (rng.random(n) < 0.5)] = -0.0
    elif kind == "distinct":
        s = rng.standard_normal(n).astype(np.float32) * 100
    elif kind == "all_inf":
        return np.full(n, np.inf, np.float32)
    else:                           # one value
        s = np.full(n, -1.5, np.float32)
    if kind != "one":
        s[rng.random(n) < 0.1] = np.inf
        s[rng.random(n) < 0.05] = np.nan
        s[rng.random(n) < 0.02] = -np.nan
    return s


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 4097])
def test_pr_curve_arrays(gpu, n):
    rng = np.random.default_rng(30 + n)
    for kind in ("groups", "distinct", "all_inf", "one"):
        score = _scores(rng, n, kind)
        correct = rng.integers(0, 2, n) * rng.integers(1, 5, n)       # any non-zero value counts
        revisit = rng.integers(0, 2, n) * -3
        got, want = _pr_curve(score, correct, revisit), ref.pr_curve(score, correct, revisit)
        for name in ("order", "cum_tp", "cum_fp", "cum_rev", "group_end", "n_predicted", "n_revisit"):
            assert np.array_equal(got[name], want[name]), (kind, name)
        if kind == "groups" and n == 4097:
            ends = np.flatnonzero(want["group_end"])
            assert len(ends) == 9 and np.diff(ends).min() > 256 and (np.signbit(score) & (score == 0)).any()
    if n >= 2:                      # -0.0 next to +0.0 is one group, in index order
        got = _pr_curve(np.array([0.0, -0.0] + [1.0] * (n - 2), np.float32), np.ones(n, np.int32), np.ones(n, np.int32))
        assert got["order"][:2].tolist() == [0, 1] and got["group_end"][:2].tolist() == [0, 1]


def _trajectory_case(n, seed):
    """n scans on a 0.25 m lattice at UTM scale whose float64 mean is a lattice point, predictions and scores of mixed quality"""
    rng = np.random.default_rng(seed)
    half = max(n // 2, 1)
    path = np.cumsum(rng.integers(-2, 3, (half, 2)), axis=0)
    P = np.concatenate([path, path[rng.integers(0, half, n - half)] + rng.integers(-6, 7, (n - half, 2))])     # the 2nd half revisits
    P[-1] += (-P.sum(axis=0)) % n                             # the sum is a multiple of n: the mean is a lattice point
    assert (P.sum(axis=0) % n == 0).all()
    pos64 = P.astype(np.float64) * 0.25 + np.array([345090.0, 4037591.25])
    pos32 = ((P - P.sum(axis=0) // n).astype(np.float64) * 0.25).astype(np.float32)
    hi = np.maximum(np.arange(n) - 50, 0).astype(np.int32)
    lo = np.where(rng.random(n) < 0.2, hi // 2, 0).astype(np.int32)
    k = 3
    nn = np.stack([np.where(hi > 0, rng.integers(0, np.maximum(hi, 1)), -1) for _ in range(k)], axis=1).astype(np.int32)
    exact = (rng.random(n) < 0.4) & (np.arange(n) >= half) & (hi > 0)
    for i in np.flatnonzero(exact):                           # a share of good predictions: the nearest admissible scan
        d = np.abs(P[:hi[i]] - P[i]).sum(axis=1)
        nn[i, 0] = int(d.argmin())
    score = np.round(rng.random(n) * 256).astype(np.float32) / 64 - 1.0     # 257 distinct values, negative ones among them
    score[rng.random(n) < 0.05] = np.inf
    return pos64, pos32, lo, hi, nn, score


@pytest.mark.parametrize("n", [0, 1, 257, 4097])
def test_evaluate_loop_closure_equals_restatement(gpu, n):
    """integer curve arrays exactly; precision, recall and the five scalars within 1e-12: both sides are float64 sums of at most
    4097 terms <= 1, so n * 2^-52 ~ 9e-13 bounds their difference (f1_threshold is a score: exact)"""
    if n == 0:
        e = np.zeros
        res = gpu.evaluate_loop_closure(e((0, 3), np.int32), e(0, np.float32), e((0, 2)), e(0, np.int32), e(0, np.int32), 5.0)
        assert res["f1_max"] == 0.0 and res["f1_threshold"] == -math.inf and res["average_precision"] == 0.0
        assert res["extended_precision"] == 0.0 and res["n_revisit"] == 0 and res["n_predicted"] == 0 and len(res["precision"]) == 0
        return
    pos64, pos32, lo, hi, nn, score = _trajectory_case(n, 40 + n)
    radius = 1.25
    for predicted in (None, np.where(np.arange(n) % 5 == 0, -1, nn[:, 1]).astype(np.int32)):
        res = gpu.evaluate_loop_closure(_cu(nn), _cu(score), pos64, _cu(lo), _cu(hi), radius,
                                        None if predicted is None else _cu(predicted))
        pred = nn[:, 0] if predicted is None else predicted
        count, pdist = ref.window_radius(pos32, pos32, lo, hi, radius, pred)
        assert np.array_equal(_np(res["count"]), count) and np.array_equal(_np(res["pred_dist"]).view(np.int32), pdist.view(np.int32))
        sc = np.where(pred < 0, np.inf, score)
        want = ref.curve(sc, pdist <= np.float32(radius), count > 0)
        assert res["n_revisit"] == int((count > 0).sum()) and res["n_predicted"] == int(np.isfinite(sc).sum())
        for name in ("tp", "fp", "fn", "thresholds"):
            assert np.array_equal(res[name], want[name]), name
        for name in ("precision", "recall"):
            assert np.abs(res[name] - want[name]).max(initial=0.0) <= 1e-12, name
        for name in ref.SCALARS:
            print(f"[loop closure] n={n} {name}: device {res[name]!r} restated {want[name]!r}")
            assert res[name] == want[name] or abs(res[name] - want[name]) <= 1e-12, name
        if n == 4097 and predicted is None:
            assert 0 < res["n_revisit"] < n and len(res["tp"]) > 200 and 0.0 < res["average_precision"] < 1.0


# ------------------------------------------------------------------ 5. LoopDetector on a planted trajectory
N_TRAJ, GAP, K_LOOP = 48, 20.0, 4
FIRST = [2, 5, 8, 11, 14, 17]                                  # first visits of the six places that are seen twice
SECOND = [30, 33, 36, 39, 42, 45]


def _trajectory():
    """48 scans, one per second.  Place p is seen at FIRST[p] and again at SECOND[p]: the second visit holds the source side
    of planted_pair(64, 7100 + p, 0.30, 0.05) and the first visit its target side, so T_rel (query keypoints into the
    candidate's frame) is the planted pose.  Every other scan is a place of its own.  Global descriptors: one unit vector per
    place, the two visits 0.01 apart."""
    rng = np.random.default_rng(77)
    feat, kp = np.zeros((N_TRAJ, 64, 128), np.float32), np.zeros((N_TRAJ, 64, 3), np.float32)
    glob = rng.standard_normal((N_TRAJ, 8))
    T = {}
    for i in range(N_TRAJ):
        if i in SECOND:
            continue
        p = FIRST.index(i) if i in FIRST else None
        f1, f2, k1, k2, Tp = planted_pair(64, 7100 + (p if p is not None else 100 + i), 0.30, 0.05)
        feat[i], kp[i] = f2, k2
        if p is not None:
            j = SECOND[p]
            feat[j], kp[j], T[j] = f1, k1, Tp
            glob[j] = glob[i] + 0.01 * rng.standard_normal(8)
    glob = (glob / np.linalg.norm(glob, axis=1, keepdims=True)).astype(np.float32)
    poses = np.tile(np.eye(4), (N_TRAJ, 1, 1))
    poses[:, 0, 3] = 3.0 * np.arange(N_TRAJ)
    out = {"global": torch.from_numpy(glob), "keypoints": torch.from_numpy(kp), "descriptors": torch.from_numpy(feat)}
    return out, 1.7e9 + np.arange(N_TRAJ, dtype=np.float64), poses, T


def _detector(gpu, **kw):
    return gpu.LoopDetector(k=K_LOOP, min_time_gap=GAP, n_k=64, dim=128, global_dim=8, ransac_max_it=PLANTED_H, **kw)


_OFFLINE = {}


def _offline(gpu):
    if not _OFFLINE:
        out, times, poses, T = _trajectory()
        r = _detector(gpu).detect(out, times, poses)
        torch.cuda.synchronize()
        _OFFLINE.update(r={k: _np(v) for k, v in r.items() if not k.startswith("_")}, data=(out, times, poses, T))
    return _OFFLINE["r"], _OFFLINE["data"]


def test_loop_detector_finds_the_planted_revisits(gpu):
    r, (out, times, poses, T) = _offline(gpu)
    assert r["loop"].dtype == np.bool_ and r["loop"].shape == (N_TRAJ,) and r["index"].tolist() == list(range(N_TRAJ))
    assert r["win_hi"].tolist() == [max(i - 19, 0) for i in range(N_TRAJ)] and (r["win_lo"] == 0).all()
    assert r["nn_index"].shape == (N_TRAJ, K_LOOP) and r["T"].shape == (N_TRAJ, K_LOOP, 4, 4)
    # scans of the first 20 s (every first visit among them) have no admissible candidate
    early = np.arange(N_TRAJ) < 20
    assert (r["nn_index"][early] == -1).all() and not r["loop"][early].any() and (r["best_index"][early] == -1).all()
    assert (r["status"][early] & NO_CANDIDATE).all() and np.isinf(r["nn_dist"][early]).all()
    for p, j in enumerate(SECOND):
        assert r["loop"][j] and r["best_index"][j] == FIRST[p] and r["nn_index"][j, 0] == FIRST[p], (j, r["best_index"][j])
        rte, rre, suc = metrics_f64(r["T_rel"][j], T[j])       # the reference's success rule, as tests/test_gpu_relocalize.py
        assert suc == 1 and rte <= 2.0 and rre <= 5.0, (j, rte, rre)
        assert np.allclose(r["pose"][j], poses[FIRST[p]] @ r["T_rel"][j], rtol=0, atol=1e-9)
    lone = [j for j in range(20, N_TRAJ) if j not in SECOND]
    print(f"[loop closure] inliers of the revisits {r['best_inliers'][SECOND].tolist()}, of the other scans {r['best_inliers'][lone].tolist()}")


@pytest.mark.parametrize("batch", [1, 5, 16])
def test_loop_detector_pushes_equal_one_detect(gpu, batch):
    want, (out, times, poses, _) = _offline(gpu)
    det = _detector(gpu)
    parts = []
    for a in range(0, N_TRAJ, batch):
        b = min(N_TRAJ, a + batch)
        parts.append(det.push({k: v[a:b] for k, v in out.items()}, times[a:b], poses[a:b]))
    assert len(det) == N_TRAJ and np.array_equal(_np(det.times), times)
    torch.cuda.synchronize()
    keys = [k for k in parts[0] if not k.startswith("_")]
    assert set(keys) == set(want)
    for k in keys:
        got = np.concatenate([_np(p[k]) for p in parts])
        assert got.dtype == want[k].dtype and np.array_equal(got.view(np.uint8), want[k].view(np.uint8)), k


def test_loop_detector_without_verification(gpu, monkeypatch):
    from egonn_amd import loop_closure
    want, (out, times, poses, _) = _offline(gpu)

    def boom(*a, **kw):
        raise AssertionError("verify=False must not touch the matcher")
    monkeypatch.setattr(loop_closure, "verify_candidates", boom)
    r = _detector(gpu, verify=False).detect(out, times)
    assert set(r) == {"nn_index", "nn_dist", "index", "win_lo", "win_hi", "loop"}
    assert np.array_equal(_np(r["nn_index"]), want["nn_index"]) and np.array_equal(_np(r["nn_dist"]), want["nn_dist"])
    assert np.array_equal(_np(r["loop"]), np.arange(N_TRAJ) >= 20)
    both = gpu.detect_loops(out["global"], times, K_LOOP, GAP)
    for k in ("nn_index", "nn_dist", "win_lo", "win_hi"):
        assert np.array_equal(_np(both[k]), want[k]), k
    with pytest.raises(ValueError, match="non-decreasing"):
        gpu.detect_loops(out["global"], times[::-1].copy(), K_LOOP, GAP)

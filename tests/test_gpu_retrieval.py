"""GPU tests of kNN and recall@k (egonn_amd/csrc/retrieval.hip, egonn_amd/retrieval.py) at the shapes where their loops
are ragged or wrap.  Two kinds of kNN input: integer-valued embeddings, on which every fp32 sum is exact and the answer
is fixed bit for bit (the tie rule, the ragged lanes, m not a multiple of 4), and real-valued ones, on which the answer
is CERTIFIED by oracle/retrieval_ref.knn_certificate with a tolerance derived from the kernel's operation count
(retrieval_ref.knn_tol): no share of mismatches is allowed anywhere.  Recall counts are integers and must equal the
float64 reference on inputs that fp32 provably cannot flip (retrieval_ref.recall_floor), plus exact boundary cases."""
import numpy as np
import pytest
import torch

from tests import ends_data as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    g.build()
    from egonn_amd import _lib
    return _lib.require_gpu()


def _knn(dev, qs, db, k, **kw):
    from egonn_amd import retrieval
    idx, dist = retrieval.knn(torch.from_numpy(qs).to(dev), torch.from_numpy(db).to(dev), k, **kw)
    assert idx.dtype == torch.int32 and idx.shape == dist.shape == (len(qs), k)
    return idx.cpu().numpy(), dist.cpu().numpy()


def _int_case(d, m, nq, seed, lim):
    """integer embeddings in [-lim, lim]; duplicates of row 1 land in other lanes, waves and strides of both kernels
    (rows r, r+1.. go to different waves of the distance kernel; i, i+64, i+256 to another lane's wave / the same thread's
    next stride of the selection); query 0 equals a database row (distance exactly 0)"""
    rng = np.random.default_rng(seed)
    db = rng.integers(-lim, lim + 1, (m, d)).astype(np.float32)
    for j in (2, 65, 130, 257, 1000, m - 1):
        if 1 < j < m:
            db[j] = db[1]
    qs = rng.integers(-lim, lim + 1, (nq, d)).astype(np.float32)
    if m > 1:
        qs[0] = db[1]
    return qs, db


# d, m, ks: every value of each axis once, next to neighbour values of the others
EXACT = [(1, 1, (1, 2)), (3, 2, (1, 2, 3, 4)), (63, 3, (2, 3, 6)), (64, 4, (1, 3, 4, 5)), (65, 5, (4, 5, 10)),
         (100, 255, (1, 254, 255, 256)), (256, 256, (2, 256, 512)), (257, 257, (1, 257, 258)), (1000, 1023, (2, 1022)),
         (4096, 4099, (1, 25, 4099, 4100)), (1, 4099, (3, 8198)), (3, 1023, (1023, 1024))]


@pytest.mark.parametrize("d,m,ks", EXACT)
def test_knn_exact_on_integer_embeddings(dev, d, m, ks):
    """squared distances are integers below 2^24: indices AND distances equal the stable argsort of the fp32 square
    roots bit for bit, the -1 / inf tail beyond m included"""
    from oracle import retrieval_ref as R
    qs, db = _int_case(d, m, 7, seed=d + m, lim=7 if d > 256 else 15)
    for k in ks:
        idx, dist = _knn(dev, qs, db, k)
        widx, wdist = R.knn_exact_int(qs, db, k)
        assert np.array_equal(idx, widx), (d, m, k)
        assert np.array_equal(dist, wdist), (d, m, k)
    if m > 2:
        assert dist[0, 0] == 0.0 and dist[0, 1] == 0.0 and idx[0, 0] <= 1 and idx[0, 0] < idx[0, 1] <= 2   # duplicates, lower index first


@pytest.mark.parametrize("nq,chunk", [(0, 4096), (1, 4096), (255, 4096), (4095, 4096), (4096, 4096), (4097, 4096),
                                      (8193, 4096), (255, 100), (257, 1)])
def test_knn_query_chunks(dev, nq, chunk):
    """the Python chunk loop of retrieval.knn: every query answered once, whatever the chunk boundary"""
    from oracle import retrieval_ref as R
    rng = np.random.default_rng(nq + chunk)
    db = rng.integers(-15, 16, (37, 5)).astype(np.float32)
    qs = rng.integers(-15, 16, (nq, 5)).astype(np.float32)
    idx, dist = _knn(dev, qs, db, 3, chunk=chunk)
    widx, wdist = R.knn_exact_int(qs, db, 3)
    assert np.array_equal(idx, widx) and np.array_equal(dist, wdist)


@pytest.mark.parametrize("name", sorted(E.KNN_REAL))
def test_knn_certified_on_real_embeddings(dev, name):
    """a valid k-nearest list up to fp32 rounding, complete statement in knn_certificate; tol = knn_tol(d) =
    ((ceil(d/64) + 8) / 2 + 1) * 2^-24, derived from the kernel's operation count (see knn_tol), not measured"""
    from oracle import retrieval_ref as R
    qs, db, k = E.KNN_REAL[name]()
    idx, dist = _knn(dev, qs, db, k)
    bad = R.knn_certificate(qs, db, idx, dist, R.knn_tol(db.shape[1]))
    assert bad == [], bad[:5]


def test_knn_non_finite_distances(dev):
    """the contract of include/egonn_hip.h: +inf distances are neighbours after every finite one, in index order, each
    once (also when k > m); a NaN distance is never a neighbour and the list ends early with (-1, inf)"""
    from oracle import retrieval_ref as R
    db = np.array([[0.0], [np.inf], [3e38], [-3e38], [np.nan], [1.0]], np.float32)
    qs = np.array([[0.5], [3e38], [np.nan], [-1.0]], np.float32)
    for k in (1, 5, 6, 9):
        idx, dist = _knn(dev, qs, db, k)
        widx, wdist = R.knn_fp32(qs, db, k)
        assert np.array_equal(idx, widx) and np.array_equal(dist, wdist), k
    rng = np.random.default_rng(1)
    db = rng.standard_normal((300, 70)).astype(np.float32)
    db[[3, 64, 259], 69] = np.inf                                               # three genuine +inf distances
    db[7, 0] = np.nan
    qs = rng.standard_normal((5, 70)).astype(np.float32)
    idx, dist = _knn(dev, qs, db, 302)
    assert (idx[:, 296:299] == [3, 64, 259]).all() and np.isposinf(dist[:, 296:]).all()
    assert (idx[:, 299:] == -1).all() and not (idx == 7).any()
    assert all(len(set(r[:299].tolist())) == 299 for r in idx)


def _counts(dev, idx, qpos32, mpos32, radius, tp=None):
    from egonn_amd import _lib
    L = _lib.load()
    nq, k = idx.shape
    t_idx = torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(dev)
    t_q, t_m = torch.from_numpy(np.ascontiguousarray(qpos32)).to(dev), torch.from_numpy(np.ascontiguousarray(mpos32)).to(dev)
    rad = torch.tensor([float(r) for r in radius], dtype=torch.float32, device=dev)
    if tp is None:
        tp = torch.full((len(radius), k), 123456, dtype=torch.int32, device=dev)      # stale counts: the call must clear them
    with torch.cuda.device(dev):
        _lib.check(L.egonn_recall_counts(t_idx.data_ptr(), t_q.data_ptr(), t_m.data_ptr(), nq, k, qpos32.shape[1],
                                         rad.data_ptr(), len(radius), tp.data_ptr(), _lib._stream()))
    return tp.cpu().numpy(), tp


@pytest.mark.parametrize("pd,nq,seed,m", [s for s in E.RECALL_SETS if s[1] != 203])
def test_recall_counts_equal_float64_reference(dev, pd, nq, seed, m):
    """egonn_recall_counts on origin-shifted fp32 positions == the float64 reference on the UTM-scale positions, exactly.
    Checked first, in float64 and over every (query, map row, radius): |distance - r| exceeds recall_floor(r) =
    (pd + 8) sqrt(pd) 2^-24 L + 2^-24 r  (L = largest offset from the origin; derivation in recall_floor) E.ROOM times."""
    from oracle import retrieval_ref as R
    qpos, mpos = E.recall_utm(seed, m, nq, pd)
    assert R.recall_margin(qpos, mpos, E.RADII) > E.ROOM
    k = 12
    idx = E.recall_indices(qpos, mpos, k, seed=nq + pd)
    origin = mpos.mean(0)
    q32, m32 = (qpos - origin).astype(np.float32), (mpos - origin).astype(np.float32)
    tp_buf = None
    for radius in (E.RADII, E.RADII[2:3], E.RADII[1:4]):                          # five, one and three radii, one buffer
        got, tp_buf = _counts(dev, idx, q32, m32, radius, tp_buf)
        want = R.recall_counts(idx, qpos, mpos, radius, k)
        assert np.array_equal(got[:len(radius)], want), (pd, nq, radius)
        assert (np.diff(got[:len(radius)], axis=1) >= 0).all()                    # monotone in nn, -1 tails included
    got, _ = _counts(dev, idx, q32, m32, E.RADII)
    assert (got[0] == 0).all() and (got[-1] == (idx[:, :1] >= 0).sum()).all() if nq else (got == 0).all()
    # a second call with other neighbours into the same buffer reuses nothing of the first
    idx2 = E.recall_indices(qpos, mpos, k, seed=999)
    got2, _ = _counts(dev, idx2, q32, m32, E.RADII, tp_buf)
    assert np.array_equal(got2, R.recall_counts(idx2, qpos, mpos, E.RADII, k))


def test_recall_counts_on_the_boundary(dev):
    """hand-built cases whose arithmetic is exact in fp32 (3-4-5 and 3-4-12 triangles on integer offsets): a neighbour
    exactly on the radius counts, as `<=` says; one float32 step inside the radius does not"""
    from oracle import retrieval_ref as R
    f = np.float32
    for pd, mrow, dist in ((2, [3, 4], 5.0), (3, [3, 4, 12], 13.0), (2, [-300, 400], 500.0)):
        mpos = np.array([mrow, [1000] * pd, [0] * pd], f)
        mpos[2, 0] = dist + 1                                                     # just outside
        qpos = np.zeros((3, pd), f)
        idx = np.array([[1, 0, 2], [2, 1, -1], [-1, -1, -1]], np.int32)
        radius = [np.nextafter(f(dist), f(0)), f(dist), np.nextafter(f(dist), f(1e9)), f(dist + 1)]
        got, _ = _counts(dev, idx, qpos, mpos, radius)
        want = R.recall_counts(idx, qpos.astype(np.float64), mpos.astype(np.float64), [float(r) for r in radius], 3)
        assert np.array_equal(got, want)
        assert got.tolist() == [[0, 0, 0], [0, 1, 1], [0, 1, 1], [1, 2, 2]]


@pytest.mark.parametrize("pd", [2, 3])
def test_recall_at_k_wrapper_utm_positions(dev, pd):
    """retrieval.recall_at_k with float64 UTM-scale positions (the origin shift is what makes this pass: the host suite
    shows the same data cast to fp32 as it is fails the floor), all queries and a strict subset with repeats, k > m"""
    from egonn_amd import retrieval
    from oracle import retrieval_ref as R
    qs, db, _ = E.knn_unit()
    (seed, m, nq), = [(s, mm, n) for p, n, s, mm in E.RECALL_SETS if p == pd and n == 203]
    db = db[:m]
    qpos, mpos = E.recall_utm(seed, m, nq, pd)
    assert R.recall_margin(qpos, mpos, E.RADII) > E.ROOM
    radius = list(E.RADII)
    for k, sel in ((25, None), (7, [5, 3, 3, 200, 0, 5, 77]), (25, [])):
        out = retrieval.recall_at_k(torch.from_numpy(db), torch.from_numpy(qs), torch.from_numpy(mpos),
                                    torch.from_numpy(qpos), radius=radius, k=k, query_indexes=sel)
        q_sel = qs if sel is None else qs[sel]
        p_sel = qpos if sel is None else qpos[sel]
        idx = out["nn_index"].cpu().numpy()
        assert idx.shape == (len(q_sel), k)
        # recall_at_k returns no distances: the certificate is fed the float64 distances of the returned rows, so its
        # distance clause is vacuous here and it checks range, order, ties and that nothing closer was left out
        dist = np.zeros((0, k), np.float32)
        if len(idx):
            dist = np.take_along_axis(R.dist64(q_sel, db), idx.astype(np.int64), 1).astype(np.float32)
        assert R.knn_certificate(q_sel, db, idx, dist, R.knn_tol(256)) == []
        want = R.recall_counts(idx, p_sel, mpos, radius, k)
        n = max(len(q_sel), 1)
        for ri, r in enumerate(radius):
            assert out["recall"][r] == [c / n for c in want[ri]], (pd, k, r)
    # k > m: the -1 tail neither counts nor crashes, recall stays monotone in nn and flat beyond m
    out = retrieval.recall_at_k(torch.from_numpy(db[:5]), torch.from_numpy(qs), torch.from_numpy(mpos[:5]),
                                torch.from_numpy(qpos), radius=radius, k=9)
    assert R.recall_margin(qpos, mpos[:5], E.RADII) > 1.0                          # another origin, the floor still holds
    idx = out["nn_index"].cpu().numpy()
    assert (idx[:, 5:] == -1).all() and (np.sort(idx[:, :5], axis=1) == np.arange(5)).all()
    want = R.recall_counts(idx, qpos, mpos[:5], radius, 9)
    for ri, r in enumerate(radius):
        assert out["recall"][r] == [c / nq for c in want[ri]]
        assert (np.diff(out["recall"][r]) >= 0).all() and len(set(out["recall"][r][4:])) == 1

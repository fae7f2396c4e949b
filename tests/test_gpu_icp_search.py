"""GPU tests of the ICP target-grid search (run with -m gpu on an MI355X) on the edge geometries of tests/icp_search_data.py:
one evaluation per geometry (icp_pairs(..., max_iteration=0, debug=True)) against the brute-force oracle, bit for bit: j(i) of
every row, n_corr, sum_d2, the fitness and rmse these imply, T = T_init.  No row is excused and nothing has a tolerance:
tests/test_icp_search_host.py shows on the CPU that every geometry reaches its edge of the search and that the winning
distances and their sum are exact.  The same through the point-to-plane entry (icp_search_kernel<1>), the batch against its
pairs alone and against offsets past the capacity, non-finite rows, and the kNN search of estimate_normals (both template
instances, the radius doubling on wide grids) on the four wide or dense target clouds against an exact kNN."""
import numpy as np
import pytest
import torch

from tests import icp_search_data as data
from tests.icp_plane_ref import knn_f64
from tests.test_icp_host import ICP_EMPTY, ICP_MAX_ITER

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


def _cu(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()                     # a copy: the geometries are read-only


def _bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def _offsets(clouds, past=0):
    off = np.zeros(len(clouds) + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in clouds])
    off[-1] += past
    return off


def _cat(clouds):
    return np.concatenate([np.asarray(c, np.float64).reshape(-1, 3) for c in clouds])


def _evaluate(gpu, srcs, tgts, T, max_dist, plane=False, past=0):
    """one evaluation of P pairs -> list of per-pair dicts"""
    so, to = _offsets(srcs), _offsets(tgts)
    tgt = _cat(tgts)
    nrm = _cu(np.tile([0.0, 0.0, 1.0], (len(tgt), 1))) if plane else None
    out = gpu.icp_pairs(_cu(_cat(srcs)), _cu(_offsets(srcs, past)), _cu(tgt), _cu(_offsets(tgts, past)), _cu(np.asarray(T, np.float64)),
                        max_dist, 0, True, nrm)
    torch.cuda.synchronize()
    r = {k: _np(v) for k, v in out.items() if not k.startswith("_")}
    assert r["T_trace"].shape == (len(srcs), 1, 4, 4) and r["eval_trace"].shape == (len(srcs), 1, 3)
    return [dict(corr=r["corr"][so[p]:so[p + 1]], n_corr=r["eval_trace"][p, 0, 0], sum_d2=r["eval_trace"][p, 0, 1],
                 stop=r["eval_trace"][p, 0, 2], fitness=r["fitness"][p], rmse=r["inlier_rmse"][p], T=r["T"][p], T0=r["T_trace"][p, 0],
                 status=int(r["status"][p]), iterations=int(r["iterations"][p])) for p in range(len(srcs))]


_RUNS = {}


def _run(gpu, name, plane):
    """the geometry's pairs through the device, one call per max_dist, computed once per estimator"""
    if (name, plane) not in _RUNS:
        g = data.geometry(name)
        got = [None] * len(g["srcs"])
        for ps, md in data.calls(name):
            res = _evaluate(gpu, [g["srcs"][p] for p in ps], [g["tgts"][p] for p in ps], g["T"][ps], md, plane)
            for p, r in zip(ps, res):
                got[p] = r
        _RUNS[(name, plane)] = got
    return _RUNS[(name, plane)]


def _check_pair(got, o, ns, nt, T_init, tag):
    """a pair's evaluation against the oracle's, exactly"""
    live = ns > 0 and nt > 0
    assert np.array_equal(got["corr"], o["j"]), (tag, np.flatnonzero(got["corr"] != o["j"])[:8], got["corr"][got["corr"] != o["j"]][:8],
                                                o["j"][got["corr"] != o["j"]][:8])
    assert got["n_corr"] == o["n_corr"], (tag, got["n_corr"], o["n_corr"])
    assert _bits(got["sum_d2"]) == _bits(o["sum_d2"]), (tag, got["sum_d2"], o["sum_d2"])
    fit, rmse = data.implied(o, ns) if live else (0.0, 0.0)
    assert _bits(got["fitness"]) == _bits(fit) and _bits(got["rmse"]) == _bits(rmse), (tag, got["fitness"], fit, got["rmse"], rmse)
    assert _bits(got["T"]) == _bits(T_init) and _bits(got["T0"]) == _bits(T_init), tag
    assert got["iterations"] == 0 and got["status"] == (ICP_MAX_ITER if live else ICP_EMPTY), (tag, got["status"])
    assert got["stop"] == (1.0 if live else 0.0), tag


# ------------------------------------------------------------------ 1. every geometry, both estimators
@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
@pytest.mark.parametrize("name", data.FINITE)
def test_search_equals_the_oracle(gpu, name, plane):
    g = data.geometry(name)
    got = _run(gpu, name, plane)
    for p, o in enumerate(g["oracle"]):
        _check_pair(got[p], o, len(g["srcs"][p]), len(g["tgts"][p]), g["T"][p], (name, p))
    if plane:                                                                 # icp_search_kernel<1> is the same search
        for a, b in zip(got, _run(gpu, name, False)):
            assert np.array_equal(a["corr"], b["corr"]) and all(_bits(a[k]) == _bits(b[k]) for k in ("n_corr", "sum_d2", "fitness", "rmse"))


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_non_finite_rows_are_never_correspondences(gpu, plane):
    """a NaN, +Inf or -Inf in one source row or in one target row: that row is never a correspondence and never counted, every
    other row is the oracle's (whose rule is that a d2 which is not finite never wins)"""
    g = data.geometry("non_finite")
    got = _run(gpu, "non_finite", plane)
    for p, o in enumerate(g["oracle"]):
        if g["bad_src"][p] is not None:
            assert got[p]["corr"][g["bad_src"][p]] == -1
        else:
            assert not (got[p]["corr"] == g["bad_tgt"][p]).any()
        assert np.isfinite([got[p]["sum_d2"], got[p]["fitness"], got[p]["rmse"]]).all()
        _check_pair(got[p], o, len(g["srcs"][p]), len(g["tgts"][p]), g["T"][p], ("non_finite", p))


# ------------------------------------------------------------------ 2. the batch
KEYS = ("n_corr", "sum_d2", "stop", "fitness", "rmse", "T", "T0")


def _same(a, b, tag):
    assert np.array_equal(a["corr"], b["corr"]) and a["status"] == b["status"] and a["iterations"] == b["iterations"], tag
    for k in KEYS:
        assert _bits(a[k]) == _bits(b[k]), (tag, k)


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_batch_equals_its_pairs_alone_and_clipped_offsets(gpu, plane):
    g = data.geometry("batch")
    srcs, tgts, T, md = g["srcs"], g["tgts"], g["T"], g["max_dist"][0]
    whole = _run(gpu, "batch", plane)
    assert [r["status"] for r in whole] == [ICP_MAX_ITER, ICP_EMPTY, ICP_EMPTY, ICP_MAX_ITER, ICP_MAX_ITER, ICP_MAX_ITER]
    for p in range(len(srcs)):
        alone = _evaluate(gpu, srcs[p:p + 1], tgts[p:p + 1], T[p:p + 1], md, plane)[0]
        _same(alone, whole[p], ("alone", p))
    clipped = _evaluate(gpu, srcs, tgts, T, md, plane, past=1000)             # the last offsets 1000 past the capacity
    for p in range(len(srcs)):
        _same(clipped[p], whole[p], ("clipped", p))


# ------------------------------------------------------------------ 3. the kNN search on the same grid
_KNN = {}


def _knn_want(name):
    if name not in _KNN:
        cloud = data.geometry(name)["tgts"][0]
        _KNN[name] = data.knn_exact(cloud, 32)
        if len(cloud) <= 1024:                                                # knn_f64 is brute force there: the yardstick itself
            assert np.array_equal(_KNN[name], knn_f64(cloud, 32)[0])
    return _KNN[name]


@pytest.mark.parametrize("knn", [3, 20, 32])
@pytest.mark.parametrize("name", data.KNN_CLOUDS)
def test_knn_lists_are_exact(gpu, name, knn):
    """(d2, index) is a total order, so the list of knn entries is the head of the list of 32; knn <= 20 and knn > 20 are the two
    template instances of nrm_knn_kernel"""
    cloud = data.geometry(name)["tgts"][0]
    want = _knn_want(name)[:, :knn]
    out = gpu.estimate_normals(_cu(cloud), _cu(np.array([0, len(cloud)], np.int64)), knn, True)
    torch.cuda.synchronize()
    got = _np(out["neighbors"])
    assert _np(out["status"]).tolist() == [0] and got.shape == want.shape
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, (name, knn, len(bad), bad[:5], got[bad[:2]], want[bad[:2]])
    assert (got[:, 0] == np.arange(len(cloud))).sum() >= len(cloud) - 2       # a point is its own first neighbour (but for the duplicates)

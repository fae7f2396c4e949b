"""GPU tests of the NDT layer (run with -m gpu on an MI355X): csrc/ndt.hip and `NDTMap` of egonn_amd/mapping.py against the
numpy restatement tests/ndt_ref.py.  Moments, mean and covariance bit for bit (the wave and tile edges of the run reduction,
absent keys, dropped points, bad picks, batching, a short capacity); eigenvalues, information matrices and the sums of an
evaluation inside bands; the free run on the planted scans; determinism alone / in a batch / replayed from a graph; and the
seams (`build_ndt_map`, `refine_against_map(method="ndt")`, save / load, `Relocalizer(ndt_map=...)`).

Bands (the tests print what they measure and assert the inequalities on the values they measure):
  MEASURED_INFO_HOST   largest difference of an information matrix between the Jacobi-schedule restatement and the eigh-based
                       one, relative to the matrix' largest entry, over the voxels of ndt_ref.finalize_case(), measured on the
                       host.  INFO_TOL must be >= 100 x that and <= 1e-9; the device is held to INFO_TOL against the eigh-based
                       value.
  SUM_TOL              the device's score, A and b of one evaluation against the float64 restatement, relative to the largest
                       entry of A (b: of A and b).  An entry sums at most 7 x 1025 products in another order: n x 2^-53 ~ 8e-13
                       of the sum of their magnitudes in the worst case, and the largest entry is a diagonal one, all of whose
                       terms are positive; exp differs by an ulp or two.  SUM_TOL = 1e-10 was set from that before the first
                       run; it must be >= 100 x MEASURED_SUM and <= 1e-9.
  FREE_TOL             Frobenius distance between the device's final pose and the free-running restatement's on the planted
                       scans; must be >= 10 x MEASURED_FREE and <= 1e-3."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ndt_ref as ref
from tests import voxel_map_ref as vref

pytestmark = pytest.mark.gpu

MEASURED_INFO_HOST = 3.353e-15      # as printed by test_finalize_against_the_restatements (a host figure)
MEASURED_SUM = 3.756e-15            # the largest value printed by test_register_teacher_forced_sums on an MI355X
MEASURED_FREE = 3.115e-15           # the largest value printed by test_free_run_on_the_planted_scans on an MI355X (12 runs)
INFO_TOL = 1e-12
SUM_TOL = 1e-10
FREE_TOL = 1e-6
VOXEL = 0.5
ORIGIN = np.array([0.5, -1.25, 0.125])
EYE = np.eye(4)[None]
FILL = 0x5A5A5A5A
SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)


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


def _c3(v):
    return (ctypes.c_double * 3)(*[float(x) for x in v])


def _scratch(nbytes):
    assert nbytes > 0
    s = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device="cuda")
    assert s.data_ptr() % 256 == 0
    return s


def _bank_of(gpu, pts, off):
    bank = gpu.CloudBank()
    bank.points = _cu(np.asarray(pts, np.float64).reshape(-1, 3))
    bank.host_offsets = [int(v) for v in off]
    return bank


class _Layer:
    """device arrays of a layer over `keys`: zeroed moments (or a pattern), a row of canary behind each"""

    def __init__(self, keys, fill=0):
        n = len(keys)
        self.n, self.rows = n, max(n, 1)
        self.keys = torch.zeros(self.rows, dtype=torch.int64, device="cuda")
        self.keys[:n] = _cu(np.asarray(keys, np.uint64).astype(np.int64))
        self.n_dev = torch.full((), n, dtype=torch.int64, device="cuda")
        self.cnt = torch.full((self.rows + 1,), fill, dtype=torch.int32, device="cuda")
        self.s1 = torch.full((self.rows + 1, 3), fill, dtype=torch.int64, device="cuda")
        self.s2 = torch.full((self.rows + 1, 6), fill, dtype=torch.int64, device="cuda")
        for t in (self.cnt, self.s1, self.s2):
            t[self.rows:] = FILL
        self.missed = torch.zeros((), dtype=torch.int64, device="cuda")
        self.status = torch.zeros((), dtype=torch.int32, device="cuda")

    def get(self):
        torch.cuda.synchronize()
        assert all(bool((t[self.rows:] == FILL).all()) for t in (self.cnt, self.s1, self.s2)), "rows behind the layer were written"
        return {"cnt": _np(self.cnt[:self.n]), "s1": _np(self.s1[:self.n]), "s2": _np(self.s2[:self.n]), "missed": int(self.missed),
                "status": int(self.status)}


def _accumulate(L, pts, off, pick, poses, origin=ORIGIN, voxel=VOXEL, points_capacity=None):
    from egonn_amd import _lib
    lib = _lib.load()
    pts, off = np.asarray(pts, np.float64).reshape(-1, 3), np.asarray(off, np.int64)
    if points_capacity is None:
        points_capacity = int(sum(off[p + 1] - off[p] for p in pick if 0 <= p < len(off) - 1))
    bank, offs, pk, ps = _cu(pts), _cu(off), _cu(np.asarray(pick, np.int32)), _cu(np.asarray(poses, np.float64))
    s = _scratch(lib.egonn_ndt_accumulate_scratch_bytes(points_capacity, len(pick)))
    _lib.call(bank.device, lib.egonn_ndt_accumulate, bank.data_ptr() if len(pts) else None, len(pts), offs.data_ptr(), len(off) - 1,
              pk.data_ptr(), ps.data_ptr(), len(pick), _c3(origin), float(voxel), points_capacity, L.keys.data_ptr(), L.n_dev.data_ptr(),
              L.rows, L.cnt.data_ptr(), L.s1.data_ptr(), L.s2.data_ptr(), L.missed.data_ptr(), L.status.data_ptr(), s.data_ptr(),
              s.numel() * 8)
    torch.cuda.synchronize()
    return L


def _check_accumulate(pts, off, pick, poses, keys=None, origin=ORIGIN, voxel=VOXEL):
    if keys is None:
        keys = vref.integrate(pts, off, pick, poses, origin, voxel)["keys"]
    got = _accumulate(_Layer(keys), pts, off, pick, poses, origin, voxel).get()
    want = ref.accumulate(keys, pts, off, pick, poses, origin, voxel)
    assert got["status"] == want["status"], (got["status"], want["status"])
    assert ref.same(got, want), (got["missed"], want["missed"])
    return want


def _cloud(n, mode, rng):
    """n points around ORIGIN at VOXEL: all in one voxel, own voxel each, or clustered runs of random length"""
    vox = {"one": np.zeros(n, np.int64), "own": np.arange(n), "clustered": np.sort(rng.integers(0, n // 8 + 1, size=n))}[mode]
    p = rng.uniform(0.05, 0.95, size=(n, 3))
    p[:, 0] += vox % 97
    p[:, 1] += vox // 97
    return ORIGIN + VOXEL * p


# ------------------------------------------------------------------ accumulate
@pytest.mark.parametrize("mode", ["one", "own", "clustered"])
def test_accumulate_at_the_wave_and_tile_edges(gpu, mode):
    rng = np.random.default_rng(11)
    for n in SIZES:
        want = _check_accumulate(_cloud(n, mode, rng), [0, n], [0], EYE)
        assert want["cnt"].sum() == n and want["missed"] == 0 and (mode != "one" or len(want["cnt"]) == 1)


def test_accumulate_long_runs_at_every_start(gpu):
    """a 300-point run of one voxel behind `start` points in voxels of their own: it begins inside a wave, on lane 63, on the
    last position of a workgroup, and crosses waves and workgroups"""
    rng = np.random.default_rng(12)
    for start in (0, 1, 63, 200, 255):
        p = rng.uniform(0.05, 0.95, size=(start + 320, 3))
        p[:start, 0] += np.arange(start) + 5
        p[start + 300:, 0] += np.arange(20) + 400
        want = _check_accumulate(ORIGIN + VOXEL * p, [0, len(p)], [0], EYE)
        assert want["cnt"].max() == 300 and len(want["cnt"]) == start + 21


def test_accumulate_rules(gpu):
    bank, off, poses = ref.random_scene()
    pick = [0, 1, 2, 3, 4, 5, 6]
    _check_accumulate(bank, off, pick, poses)
    # keys absent from the layer: missed is exact
    keys = vref.integrate(bank, off, [0, 1], poses[:2], ORIGIN, VOXEL)["keys"]
    want = _check_accumulate(bank, off, [0, 1, 2, 4], poses[[0, 1, 2, 4]], keys=keys)
    assert 0 < want["missed"] < off[3] - off[2] + off[5] - off[4]
    # NaN / inf: RANGE, the other points as if they were absent
    bad = bank[off[0]: off[1]].copy()
    bad[[3, 77], 0], bad[100, 2] = np.nan, np.inf
    keys0 = vref.integrate(bank, off, [0], poses[:1], ORIGIN, VOXEL)["keys"]
    want = _check_accumulate(bad, [0, len(bad)], [0], poses[:1], keys=keys0)
    assert want["status"] == ref.RANGE and want["cnt"].sum() == len(bad) - 3
    # a bad pick, a cloud picked twice, an empty cloud
    want = _check_accumulate(bank, off, [0, 9, 1, -1], poses[[0, 1, 1, 2]], keys=keys)
    assert want["status"] == ref.BAD_INDEX
    want = _check_accumulate(bank, off, [2, 3, 2], poses[[2, 3, 2]])
    assert want["cnt"].sum() == 2 * (off[3] - off[2])
    # a UTM-sized origin
    org = np.array([3e5, 4e6, 50.0])
    far = poses.copy()
    far[:, :3, 3] += org
    _check_accumulate(bank, off, pick, far, origin=org)
    # an empty layer: every valid point is missed
    got = _accumulate(_Layer(np.zeros(0, np.uint64)), bank, off, [0], poses[:1]).get()
    assert got["missed"] == off[1] and got["status"] == 0


@pytest.mark.parametrize("batches", [1, 2, 5])
def test_accumulate_in_batches_and_reversed(gpu, batches):
    bank, off, poses = ref.random_scene()
    pick = np.array([0, 1, 2, 3, 4, 5, 6, 2, 0])
    ps = poses[pick]
    keys = vref.integrate(bank, off, pick, ps, ORIGIN, VOXEL)["keys"]
    one = ref.accumulate(keys, bank, off, pick, ps, ORIGIN, VOXEL)
    for order in (np.arange(len(pick)), np.arange(len(pick))[::-1]):
        L = _Layer(keys)
        for part in np.array_split(order, batches):
            _accumulate(L, bank, off, pick[part], ps[part])
        assert ref.same(L.get(), one)


def test_accumulate_capacity_leaves_the_arrays_untouched(gpu):
    bank, off, poses = ref.random_scene()
    keys = vref.integrate(bank, off, [0, 1], poses[:2], ORIGIN, VOXEL)["keys"]
    L = _accumulate(_Layer(keys, fill=7), bank, off, [0, 1], poses[:2], points_capacity=int(off[2]) - 1)
    got = L.get()
    assert got["status"] == ref.CAPACITY and got["missed"] == 0
    assert (got["cnt"] == 7).all() and (got["s1"] == 7).all() and (got["s2"] == 7).all()
    # the capacity itself is enough
    L = _accumulate(_Layer(keys), bank, off, [0, 1], poses[:2], points_capacity=int(off[2]))
    assert ref.same(L.get(), ref.accumulate(keys, bank, off, [0, 1], poses[:2], ORIGIN, VOXEL))


# ------------------------------------------------------------------ finalize
def _finalize(keys, acc, voxel, min_points=6, min_eig_ratio=0.01):
    from egonn_amd import _lib
    lib = _lib.load()
    n = len(keys)
    L = _Layer(keys)
    L.cnt[:n], L.s1[:n], L.s2[:n] = _cu(acc["cnt"]), _cu(acc["s1"]), _cu(acc["s2"])
    f64 = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device="cuda")        # noqa: E731
    g = {"mean": f64(L.rows + 1, 3), "info": f64(L.rows + 1, 6), "eigenvalues": f64(L.rows + 1, 3), "normal": f64(L.rows + 1, 3),
         "cov": f64(L.rows + 1, 6), "valid": torch.full((L.rows + 1,), 9, dtype=torch.uint8, device="cuda"),
         "n_valid": torch.full((), -5, dtype=torch.int64, device="cuda")}
    _lib.call(L.keys.device, lib.egonn_ndt_finalize, L.keys.data_ptr(), L.n_dev.data_ptr(), L.rows, L.cnt.data_ptr(), L.s1.data_ptr(),
              L.s2.data_ptr(), float(voxel), int(min_points), float(min_eig_ratio), g["mean"].data_ptr(), g["info"].data_ptr(),
              g["eigenvalues"].data_ptr(), g["normal"].data_ptr(), g["valid"].data_ptr(), g["n_valid"].data_ptr(), g["cov"].data_ptr())
    torch.cuda.synchronize()
    for k in ("mean", "info", "eigenvalues", "normal", "cov"):
        assert bool((g[k][n:] == -7.0).all()), k
    assert bool((g["valid"][n:] == 9).all())
    out = {k: _np(v[:n]) for k, v in g.items() if v.dim()}
    out["n_valid"] = int(g["n_valid"])
    return out, g, L


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_finalize_against_the_restatements(gpu):
    c = ref.finalize_case()
    a, keys = c["acc"], c["keys"]
    J = ref.finalize(keys, a["cnt"], a["s1"], a["s2"], c["voxel"])
    E = ref.finalize(keys, a["cnt"], a["s1"], a["s2"], c["voxel"], eig="eigh")
    host = ref.info_rel_diff(J["info"], E["info"])
    print("MEASURED_INFO_HOST =", host)
    assert 100.0 * host <= INFO_TOL <= 1e-9 and 100.0 * MEASURED_INFO_HOST <= INFO_TOL
    dev, _, _ = _finalize(keys, a, c["voxel"])
    assert np.array_equal(_bits(dev["mean"]), _bits(J["mean"])) and np.array_equal(_bits(dev["cov"]), _bits(J["cov"]))
    assert np.array_equal(dev["valid"], J["valid"]) and np.array_equal(dev["valid"], E["valid"]) and dev["n_valid"] == J["n_valid"] > 50
    v = dev["valid"].astype(bool)
    for f in ("mean", "cov", "info", "eigenvalues", "normal"):
        assert not dev[f][~v].any(), f
    assert (np.abs(dev["eigenvalues"] - E["eigenvalues"])[v] <= 1e-12 * E["eigenvalues"][v][:, 2:3]).all()
    assert (np.diff(dev["eigenvalues"], axis=1) >= 0).all()
    d = ref.info_rel_diff(dev["info"], E["info"])
    print("device info against eigh:", d, "against the Jacobi restatement:", ref.info_rel_diff(dev["info"], J["info"]))
    assert d <= INFO_TOL
    # normals: the eigenvector of the smallest eigenvalue where it is separated, the sign rule everywhere
    lam, vec = np.linalg.eigh(ref.full(J["cov"]))
    sep = v & (lam[:, 1] - lam[:, 0] > 1e-3 * lam[:, 2])
    assert sep.sum() > 30 and (np.abs(np.abs((dev["normal"] * vec[:, :, 0]).sum(1)) - 1.0)[sep] <= 1e-9).all()
    lead = np.where(dev["normal"][:, 0] != 0, dev["normal"][:, 0], np.where(dev["normal"][:, 1] != 0, dev["normal"][:, 1], dev["normal"][:, 2]))
    assert (lead[v] > 0).all()
    # the special voxels are the last five keys: plane z, tilted plane, line, one point eight times, five points
    assert dev["valid"][-5:].tolist() == [1, 1, 1, 0, 0]
    assert dev["normal"][-5].tolist() == [0.0, 0.0, 1.0] and dev["eigenvalues"][-5, 0] == 0.0
    assert dev["info"][-5, 5] == 1.0 / (0.01 * dev["eigenvalues"][-5, 2])
    assert np.abs(dev["normal"][-4] - np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)).max() < 1e-9
    assert np.abs(dev["eigenvalues"][-3, :2]).max() <= 1e-12 * dev["eigenvalues"][-3, 2]


def test_finalize_min_points_edge(gpu):
    c = ref.finalize_case()
    a, keys = c["acc"], c["keys"]
    for mp in (5, 6, 7):
        dev, _, _ = _finalize(keys, a, c["voxel"], min_points=mp)
        want = ref.finalize(keys, a["cnt"], a["s1"], a["s2"], c["voxel"], min_points=mp)
        assert np.array_equal(dev["valid"], want["valid"]) and dev["n_valid"] == want["n_valid"]
        assert not dev["valid"][a["cnt"] < mp].any()
    assert (a["cnt"] == 5).any() and (a["cnt"] == 6).any()
    dev, _, _ = _finalize(keys, a, c["voxel"], min_eig_ratio=0.25)
    want = ref.finalize(keys, a["cnt"], a["s1"], a["s2"], c["voxel"], min_eig_ratio=0.25, eig="eigh")
    assert ref.info_rel_diff(dev["info"], want["info"]) <= INFO_TOL


# ------------------------------------------------------------------ register
class _Gauss:
    """a layer's Gaussians on the device, made by the device's own finalize from the restatement's moments"""

    def __init__(self, keys, acc, voxel):
        self.host, self.g, self.L = _finalize(keys, acc, voxel)
        self.keys, self.voxel = np.asarray(keys, np.uint64), voxel
        self.G = {k: self.host[k] for k in ("mean", "info", "valid")}


def _register(M, clouds, T_init, neighbors=1, max_iteration=30, eps_rot=1e-5, eps_trans=1e-4, out=None):
    from egonn_amd import _lib
    lib = _lib.load()
    P, K = len(clouds), max_iteration
    off = np.zeros(P + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in clouds])
    ns = int(off[-1])
    if out is None:
        src = _cu(np.concatenate([np.asarray(c, np.float64).reshape(-1, 3) for c in clouds]).reshape(-1, 3))
        offs, T0 = _cu(off), _cu(np.asarray(T_init, np.float64))
    else:                                                                      # a captured call: no copy, no allocation
        src, offs, T0 = out["_in"]
    f64 = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device="cuda")        # noqa: E731
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device="cuda")            # noqa: E731
    o = out or {"T": f64(P, 4, 4), "fitness": f64(P), "score": f64(P), "iterations": i32(P), "status": i32(P), "T_trace": f64(P, K + 1, 4, 4),
                "eval_trace": f64(P, K + 1, 4), "sums_trace": f64(P, K + 1, 30),
                "scratch": _scratch(lib.egonn_ndt_register_scratch_bytes(ns, P))}
    o["_in"] = (src, offs, T0)
    _lib.call(src.device, lib.egonn_ndt_register, src.data_ptr() if ns else None, ns, offs.data_ptr(), P, T0.data_ptr(), M.L.keys.data_ptr(),
              M.L.n_dev.data_ptr(), M.L.rows, M.g["mean"].data_ptr(), M.g["info"].data_ptr(), M.g["valid"].data_ptr(), float(M.voxel),
              neighbors, K, eps_rot, eps_trans, o["T"].data_ptr(), o["fitness"].data_ptr(), o["score"].data_ptr(),
              o["iterations"].data_ptr(), o["status"].data_ptr(), o["T_trace"].data_ptr(), o["eval_trace"].data_ptr(),
              o["sums_trace"].data_ptr(), o["scratch"].data_ptr(), o["scratch"].numel() * 8)
    return o


def _res(o):
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in o.items() if torch.is_tensor(v) and k != "scratch"}


def _unpack(s30):
    A = np.zeros((6, 6))
    e = 2
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = s30[e]
            e += 1
    return {"n_term": int(s30[0]), "n_pts": int(s30[1]), "A": A, "b": s30[23:29].copy(), "score": float(s30[29])}


_WORST = {"sum": 0.0, "free": 0.0}


def _check_sums(dev, want):
    """one evaluation: the counts exactly, score / A / b inside SUM_TOL of the largest entry"""
    assert (dev["n_term"], dev["n_pts"]) == (want["n_term"], want["n_pts"]), (dev["n_term"], dev["n_pts"], want["n_term"], want["n_pts"])
    big = max(np.abs(want["A"]).max(), 1e-300)
    d = max(np.abs(dev["A"] - want["A"]).max() / big, np.abs(dev["b"] - want["b"]).max() / max(big, np.abs(want["b"]).max()),
            abs(dev["score"] - want["score"]) / max(want["score"], 1e-300)) if want["n_term"] else 0.0
    _WORST["sum"] = max(_WORST["sum"], d)
    assert d <= SUM_TOL and 100.0 * d <= SUM_TOL, d
    return d


@pytest.fixture(scope="module")
def planted(gpu):
    c = ref.planted_case()
    return c, [_Gauss(L["keys"], L["acc"], 1.0) for L in c["layers"]]


@pytest.mark.parametrize("neighbors", [1, 7])
def test_register_teacher_forced_sums(gpu, planted, neighbors):
    """every evaluation of a short run, under the device's own T_k, against the float64 restatement on the device's Gaussians"""
    c, layers = planted
    M, cloud = layers[0], c["clouds"][0]
    for n in (1, 63, 64, 65, 256, 257, 1025):
        src = cloud[7: 7 + n]
        r = _res(_register(M, [src], c["T0"][:1], neighbors, max_iteration=3))
        rounds = int(r["iterations"][0]) + 1
        for k in range(rounds):
            want = ref.evaluate(src, r["T_trace"][0, k], M.keys, M.G, 1.0, neighbors)
            dev = _unpack(r["sums_trace"][0, k])
            _check_sums(dev, want)
            assert r["eval_trace"][0, k, :3].tolist() == [dev["n_term"], dev["n_pts"], dev["score"]]
        assert r["eval_trace"][0, rounds - 1, 3] == 1.0 and not r["eval_trace"][0, rounds:].any()
        assert float(r["fitness"][0]) == _unpack(r["sums_trace"][0, rounds - 1])["n_pts"] / n
    print("MEASURED_SUM so far =", _WORST["sum"])
    assert 100.0 * MEASURED_SUM <= SUM_TOL <= 1e-9


def test_register_faces_and_the_ends_of_the_index_range(gpu):
    """points exactly on voxel faces (the corner of a voxel belongs to it: floor), and a layer whose voxels sit at index -2^20
    and 2^20 - 1: a point one voxel beyond the range has no voxel of its own and still meets its in-range neighbour"""
    rng = np.random.default_rng(21)
    lo, hi = -float(2 ** 20), float(2 ** 20 - 1)
    corners = np.array([[lo, lo, lo], [hi, hi, hi], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    pts = np.concatenate([c + rng.uniform(0.1, 0.9, size=(12, 3)) for c in corners])
    off = np.array([0, len(pts)])
    keys = vref.integrate(pts, off, [0], EYE, (0, 0, 0), 1.0)["keys"]
    acc = ref.accumulate(keys, pts, off, [0], EYE, (0, 0, 0), 1.0)
    assert len(keys) == 5 and acc["missed"] == 0 and acc["status"] == 0
    M = _Gauss(keys, acc, 1.0)
    assert M.host["valid"].tolist() == [1] * 5
    src = np.concatenate([corners, corners + [1.0, 0.0, 0.0], corners + [0.0, 0.0, 1.0], corners - [0.0, 1.0, 0.0],
                          corners + 0.5, [[hi + 1.5, hi + 0.5, hi + 0.5], [lo - 0.5, lo + 0.5, lo + 0.5], [hi + 2.5, hi, hi]],
                          [[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [1e300, 0.0, 0.0]]])
    for nb in (1, 7):
        r = _res(_register(M, [src], EYE, nb, max_iteration=0))
        want = ref.evaluate(src, np.eye(4), M.keys, M.G, 1.0, nb)
        _check_sums(_unpack(r["sums_trace"][0, 0]), want)
        assert want["n_pts"] == (12 if nb == 1 else 27) and int(r["status"][0]) == ref.MAX_ITER
    assert ref.evaluate(src[-6:-3], np.eye(4), M.keys, M.G, 1.0, 7)["n_pts"] == 2, "beyond the range: the neighbour inside counts"
    assert ref.evaluate(src[-6:-3], np.eye(4), M.keys, M.G, 1.0, 1)["n_pts"] == 0


def test_register_stop_rules(gpu, planted):
    c, layers = planted
    M, cloud, T0 = layers[0], c["clouds"][0][:400], c["T0"][0]
    v = np.nonzero(M.host["valid"])[0][0]
    inside = np.tile(M.host["mean"][v] + [0.001, 0.002, -0.001], (8, 1))
    far = cloud + 1e4
    clouds = [cloud, np.zeros((0, 3)), far, inside]
    Ts = np.stack([T0, T0, T0, np.eye(4)])
    r = _res(_register(M, clouds, Ts, 1))
    assert r["status"].tolist()[1:] == [ref.EMPTY, ref.FEW_CORR, ref.SINGULAR] and r["iterations"].tolist()[1:] == [0, 0, 0]
    assert np.array_equal(_bits(r["T"][1:]), _bits(Ts[1:])), "a pair that cannot step returns T_init bit for bit"
    assert r["fitness"].tolist()[1:] == [0.0, 0.0, 1.0] and r["score"][1] == 0.0 and r["score"][2] == 0.0 and 0.9 < r["score"][3] <= 1.0
    assert _unpack(r["sums_trace"][3, 0])["n_term"] == 8
    assert int(r["iterations"][0]) > 0 and int(r["status"][0]) in (0, ref.MAX_ITER)
    # max_iteration = 0: one evaluation, MAX_ITER, T_init
    r0 = _res(_register(M, clouds, Ts, 7, max_iteration=0))
    assert r0["status"].tolist() == [ref.MAX_ITER, ref.EMPTY, ref.MAX_ITER, ref.MAX_ITER] and not r0["iterations"].any()
    assert np.array_equal(_bits(r0["T"]), _bits(Ts))
    want = ref.evaluate(cloud, T0, M.keys, M.G, 1.0, 7)
    assert float(r0["fitness"][0]) == want["n_pts"] / len(cloud) and abs(r0["score"][0] - want["score"] / len(cloud)) <= SUM_TOL


@pytest.mark.parametrize("neighbors", [1, 7])
def test_free_run_on_the_planted_scans(gpu, planted, neighbors):
    c, layers = planted
    for k in range(6):
        want = ref.register(c["clouds"][k], c["T0"][k], layers[k].keys, layers[k].G, 1.0, neighbors)
        r = _res(_register(layers[k], [c["clouds"][k]], c["T0"][k: k + 1], neighbors))
        d = float(np.linalg.norm(r["T"][0] - want["T"]))
        _WORST["free"] = max(_WORST["free"], d)
        d0, d1 = np.linalg.norm(c["T0"][k] - c["T_planted"][k]), np.linalg.norm(r["T"][0] - c["T_planted"][k])
        last = want["steps"][-1] if want.get("steps") else np.zeros(6)
        near = any(abs(np.abs(last[s]).max() / e - 1.0) < 1e-3 for s, e in ((slice(0, 3), 1e-5), (slice(3, 6), 1e-4)))
        print(f"[ndt] neighbors {neighbors} scan {k}: device against the restatement {d:.3e}, {d0:.4f} -> {d1:.4f}, rounds "
              f"{int(r['iterations'][0])} / {want['iterations']}, status {int(r['status'][0])} / {want['status']}")
        assert 10.0 * d <= FREE_TOL and d1 < d0
        if not near:
            assert int(r["iterations"][0]) == want["iterations"] and int(r["status"][0]) == want["status"]
        assert abs(float(r["fitness"][0]) - want["fitness"]) <= 2.0 / len(c["clouds"][k])
    print("MEASURED_FREE candidate =", _WORST["free"])
    assert 10.0 * MEASURED_FREE <= FREE_TOL <= 1e-3


# ------------------------------------------------------------------ determinism and capture
def _capture(lib, _lib, st, fn):
    g = ctypes.c_void_p()
    _lib.check(lib.egonn_graph_begin(st.cuda_stream))
    try:
        fn()
    finally:
        rc = lib.egonn_graph_end(st.cuda_stream, ctypes.byref(g))
    _lib.check(rc)
    return g


KEYS = ("T", "fitness", "score", "iterations", "status", "T_trace", "eval_trace", "sums_trace")


def test_a_pair_has_the_same_bits_alone_and_in_any_batch(gpu, planted):
    c, layers = planted
    M = layers[0]
    a, b, d = c["clouds"][0], c["clouds"][0][100:700], c["clouds"][0][::3]
    Ta, Tb, Td = c["T0"][0], c["T_planted"][0], c["T0"][0] @ ref.vec6_to_T(np.array([0.01, 0, 0.005, 0.1, 0, 0]))
    for nb in (1, 7):
        alone = _res(_register(M, [a], Ta[None], nb))
        again = _res(_register(M, [a], Ta[None], nb))
        first = _res(_register(M, [a, b, d], np.stack([Ta, Tb, Td]), nb))
        last = _res(_register(M, [d, np.zeros((0, 3)), b, a], np.stack([Td, Td, Tb, Ta]), nb))
        for k in KEYS:
            assert np.array_equal(alone[k], again[k], equal_nan=True), k
            assert np.array_equal(alone[k][0], first[k][0], equal_nan=True) and np.array_equal(alone[k][0], last[k][3], equal_nan=True), k
            assert np.array_equal(first[k][1], last[k][2], equal_nan=True) and np.array_equal(first[k][2], last[k][0], equal_nan=True), k
        assert int(alone["iterations"][0]) > 3


def test_edge_sizes_in_one_batch_equal_the_pair_alone(gpu, planted):
    """300, 0, 256, 257 and 1 source points in one batch: an empty pair between two others, exactly one workgroup, one point into a
    second, a single point; each against the same pair run alone, which is also the single-pair batch"""
    c, layers = planted
    M, cloud = layers[0], c["clouds"][0][::3]                                  # every third point: spread over the whole scene
    clouds = [cloud[:300], cloud[:0], cloud[7:263], cloud[7:264], cloud[50:51]]
    assert [len(x) for x in clouds] == [300, 0, 256, 257, 1]
    Ts = np.stack([c["T0"][0]] * 4 + [c["T_planted"][0]])
    for nb in (1, 7):
        a = _res(_register(M, clouds, Ts, nb))
        assert int(a["status"][1]) == ref.EMPTY and (a["iterations"][[0, 2, 3]] >= 1).all()
        for pos in range(len(clouds)):
            one = _res(_register(M, clouds[pos:pos + 1], Ts[pos:pos + 1], nb))
            for k in KEYS:
                assert np.array_equal(one[k][0], a[k][pos], equal_nan=True), (nb, k, pos)


def test_replayed_graph_is_bit_equal_after_the_scratch_was_overwritten(gpu, planted):
    from egonn_amd import _lib
    lib = _lib.load()
    c, layers = planted
    M, clouds = layers[1], [c["clouds"][1], c["clouds"][1][:300]]
    Ts = np.stack([c["T0"][1], c["T0"][1]])
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        o = _register(M, clouds, Ts, 7)
        st.synchronize()
        eager = _res(o)
        g = _capture(lib, _lib, st, lambda: _register(M, clouds, Ts, 7, out=o))
        for rep in range(2):
            for k in KEYS:
                o[k].fill_(-3)
            o["scratch"].fill_(-1)                                             # what a freed scratch holds is anybody's
            _lib.check(lib.egonn_graph_launch(g, st.cuda_stream))
            st.synchronize()
            got = _res(o)
            for k in KEYS:
                assert np.array_equal(got[k], eager[k], equal_nan=True), (rep, k)
    lib.egonn_graph_destroy(g)
    torch.cuda.current_stream().wait_stream(st)


# ------------------------------------------------------------------ the seams
@pytest.fixture(scope="module")
def planted_bank(gpu):
    from tests import tuples_data as D
    raws, planted, gps = D.planted_sequence()
    return gpu.CloudBank().add(raws), planted, gps


def test_python_layer_equals_the_c_calls(gpu, planted, planted_bank):
    """NDTMap over the voxel map of five planted scans: the restatement's keys, moments and Gaussians' validity; register through
    Python equals the restatement's frame handling"""
    c, layers = planted
    bank, pl, gps = planted_bank
    others = c["layers"][0]["others"]
    vm = gpu.VoxelMap(1.0, origin=pl[0, :3, 3]).insert(bank, pl[others], others)
    ndt = gpu.NDTMap(vm).accumulate(bank, pl[others], others)
    vm.insert(bank, pl[:1], [0])                                              # a later insert does not disturb the snapshot
    G = ndt.finalize(debug=True)
    assert ndt.status == 0 and ndt.missed == 0 and ndt.n_voxels == len(G["valid"])
    # the bank's clouds are the device's downsample (fp32 means): the moments are compared through a restatement of them
    pts, off = _np(bank.points[: bank.n_points]), np.asarray(bank.host_offsets, np.int64)
    keys = vref.integrate(pts, off, others, pl[others], pl[0, :3, 3], 1.0)["keys"]
    acc = ref.accumulate(keys, pts, off, others, pl[others], pl[0, :3, 3], 1.0)
    assert np.array_equal(_np(ndt.keys).astype(np.uint64), keys)
    assert ref.same({"cnt": _np(ndt.cnt), "s1": _np(ndt.s1), "s2": _np(ndt.s2), "missed": ndt.missed}, acc)
    want = ref.finalize(keys, acc["cnt"], acc["s1"], acc["s2"], 1.0)
    assert np.array_equal(_np(G["valid"]), want["valid"]) and int(G["n_valid"]) == want["n_valid"] > 150
    assert np.array_equal(_bits(_np(G["mean"])), _bits(want["mean"])) and np.array_equal(_bits(_np(G["cov"])), _bits(want["cov"]))
    # accumulate in two calls, reversed
    two = gpu.NDTMap(gpu.VoxelMap(1.0, origin=pl[0, :3, 3]).insert(bank, pl[others], others))
    two.accumulate(bank, pl[others[3:]], others[3:]).accumulate(bank, pl[others[:3]][::-1].copy(), others[:3][::-1])
    assert torch.equal(two.cnt, ndt.cnt) and torch.equal(two.s1, ndt.s1) and torch.equal(two.s2, ndt.s2)


def test_scan_to_map_ndt_moves_towards_the_planted_pose(gpu, planted_bank, tmp_path):
    """The seam: build_ndt_map of the other five scans at their planted poses, refine_against_map(method="ndt") from the "GPS"
    pose: every scan ends nearer to its planted pose (the condition tests/test_ndt_host.py confirms for the restatement); a
    saved and loaded map registers bit-equal; method="icp" is the call without the argument."""
    bank, pl, gps = planted_bank
    for k in range(6):
        others = [j for j in range(6) if j != k]
        vm = gpu.VoxelMap(1.0, origin=pl[0, :3, 3]).insert(bank, pl[others], others)
        ndt = gpu.NDTMap(vm).accumulate(bank, pl[others], others)
        ndt.finalize()
        for nb in (1, 7):
            r = gpu.refine_against_map(None, bank, [k], gps[k: k + 1], method="ndt", ndt=ndt, neighbors=nb)
            pose = _np(r["poses"])[0]
            d0, d1 = np.linalg.norm(gps[k] - pl[k]), np.linalg.norm(pose - pl[k])
            print(f"[ndt] scan {k} neighbors {nb}: |gps - planted| {d0:.4f}, |ndt - planted| {d1:.4f}, fitness {float(r['fitness'][0]):.3f}, "
                  f"score {float(r['score'][0]):.3f}, rounds {int(r['iterations'][0])}, status {int(r['status'][0])}")
            assert d1 < d0, (k, nb)
        if k == 0:
            path = str(tmp_path / "ndt.npz")
            ndt.save(path)
            back = gpu.NDTMap.load(path)
            assert back.voxel_size == 1.0 and np.array_equal(back.origin, ndt.origin) and back.missed == ndt.missed
            r2 = gpu.refine_against_map(None, bank, [k], gps[k: k + 1], method="ndt", ndt=back, neighbors=7)
            for f in ("poses", "fitness", "score", "iterations", "status"):
                assert torch.equal(r[f], r2[f]), f
            a = gpu.refine_against_map(vm, bank, [k], gps[k: k + 1], half_extent=30.0)
            b = gpu.refine_against_map(vm, bank, [k], gps[k: k + 1], half_extent=30.0, method="icp")
            for f in ("poses", "fitness", "inlier_rmse", "status"):
                assert torch.equal(a[f], b[f]), f
    whole = gpu.build_ndt_map(bank, pl)
    assert whole.voxel_size == 1.0 and whole.missed == 0 and whole.status == 0 and int(whole.gaussians["n_valid"]) > 150
    with pytest.raises(ValueError, match="finalize"):
        gpu.NDTMap(gpu.build_map(bank, pl, 1.0)).register(bank.points[:10], torch.tensor([0, 10]), pl[:1])


def test_relocalizer_with_an_ndt_map(gpu):
    """The scene of the relocalisation refinement test (keypoints with 0.15 m noise bound what RANSAC can reach): the NDT map of
    the three map clouds (2 m voxels: a synthetic scan of 5000 points is sparse) started at the verified winner's pose ends
    nearer to the planted pose.  Without ndt_map the result has no new key."""
    from egonn_amd.synth import planted_scan_pair
    from tests.test_gpu_relocalize import _TableExtractor
    from tests.test_registration_host import planted_pair
    from tests.test_relocalize_host import planted_map_poses
    n = 3
    pairs = [planted_pair(64, 7100 + m, 0.30, 0.15) for m in range(n)]
    qc, mc = [], []
    for i, p in enumerate(pairs):
        R = p[4][:3, :3]
        ypr = (np.arctan2(R[1, 0], R[0, 0]), -np.arcsin(R[2, 0]), np.arctan2(R[2, 1], R[2, 2]))
        s, t, _, _ = planted_scan_pair(60 + i, 5000, translation=p[4][:3, 3], yaw_pitch_roll=ypr)
        qc.append(s)
        mc.append(t)
    poses = planted_map_poses(n)
    km = gpu.KeypointMap(n_k=64, dim=128, global_dim=8)
    km.add({"global": torch.eye(8)[:n], "keypoints": torch.from_numpy(np.stack([p[3] for p in pairs])),
            "descriptors": torch.from_numpy(np.stack([p[1] for p in pairs]))}, poses)
    km.clouds = gpu.CloudBank(crop=(-80, 80, -80, 80, -30.0, None)).add(mc)
    ndt = gpu.build_ndt_map(km.clouds, poses, voxel_size=2.0)
    assert ndt.status == 0 and ndt.missed == 0
    ex = _TableExtractor(np.eye(8, dtype=np.float32)[[0, 1, 2]], np.stack([p[2] for p in pairs]), np.stack([p[0] for p in pairs]))
    ex.rows = [0, 1, 2]
    nn3 = np.array([[1, 0], [1, 2], [2, 0]], np.int32)
    plain = gpu.Relocalizer(ex, km, k=2, ransac_max_it=2000).localize(qc, nn_index=nn3)
    r = gpu.Relocalizer(ex, km, k=2, ransac_max_it=2000, ndt_map=ndt).localize(qc, nn_index=nn3)
    new = {"pose_ndt", "ndt_fitness", "ndt_score", "ndt_iterations", "ndt_status"}
    assert {k for k in r if not k.startswith("_")} - {k for k in plain if not k.startswith("_")} == new
    assert torch.equal(plain["pose"], r["pose"]) and np.array_equal(_np(r["best_index"]), np.arange(n))
    for q in range(n):
        true = poses[q] @ pairs[q][4]
        e0, e1 = np.linalg.norm(_np(r["pose"])[q] - true), np.linalg.norm(_np(r["pose_ndt"])[q] - true)
        print(f"[ndt] relocalizer query {q}: |pose - planted| {e0:.4f}, |pose_ndt - planted| {e1:.4f}, fitness "
              f"{float(r['ndt_fitness'][q]):.3f}, rounds {int(r['ndt_iterations'][q])}, status {int(r['ndt_status'][q])}")
        assert e1 < e0, q
    both = gpu.Relocalizer(ex, km, k=2, ransac_max_it=2000, ndt_map=ndt, refine=True).localize(qc, nn_index=nn3)
    assert torch.equal(both["pose_ndt"], r["pose_ndt"]) and "pose_refined" in both

"""GPU tests of the spectral geometric verification (run with -m gpu on an MI355X): egonn_spectral_verify against the float64
restatement (tests/spectral_ref.py) over every size at which the kernel changes its path (m around the wave and LDS limits,
n_max on both sides of the LDS / slab switch, more pairs than slabs), the exact complete-graph case, the degenerate ends of
the input space, batch / order / run / replay invariance bit for bit, and the Python surface: register_pairs,
verify_candidates, Relocalizer and LoopDetector under method="spectral".  tests/test_spectral_host.py checks, without a GPU,
that no decision compared here sits within 1e-6 of its threshold.

Figures measured on an MI355X (what the tests print; the bound in brackets), device against restatement:
  exact case q = p: |eigenvalue - (m - 1)| at most 2.6e-13 (1e-12, flat);
  size sweep, n_max 128 / 256, 257 pairs each: eigenvalue 3.6e-8 / 4.5e-8 (m * 2^-23 + 1e-9 * eigenvalue: 1.5e-5 at m = 128),
  weights 3.2e-9 / 2.7e-9 (1e-5), T 1.9e-14 / 1.8e-14 in Frobenius norm (1e-9), inlier_rmse 2.0e-14 / 1.7e-14 (1e-9),
  rte 1.5e-14 / 1.6e-14 (1e-9), rre 3.8e-10 / 2.2e-10 degrees (1e-9 + the conditioning of acos), 0 pairs excused;
  register_pairs(method="spectral"), n128_out60 / n256_n2_200: 8 of 8 and 4 of 4 solved, eigenvalue 7.1e-8 / 3.8e-8,
  T 5.4e-15, rte 2.3e-15 / 9.7e-16, rre 3.2e-10 / 2.1e-10 (1e-9); RANSAC on the same pairs: the same inlier counts, all solved;
  60 high-outlier pairs: all solved, eigenvalue 4.6e-8, weights 5.9e-9, T 4.4e-14, rre 1.6e-10, 0 excused."""
import ctypes

import numpy as np
import pytest
import torch

from tests import spectral_ref as ref
from tests.match_data import gather_host
from tests.test_registration_host import (STATUS_BAD_INDEX, STATUS_CLIPPED, STATUS_FEW_CORR, STATUS_NO_MODEL, edge_pairs, pad_batch,
                                          planted_case as registration_case)
from tests.test_relocalize_host import BAD_INDEX, NO_CANDIDATE, PLANTED_K, PLANTED_M, UNVERIFIED, WEAK_OF

pytestmark = pytest.mark.gpu

MARGIN = 1e-6
OUT_KEYS = ("eigenvalue", "score", "weights", "n_seeds", "T", "inliers", "fitness", "inlier_rmse", "correspondence_set", "status",
            "rte", "rre", "success", "repeatability")


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


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _pack(cases, n_max):
    """[(k1, k2, corr, T)] -> dict of padded host arrays"""
    P = len(cases)
    pk = dict(kp1=np.zeros((P, n_max, 3), np.float32), kp2=np.zeros((P, n_max, 3), np.float32),
              corr=np.full((P, n_max, 2), -1, np.int32), n_corr=np.zeros(P, np.int32), n1=np.zeros(P, np.int32),
              n2=np.zeros(P, np.int32), T_gt=np.tile(np.eye(4), (P, 1, 1)))
    for i, (k1, k2, corr, T) in enumerate(cases):
        pk["n1"][i], pk["n2"][i], pk["n_corr"][i] = len(k1), len(k2), len(corr)
        pk["kp1"][i, :len(k1)], pk["kp2"][i, :len(k2)], pk["corr"][i, :len(corr)], pk["T_gt"][i] = k1, k2, corr, T
    return pk


def _run(gpu, pk, **kw):
    r = gpu.spectral_verify(_cu(pk["kp1"]), _cu(pk["kp2"]), _cu(pk["corr"]), _cu(pk["n_corr"]), _cu(pk["n1"]), _cu(pk["n2"]),
                            _cu(pk["T_gt"]), **kw)
    torch.cuda.synchronize()
    return {k: _np(r[k]) for k in OUT_KEYS}


def _same(a, b, i=slice(None), j=slice(None), keys=OUT_KEYS):
    for k in keys:
        assert np.array_equal(_bits(a[k][i]), _bits(b[k][j])), k


class _Worst:
    """the largest differences seen, printed as the measured figures"""

    def __init__(self):
        self.v = dict(eigenvalue=0.0, eigenvalue_bound=0.0, weights=0.0, T=0.0, inlier_rmse=0.0, rte=0.0, rre=0.0, excused=0, pairs=0)

    def up(self, k, x):
        self.v[k] = max(self.v[k], float(x))


def _compare(name, got, p, want, m, n_max, worst):
    """pair p of a device result against the restatement's dict, by the bounds of the contract"""
    assert np.isfinite([got[k][p] for k in ("eigenvalue", "score", "inlier_rmse", "fitness", "rte", "rre", "repeatability")]).all(), name
    assert np.isfinite(got["weights"][p]).all() and np.isfinite(got["T"][p]).all(), name
    lam = want["eigenvalue"]
    bound = m * 2.0 ** -23 + 1e-9 * lam        # M entries in [0, 1] stored as fp32 move by <= 2^-25 each, |dl| <= m max|dM|: 4 x that
    err = abs(got["eigenvalue"][p] - lam)
    worst.up("eigenvalue", err)
    if err > bound:
        worst.up("eigenvalue_bound", err / bound)
    assert err <= bound, (name, got["eigenvalue"][p], lam, bound)
    assert abs(got["score"][p] - want["score"]) <= bound / max(n_max - 1, 1), name
    assert (got["weights"][p, m:] == 0).all(), name
    if want["gap"] > 1.0:
        worst.up("weights", np.abs(got["weights"][p] - want["weights"]).max())
        assert np.abs(got["weights"][p] - want["weights"]).max() <= 1e-5, name
    worst.v["pairs"] += 1
    assert got["status"][p] == want["status"], (name, got["status"][p], want["status"])
    if want["seed_margin"] < MARGIN or want["residual_margin"] < MARGIN:        # a tie: the sets may differ legitimately
        worst.v["excused"] += 1
        return
    assert got["n_seeds"][p] == want["n_seeds"] and got["inliers"][p] == want["inliers"], \
        (name, got["n_seeds"][p], want["n_seeds"], got["inliers"][p], want["inliers"])
    k = want["inliers"]
    assert np.array_equal(got["correspondence_set"][p, :k], want["correspondence_set"]) and (got["correspondence_set"][p, k:] == -1).all(), name
    assert got["fitness"][p] == want["fitness"], name
    worst.up("T", np.linalg.norm(got["T"][p] - want["T"]))
    worst.up("inlier_rmse", abs(got["inlier_rmse"][p] - want["inlier_rmse"]))
    assert np.linalg.norm(got["T"][p] - want["T"]) <= 1e-9 and abs(got["inlier_rmse"][p] - want["inlier_rmse"]) <= 1e-9, name
    worst.up("rte", abs(got["rte"][p] - want["rte"]))
    worst.up("rre", abs(got["rre"][p] - want["rre"]))
    # rre = acos(c), c = (trace - 1) / 2.  Each side sums nine products (|trace| <= 3): 18 operations that round by at most
    # 3 * 2^-53 each, then a halving: 13.5 * 2^-52 per side, 27 * 2^-52 between the two; 32 leaves room for the few ulp by
    # which the two rotations themselves differ (Horn against SVD).  acos magnifies that by 1 / sin(rre), so the bound is 1e-9
    # plus what 32 ulp of c move the angle at the restatement's value: 2.6e-6 degrees at rre = 0, 1.6e-11 at rre = 0.03
    # degrees, where test_register_pairs_spectral_on_planted_cases asks for 1e-9 flat
    c, d = np.cos(np.deg2rad(want["rre"])), 32 * 2.0 ** -52
    rre_tol = 1e-9 + np.rad2deg(np.arccos(np.clip(c - d, -1, 1)) - np.arccos(np.clip(c + d, -1, 1)))
    assert abs(got["rte"][p] - want["rte"]) <= 1e-9 and abs(got["rre"][p] - want["rre"]) <= rre_tol, (name, got["rre"][p], want["rre"])
    assert got["success"][p] == want["success"] and got["repeatability"][p] == want["repeatability"], name


# ------------------------------------------------------------------ 1. sizes
@pytest.mark.parametrize("n_max", [128, 256])
def test_size_sweep_equals_restatement(gpu, n_max):
    """every m of the sweep in one batch of 257 pairs (the cases cycled, so neighbours differ in m), each against the
    restatement; then each case alone (P = 1), three at a time (P = 3) and, where M lives in scratch slabs, 600 pairs on the
    512 slabs: bit-equal to its row of the large batch"""
    cases = [c for c in ref.sweep_cases() if c[1] == n_max]
    want = ref.solved("sweep", ref.sweep_cases)
    order = [i % len(cases) for i in range(257)]
    big = _run(gpu, _pack([cases[i][2:] for i in order], n_max))
    worst = _Worst()
    for p, i in enumerate(order):
        _compare(cases[i][0], big, p, want[cases[i][0]], len(cases[i][4]), n_max, worst)
    print(f"[spectral] sweep n_max={n_max}: {worst.v}")
    assert worst.v["excused"] == 0
    for i, c in enumerate(cases):
        _same(_run(gpu, _pack([c[2:]], n_max)), big, 0, i)
    for lo in range(0, len(cases) - 2, 3):
        trio = [lo + 2, lo, lo + 1]
        _same(_run(gpu, _pack([cases[i][2:] for i in trio], n_max)), big, slice(None), trio)
    if n_max > 128:
        order = [(7 * i + 3) % len(cases) for i in range(600)]
        _same(_run(gpu, _pack([cases[i][2:] for i in order], n_max)), big, slice(None), order)


@pytest.mark.parametrize("n_max,m", [(128, 3), (128, 64), (128, 128), (256, 129), (256, 256)])
def test_identical_sets_are_exact(gpu, n_max, m):
    """q = p, and p under a consistent permutation of both sides: M = 1 - I, eigenvalue = m - 1, uniform weights, T = identity"""
    rng = np.random.default_rng(m)
    p = rng.uniform(-50, 50, (m, 3)).astype(np.float32)
    ident = np.stack([np.arange(m), np.arange(m)], 1).astype(np.int32)
    perm = rng.permutation(m)
    inv = np.argsort(perm)
    got = _run(gpu, _pack([(p, p, ident, np.eye(4)), (p[perm], p, np.stack([np.arange(m), perm], 1).astype(np.int32), np.eye(4)),
                           (p, p[perm], np.stack([np.arange(m), inv], 1).astype(np.int32), np.eye(4))], n_max))
    for i in range(3):
        print(f"[spectral] exact n_max={n_max} m={m} form {i}: |eigenvalue - (m - 1)| = {abs(got['eigenvalue'][i] - (m - 1)):.3e}")
        assert abs(got["eigenvalue"][i] - (m - 1)) <= 1e-12, (i, got["eigenvalue"][i])
        assert np.abs(got["weights"][i, :m] - 1 / np.sqrt(m)).max() <= 1e-15 and (got["weights"][i, m:] == 0).all()
        assert got["n_seeds"][i] == m and got["inliers"][i] == m and got["status"][i] == 0 and got["success"][i] == 1
        assert np.linalg.norm(got["T"][i] - np.eye(4)) <= 1e-12 and got["inlier_rmse"][i] <= 1e-12


# ------------------------------------------------------------------ 2. edges
def test_edge_pairs_through_register_pairs(gpu):
    """the degenerate ends of the registration suite, through the same matching: the operator's outputs equal the restatement's
    on the device's own correspondences"""
    worst = _Worst()
    for name, (f1, f2, k1, k2, T) in edge_pairs().items():
        n_max = max(len(f1), len(f2), 1)
        F1, F2, K1, K2, n1, n2 = pad_batch([(f1, f2, k1, k2)], n_max=n_max)
        r = gpu.register_pairs(_cu(F1), _cu(F2), _cu(K1), _cu(K2), n1=_cu(n1), n2=_cu(n2), T_gt=_cu(T[None]), method="spectral")
        torch.cuda.synchronize()
        assert "best_t" not in r and {"eigenvalue", "score", "weights", "n_seeds", "corr", "n_corr"} <= set(r)
        got = {k: _np(r[k]) for k in OUT_KEYS}
        m = int(r["n_corr"][0])
        want = ref.spectral_f64(k1, k2, _np(r["corr"])[0, :m], n_max, T, gap=True)
        _compare(name, got, 0, want, m, n_max, worst)
        print(f"[spectral] edge {name}: m {m}, eigenvalue {got['eigenvalue'][0]:.4f}, seeds {got['n_seeds'][0]}, "
              f"inliers {got['inliers'][0]}, status {got['status'][0]}")
        if name in ("n_corr_0", "n_corr_1", "n_corr_2"):
            assert got["status"][0] == STATUS_FEW_CORR | STATUS_NO_MODEL and got["inliers"][0] == 0
        if name in ("identical_keypoints", "collinear", "no_accepted_hypothesis"):
            assert got["status"][0] == STATUS_NO_MODEL and got["inliers"][0] == 0 and np.array_equal(got["T"][0], np.eye(4))
        if name in ("n_corr_3", "n1_ne_n2", "duplicate_descriptors"):
            assert got["status"][0] == 0 and got["success"][0] == 1
    assert worst.v["excused"] == 0


def _duplicate_case():
    """64 keypoints, 12 correspondences: the 8 of a sweep pair (4 of them planted) and 4 more that point at targets those
    already use (what the matcher's all-(i, j(i)) fallback produces)"""
    k1, k2, corr, T = ref.sweep_pair(8, 64, seed=3)
    extra = np.stack([np.setdiff1d(np.arange(64), corr[:, 0])[:4], corr[[0, 0, 3, 5], 1]], 1).astype(np.int32)
    both = np.concatenate([corr, extra])
    return k1, k2, both[np.argsort(both[:, 0], kind="stable")], T


def test_duplicated_targets_bad_indices_and_clipped_counts(gpu):
    worst = _Worst()
    dup = _duplicate_case()
    k1, k2, corr, T = ref.sweep_pair(65, 128, seed=4)
    f1, f2, full, Tf = ref.sweep_pair(128, 128, seed=14)
    bad = corr.copy()
    bad[[2, 40], 0], bad[[7, 64], 1] = [-3, 128 + 9], [-1, 2 ** 31 - 1]
    clamped = np.stack([np.clip(bad[:, 0], 0, 127), np.clip(bad[:, 1], 0, 127)], 1).astype(np.int32)
    pk = _pack([dup, (k1, k2, bad, T), (k1, k2, clamped, T), (f1, f2, full, Tf), (k1, k2, corr, T), (k1, k2, corr, T)], 128)
    pk["n1"][3], pk["n_corr"][3] = 128 + 7, 128 + 5          # counts above n_max: clipped to it
    pk["n2"][4] = -2                                         # an empty side: no correspondences
    pk["n_corr"][5] = -4
    got = _run(gpu, pk)
    _compare("duplicated targets", got, 0, ref.spectral_f64(dup[0], dup[1], dup[2], 128, dup[3], gap=True), len(dup[2]), 128, worst)
    assert got["status"][0] == 0 and got["success"][0] == 1
    _compare("bad indices", got, 1, ref.spectral_f64(k1, k2, bad, 128, T, gap=True), 65, 128, worst)
    assert got["status"][1] == STATUS_BAD_INDEX and got["status"][2] == 0
    _same(got, got, 1, 2, [k for k in OUT_KEYS if k != "status"])
    want3 = ref.spectral_f64(f1, f2, full, 128, Tf, gap=True)
    want3["status"] |= STATUS_CLIPPED
    _compare("clipped counts", got, 3, want3, 128, 128, worst)
    for p in (4, 5):
        assert got["status"][p] == STATUS_CLIPPED | STATUS_FEW_CORR | STATUS_NO_MODEL and got["inliers"][p] == 0
        assert got["eigenvalue"][p] == 0 and got["n_seeds"][p] == 0 and not got["weights"][p].any() and np.array_equal(got["T"][p], np.eye(4))
    assert got["repeatability"][4] == 0 and got["fitness"][4] == 0
    assert worst.v["excused"] == 0


def test_nothing_is_read_beyond_the_counts(gpu):
    """NaN keypoints beyond n1 / n2 and wild correspondence rows beyond n_corr change no bit of any output"""
    cases = [ref.sweep_pair(63, 96, seed=5), ref.sweep_pair(3, 96, seed=6), ref.sweep_pair(0, 96, seed=7)]
    pk = _pack(cases, 128)                                   # 96 keypoints per side in rows of 128
    clean = _run(gpu, pk)
    dirty = {k: v.copy() for k, v in pk.items()}
    for i in range(3):
        dirty["kp1"][i, pk["n1"][i]:] = np.nan
        dirty["kp2"][i, pk["n2"][i]:] = np.nan
        dirty["corr"][i, pk["n_corr"][i]:] = [[2 ** 31 - 1, -2 ** 31]]
    got = _run(gpu, dirty)
    _same(got, clean)
    for k in OUT_KEYS:
        assert np.isfinite(got[k].astype(np.float64)).all(), k
    assert clean["status"].tolist() == [0, 0, STATUS_FEW_CORR | STATUS_NO_MODEL] and clean["inliers"][0] >= 32


# ------------------------------------------------------------------ 3. invariance and replay
def _scribble():
    """allocate and fill what the caching allocator hands out next: memory a call has freed since is overwritten"""
    junk = [torch.full((1 << k,), 0x7f, dtype=torch.uint8, device="cuda") for k in range(8, 22)]
    torch.cuda.synchronize()
    return junk


@pytest.mark.parametrize("n_max", [128, 256])
def test_two_runs_and_a_replayed_graph_are_bit_equal(gpu, n_max):
    from egonn_amd import _lib
    lib = _lib.load()
    m_a, m_b = (100, 64) if n_max == 128 else (200, 129)
    a = _pack([ref.sweep_pair(m_a, n_max, seed=8), ref.sweep_pair(m_b, n_max, seed=9), ref.sweep_pair(5, n_max, seed=10)], n_max)
    b = _pack([ref.sweep_pair(m_b, n_max, seed=11), ref.sweep_pair(2, n_max, seed=12), ref.sweep_pair(m_a, n_max, seed=13)], n_max)
    first, again, want_b = _run(gpu, a), _run(gpu, a), _run(gpu, b)
    _same(first, again)
    names = ("kp1", "kp2", "corr", "n_corr", "n1", "n2", "T_gt")
    dev = {k: _cu(a[k]) for k in names}
    args = lambda: (dev["kp1"], dev["kp2"], dev["corr"], dev["n_corr"], dev["n1"], dev["n2"], dev["T_gt"])      # noqa: E731
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        out = gpu.spectral_verify(*args())                   # eager once: every buffer exists now
        st.synchronize()
        g = ctypes.c_void_p()
        _lib.check(lib.egonn_graph_begin(st.cuda_stream))
        try:
            gpu.spectral_verify(*args(), out=out)
        finally:
            rc = lib.egonn_graph_end(st.cuda_stream, ctypes.byref(g))
        _lib.check(rc)
        junk = _scribble()
        for k in OUT_KEYS:
            out[k].fill_(-3)
        _lib.check(lib.egonn_graph_launch(g, st.cuda_stream))
        st.synchronize()
        _same({k: _np(out[k]) for k in OUT_KEYS}, first)
        for k in names:                                      # the caller's tensors changed in place
            dev[k].copy_(_cu(b[k]))
        for k in OUT_KEYS:
            out[k].fill_(-3)
        _lib.check(lib.egonn_graph_launch(g, st.cuda_stream))
        st.synchronize()
        replay = {k: _np(out[k]).copy() for k in OUT_KEYS}
        with pytest.raises(ValueError, match="other shapes"):
            gpu.spectral_verify(dev["kp1"][:2], dev["kp2"][:2], dev["corr"][:2], dev["n_corr"][:2], out=out)
    lib.egonn_graph_destroy(g)
    torch.cuda.current_stream().wait_stream(st)
    _same(replay, want_b)
    del junk


# ------------------------------------------------------------------ 4. the Python surface
@pytest.mark.parametrize("name", ["n128_out60", "n256_n2_200"])
def test_register_pairs_spectral_on_planted_cases(gpu, name):
    from tests.test_registration_host import PLANTED_CASES
    pairs = registration_case(name)
    want = ref.solved("registration", ref.planted_registration_cases)
    n_max = PLANTED_CASES[name]["n"]
    F1, F2, K1, K2, n1, n2 = pad_batch([p[:4] for p in pairs], n_max=n_max)
    T = np.stack([p[4] for p in pairs])
    dev = [_cu(x) for x in (F1, F2, K1, K2)]
    r = gpu.register_pairs(*dev, n1=_cu(n1), n2=_cu(n2), T_gt=_cu(T), method="spectral", ransac_max_it=1, seed=99, pair_ids=_cu(n1))
    old = gpu.register_pairs(*dev, n1=_cu(n1), n2=_cu(n2), T_gt=_cu(T), ransac_max_it=PLANTED_CASES[name]["H"])
    torch.cuda.synchronize()
    got = {k: _np(r[k]) for k in OUT_KEYS}
    worst = _Worst()
    restated = ref.planted_registration_cases((name,))
    for p in range(len(pairs)):
        w = want[f"{name}[{p}]"]
        m = int(r["n_corr"][p])
        assert np.array_equal(_np(r["corr"])[p, :m], restated[p][4])                                    # the restated matching
        _compare(f"{name}[{p}]", got, p, w, m, n_max, worst)
        assert got["success"][p] == w["success"] == 1 and abs(got["rre"][p] - w["rre"]) <= 1e-9 and abs(got["rte"][p] - w["rte"]) <= 1e-9
        print(f"[spectral] {name}[{p}]: spectral inliers {got['inliers'][p]} rte {got['rte'][p]:.4f} rre {got['rre'][p]:.4f} "
              f"eigenvalue {got['eigenvalue'][p]:.2f} | ransac inliers {int(old['inliers'][p])} rte {float(old['rte'][p]):.4f} "
              f"rre {float(old['rre'][p]):.4f} success {int(old['success'][p])}")
    print(f"[spectral] {name}: {worst.v}")
    assert worst.v["excused"] == 0


def _planted_reloc(gpu, utm):
    from tests.test_gpu_relocalize import _kmap, _planted_inputs
    c, poses, T_gt = _planted_inputs(utm)
    return c, poses, T_gt, _kmap(gpu, c, poses)


@pytest.mark.parametrize("utm", [False, True])
def test_verify_candidates_spectral(gpu, utm):
    from tests.test_gpu_relocalize import _check_pick
    c, poses, T_gt, km = _planted_reloc(gpu, utm)
    M = PLANTED_M + 1
    qid = _cu(np.arange(PLANTED_M, dtype=np.int32))
    r = gpu.verify_candidates(_cu(c["q_feat"]), _cu(c["q_kp"]), None, km, _cu(c["nn"]), query_ids=qid, T_gt=_cu(T_gt), method="spectral")
    torch.cuda.synchronize()
    r = {k: _np(v) for k, v in r.items() if not k.startswith("_")}
    assert "best_t" not in r and r["weights"].shape == (PLANTED_M, PLANTED_K, 64) and r["eigenvalue"].shape == (PLANTED_M, PLANTED_K)
    # recall@1 = 1 after the rerank: the true entry first, the weak twin second, the pose the restated product
    assert np.array_equal(r["reranked"][:, 0], c["truth"]) and r["reranked"][WEAK_OF, 1] == PLANTED_M and (r["status"] == 0).all()
    assert np.array_equal(r["best_index"], np.arange(PLANTED_M)) and (r["best_success"] == 1).all()
    _check_pick(r, c["nn"], M, poses)
    want = {k: ref.spectral_f64(*v[:3], 64, v[3]) for k, v in ref.planted_relocalization_cases().items()}
    for q in range(PLANTED_M):
        col = int(np.nonzero(c["nn"][q] == q)[0][0])
        assert r["inliers"][q, col] == want[(q, q)]["inliers"] and r["n_seeds"][q, col] == want[(q, q)]["n_seeds"], q
        assert np.linalg.norm(r["T"][q, col] - want[(q, q)]["T"]) <= 1e-9
        assert r["score"][q, col] == r["score"][q].max()
        assert abs(r["eigenvalue"][q, col] - want[(q, q)]["eigenvalue"]) <= 64 * 2.0 ** -23 + 1e-9 * want[(q, q)]["eigenvalue"]
    print(f"[spectral] planted relocalisation (utm={utm}): eigenvalues per query\n{np.round(r['eigenvalue'], 2)}\ninliers\n{r['inliers']}")
    # invalid candidates, and every pair against spectral_verify's own path on host-gathered operands
    nn = c["nn"].copy()
    nn[5, 3], nn[4, 1], nn[1] = -1, 99, [-1, -5, 7, -1]
    gt = T_gt.copy()
    gt[(nn < 0) | (nn >= M)] = np.eye(4)
    out = gpu.verify_candidates(_cu(c["q_feat"]), _cu(c["q_kp"]), None, km, _cu(nn), query_ids=qid, T_gt=_cu(gt), method="spectral",
                                min_inliers=5)
    torch.cuda.synchronize()
    v = {k: _np(x) for k, x in out.items() if not k.startswith("_")}
    n64 = np.full(PLANTED_M, 64, np.int32)
    F1, F2, K1, K2, n1, n2 = gather_host(c["q_feat"], c["q_kp"], n64, c["map_feat"], c["map_kp"], np.full(M, 64, np.int32), nn)
    w = gpu.register_pairs(_cu(F1), _cu(F2), _cu(K1), _cu(K2), n1=_cu(n1), n2=_cu(n2), T_gt=_cu(gt.reshape(-1, 4, 4)), method="spectral")
    torch.cuda.synchronize()
    for mine, theirs in (("T", "T"), ("inliers", "inliers"), ("fitness", "fitness"), ("inlier_rmse", "inlier_rmse"),
                         ("pair_status", "status"), ("corr", "corr"), ("n_corr", "n_corr"), ("rte", "rte"), ("rre", "rre"),
                         ("success", "success"), ("eigenvalue", "eigenvalue"), ("score", "score"), ("weights", "weights"),
                         ("n_seeds", "n_seeds")):
        assert np.array_equal(_bits(v[mine]), _bits(_np(w[theirs]).reshape(v[mine].shape))), mine
    _check_pick(v, nn, M, poses, min_inliers=5)
    assert v["status"][1] == NO_CANDIDATE | BAD_INDEX | UNVERIFIED and v["best_index"][1] == -1 and (v["reranked"][1] == -1).all()
    assert v["status"][5] == NO_CANDIDATE and v["status"][4] == NO_CANDIDATE | BAD_INDEX and v["best_index"][4] == 4
    assert (v["best_index"][[0, 2, 3, 5]] == [0, 2, 3, 5]).all() and (v["eigenvalue"][1] == 0).all() and (v["inliers"][1] == 0).all()
    # an `out` of one method is refused for the other
    with pytest.raises(ValueError, match="other method"):
        gpu.verify_candidates(_cu(c["q_feat"]), _cu(c["q_kp"]), None, km, _cu(nn), query_ids=qid, T_gt=_cu(gt), out=out)
    ransac = gpu.verify_candidates(_cu(c["q_feat"]), _cu(c["q_kp"]), None, km, _cu(nn), query_ids=qid, T_gt=_cu(gt), ransac_max_it=64)
    with pytest.raises(ValueError, match="other method"):
        gpu.verify_candidates(_cu(c["q_feat"]), _cu(c["q_kp"]), None, km, _cu(nn), query_ids=qid, T_gt=_cu(gt), out=ransac,
                              method="spectral")
    torch.cuda.synchronize()


def test_relocalizer_and_loop_detector_end_to_end(gpu):
    from tests.test_gpu_loop_closure import FIRST, SECOND, _detector, _trajectory
    from tests.test_gpu_relocalize import _TableExtractor
    from tests.test_registration_host import metrics_f64
    c, poses, T_gt, km = _planted_reloc(gpu, False)
    glob = np.zeros((PLANTED_M, 8), np.float32)               # global descriptors that retrieve exactly the planted lists
    for q in range(PLANTED_M):
        glob[q, c["nn"][q]] = [0.9, 0.8, 0.7, 0.6]
    reloc = gpu.Relocalizer(_TableExtractor(glob, c["q_kp"], c["q_feat"]), km, k=PLANTED_K, method="spectral")
    r = reloc.localize(list(range(PLANTED_M)))
    assert np.array_equal(_np(r["nn_index"]), c["nn"]) and np.array_equal(_np(r["best_index"]), np.arange(PLANTED_M))
    assert "eigenvalue" in r and "best_t" not in r
    for q in range(PLANTED_M):
        assert metrics_f64(_np(r["pose"])[q], poses[q] @ c["T_planted"][q])[2] == 1, q
    out, times, tposes, T = _trajectory()
    d = _detector(gpu, verify_method="spectral").detect(out, times, tposes)
    torch.cuda.synchronize()
    d = {k: _np(v) for k, v in d.items() if not k.startswith("_")}
    for p, j in enumerate(SECOND):
        assert d["loop"][j] and d["best_index"][j] == FIRST[p], (j, d["best_index"][j])
        assert metrics_f64(d["T_rel"][j], T[j])[2] == 1, j
    lone = [j for j in range(20, len(times)) if j not in SECOND]
    print(f"[spectral] loop closure: eigenvalue of the revisits' winners "
          f"{np.round(d['eigenvalue'][SECOND].max(1), 2).tolist()}, largest of the other scans {np.round(d['eigenvalue'][lone].max(), 2)}; "
          f"inliers {d['best_inliers'][SECOND].tolist()} against {d['best_inliers'][lone].tolist()}")


def test_high_outlier_ratios_on_the_device(gpu):
    """5, 8 and 13 planted inliers among 128 correspondences, 20 seeds each, in one batch: solved as by the restatement"""
    cases = ref.high_outlier_cases()
    want = ref.solved("high", ref.high_outlier_cases)
    got = _run(gpu, _pack([c[2:6] for c in cases], 128))
    worst = _Worst()
    for p, c in enumerate(cases):
        _compare(c[0], got, p, want[c[0]], 128, 128, worst)
        assert got["success"][p] == want[c[0]]["success"] == 1, c[0]
    print(f"[spectral] high outlier ratios, {len(cases)} pairs: {worst.v}; eigenvalues "
          f"{[round(float(got['eigenvalue'][[p for p, c in enumerate(cases) if c[0].startswith(f'in{n}_')]].mean()), 2) for n in ref.HIGH_OUTLIER]}")
    assert worst.v["excused"] == 0 and int(got["success"].sum()) == len(cases)

"""CPU tests of the keypoint-set registration (egonn_match_mutual / egonn_ransac_pairs / egonn_registration_finish) and the
home of its float64 restatement, which tests/test_gpu_registration.py imports.

Restated contract (egonn_amd/csrc/match.hip, egonn_amd/csrc/registration.hip; the reference delegates to Open3D,
eval/evaluate.py:381-399 [recall]):
  correspondences  d2[i][j] = |a_i - b_j|^2 in float64; j(i) = argmin_j, i(j) = argmin_i, ties lowest index; keep (i, j(i))
                   iff i(j(i)) == i; fewer than 3 kept -> every (i, j(i)); ascending i.
  draw             splitmix64 of (seed, pair id, t, slot), multiply-high onto [0, n_corr)            (draw() below)
  hypothesis t     3 draws; -1 if two coincide or a triangle has |e1 x e2|^2 <= 1e-6 |e1|^2 |e2|^2; -2 unless every edge has
                   ls^2 >= 0.64 lt^2 and lt^2 >= 0.64 ls^2; Kabsch (np.linalg.svd, reflection corrected) of the 3 pairs; -3 if a
                   sample residual > dist_th; else inliers = #{|T s - t| < dist_th} over all correspondences, err2 = sum d^2.
  best             most inliers, then smallest err2, then lowest t; none with an inlier -> identity, status NO_MODEL.
  final            every source keypoint under T, nearest target keypoint (lowest index) closer than dist_th.
  metrics          rte, rre (degrees), success = rte <= 2 and rre <= 5, repeatability under T_gt (float64).
The device computes the 3-point transform in closed form (plane frames + 2 x 2 polar factor); the SVD here is an independent
route to the same least-squares rotation."""
import os
import re

import numpy as np
import pytest
import torch

from egonn_amd.synth import pad_keypoint_pairs as pad_batch, planted_keypoint_pair as planted_pair, rot_zyx

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = (1 << 64) - 1
STATUS_CLIPPED, STATUS_FEW_CORR, STATUS_NO_MODEL, STATUS_BAD_INDEX = 1, 2, 4, 8
NEW_SYMBOLS = ["egonn_match_mutual_scratch_bytes", "egonn_match_mutual", "egonn_ransac_pairs", "egonn_registration_finish",
               "egonn_registration_scratch_bytes"]

# Hypotheses within BAND of a decision threshold are excused from the per-hypothesis parity of the GPU test.  The issue
# asks for a band >= 100 x the largest measured difference between the device's and this restatement's transformed
# coordinates and <= 1e-6 m; the measurement is recorded in tests/test_gpu_registration.py.  The geometry checks that
# read only input coordinates (edge lengths, triangle degeneracy) compare squared lengths, whose two evaluations differ by
# float64 rounding of centred coordinates (relative ~1e-15): the same number is used as a relative band there.
BAND = 1e-9


# ------------------------------------------------------------------ restatement
def match_f64(f1, f2):
    """-> corr (n_corr, 2) int32, gap (n1,), gap2 (n2,): best-vs-second-best squared-distance gaps of the row / column searches"""
    a, b = np.asarray(f1, dtype=np.float64), np.asarray(f2, dtype=np.float64)
    n1, n2 = len(a), len(b)
    if n1 == 0 or n2 == 0:
        return np.zeros((0, 2), np.int32), np.zeros(n1), np.zeros(n2)
    d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    j_of_i, i_of_j = d2.argmin(1), d2.argmin(0)                 # numpy argmin: first (lowest) index on ties

    def gap(m):
        if m.shape[1] < 2:
            return np.full(m.shape[0], np.inf)
        s = np.sort(m, axis=1)
        return s[:, 1] - s[:, 0]
    mutual = i_of_j[j_of_i] == np.arange(n1)
    keep = mutual if mutual.sum() >= 3 else np.ones(n1, bool)
    i = np.nonzero(keep)[0]
    return np.stack([i, j_of_i[i]], 1).astype(np.int32), gap(d2), gap(d2.T)


def match_band(f1, f2):
    """Two float64 evaluations of d2 = sum of D squares differ by at most 2 x (D + 1) u S with u = 2^-53 and S the largest
    possible d2, (|a|_max + |b|_max)^2 (standard bound (n + 1) u sum|terms| per evaluation, the subtraction included;
    the conversions from fp32 are exact).  For unit descriptors, D = 128: 2 * 129 * 2^-53 * 4 = 1.1e-13, ~500 ulp of 1.0."""
    a, b = np.asarray(f1, dtype=np.float64), np.asarray(f2, dtype=np.float64)
    if len(a) == 0 or len(b) == 0:
        return 0.0
    s = (np.linalg.norm(a, axis=1).max() + np.linalg.norm(b, axis=1).max()) ** 2
    return 2.0 * (a.shape[1] + 1) * 2.0 ** -53 * s


def draw(seed, pair_id, t, slot, n):
    """the integer draw, bit for bit (t may be an array)"""
    t = np.asarray(t, dtype=np.uint64)
    ctr = (np.uint64(pair_id) << np.uint64(34)) | (t << np.uint64(2)) | np.uint64(slot)
    with np.errstate(over="ignore"):
        z = np.uint64(seed & MASK) + np.uint64(0x9E3779B97F4A7C15) * (ctr + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (((z >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def draw_scalar(seed, pair_id, t, slot, n):
    """the same function in Python integers (cross-check of the numpy wrap-around)"""
    ctr = (pair_id << 34) | (t << 2) | slot
    z = (seed + 0x9E3779B97F4A7C15 * (ctr + 1)) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return ((z >> 32) * n) >> 32


def centred(k1, k2, corr):
    """centred correspondence coordinates: sums in ascending order (np.cumsum is sequential)"""
    s = np.asarray(k1, dtype=np.float64)[corr[:, 0]]
    q = np.asarray(k2, dtype=np.float64)[corr[:, 1]]
    cs, cq = np.cumsum(s, 0)[-1] / len(s), np.cumsum(q, 0)[-1] / len(q)
    return s - cs, q - cq, cs, cq


def kabsch(S, Q):
    """(..., m, 3) point sets -> R (..., 3, 3), t (..., 3) minimising sum |R s + t - q|^2, det R = +1"""
    cs, cq = S.mean(-2, keepdims=True), Q.mean(-2, keepdims=True)
    Hm = np.swapaxes(S - cs, -1, -2) @ (Q - cq)
    U, _, Vt = np.linalg.svd(Hm)
    d = np.sign(np.linalg.det(np.swapaxes(Vt, -1, -2) @ np.swapaxes(U, -1, -2)))
    D = np.zeros(Hm.shape)
    D[..., 0, 0] = D[..., 1, 1] = 1.0
    D[..., 2, 2] = d
    R = np.swapaxes(Vt, -1, -2) @ D @ np.swapaxes(U, -1, -2)
    t = cq[..., 0, :] - (R @ cs[..., 0, :, None])[..., 0]
    return R, t


def _near(a, b, rel):
    return np.abs(a - b) < rel * np.maximum(np.abs(a), np.abs(b))       # strict: 0 against 0 is exact on both sides


def ransac_f64(k1, k2, corr, seed, pair_id, H, dist_th=0.5, band=BAND):
    """per-hypothesis table of one pair: count (H,) int32, err2 (H,), near (H,) bool, R (H,3,3), t (H,3) in the CALLER's
    coordinates (identity where not accepted)"""
    count = np.full(H, -1, np.int32)
    err2 = np.zeros(H)
    near = np.zeros(H, bool)
    R_all = np.tile(np.eye(3), (H, 1, 1))
    t_all = np.zeros((H, 3))
    nc = len(corr)
    if nc < 3:
        return dict(count=count, err2=err2, near=near, R=R_all, t=t_all)
    s, q, cs, cq = centred(k1, k2, corr)
    th2 = dist_th * dist_th
    tt = np.arange(H)
    idx = np.stack([draw(seed, pair_id, tt, k, nc) for k in range(3)], 1)
    ok = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2])
    S, Q = s[idx], q[idx]                                          # (H,3,3)

    def tri(P3):
        e1, e2, e3 = P3[:, 1] - P3[:, 0], P3[:, 2] - P3[:, 0], P3[:, 2] - P3[:, 1]
        n = np.cross(e1, e2)
        return (n * n).sum(1), (e1 * e1).sum(1), (e2 * e2).sum(1), (e3 * e3).sum(1)
    ns2, a1, a2, a3 = tri(S)
    nt2, b1, b2, b3 = tri(Q)
    nondeg = (ns2 > 1e-6 * a1 * a2) & (nt2 > 1e-6 * b1 * b2)
    near |= ok & (_near(ns2, 1e-6 * a1 * a2, band) | _near(nt2, 1e-6 * b1 * b2, band))
    ok &= nondeg
    edge = np.ones(H, bool)
    for ls, lt in ((a1, b1), (a2, b2), (a3, b3)):
        edge &= (ls >= 0.64 * lt) & (lt >= 0.64 * ls)
        near |= ok & (_near(ls, 0.64 * lt, band) | _near(lt, 0.64 * ls, band))
    count[ok & ~edge] = -2
    ok &= edge
    h = np.nonzero(ok)[0]
    if len(h) == 0:
        return dict(count=count, err2=err2, near=near, R=R_all, t=t_all)
    R, t = kabsch(S[h], Q[h])
    res = np.einsum("hij,hkj->hki", R, S[h]) + t[:, None, :] - Q[h]
    r2 = (res * res).sum(-1)                                       # (h,3)
    dband = 2.0 * dist_th * band                                   # |d - th| <= band  <=>  |d^2 - th^2| <= 2 th band
    near[h] |= (np.abs(r2 - th2) <= dband).any(1)
    passed = (r2 <= th2).all(1)
    count[h[~passed]] = -3
    h, R, t = h[passed], R[passed], t[passed]
    for lo in range(0, len(h), 512):
        hh, Rc, tc = h[lo:lo + 512], R[lo:lo + 512], t[lo:lo + 512]
        d2 = ((np.einsum("hij,cj->hci", Rc, s) + tc[:, None, :] - q[None]) ** 2).sum(-1)     # (h, nc)
        inl = d2 < th2
        count[hh] = inl.sum(1)
        err2[hh] = np.where(inl, d2, 0.0).sum(1)
        near[hh] |= (np.abs(d2 - th2) <= dband).any(1)
    R_all[h] = R
    t_all[h] = cq + t - (R @ cs[:, None])[..., 0]
    return dict(count=count, err2=err2, near=near, R=R_all, t=t_all)


def hypothesis_transform_f64(k1, k2, corr, seed, pair_id, t):
    """R (3,3), t (3,) of hypothesis t alone, in the caller's coordinates (SVD Kabsch of its three drawn pairs; no checks)"""
    s, q, cs, cq = centred(k1, k2, corr)
    idx = [int(draw(seed, pair_id, t, k, len(corr))) for k in range(3)]
    R, tv = kabsch(s[idx], q[idx])
    return R, cq + tv - R @ cs


def best_rule(count, err2):
    """argbest (most inliers, smallest err2, lowest t) of a table; -1 when no hypothesis has an inlier"""
    c = np.asarray(count)
    if len(c) == 0 or c.max() <= 0:
        return -1
    cand = np.nonzero(c == c.max())[0]
    e = np.asarray(err2)[cand]
    return int(cand[np.nonzero(e == e.min())[0][0]])


def final_eval(k1, k2, T, dist_th=0.5):
    """-> inliers, fitness, rmse, correspondence set (inliers, 2)"""
    a, b = np.asarray(k1, dtype=np.float64), np.asarray(k2, dtype=np.float64)
    if len(a) == 0 or len(b) == 0:
        return 0, 0.0, 0.0, np.zeros((0, 2), np.int32)
    p = a @ T[:3, :3].T + T[:3, 3]
    d2 = ((p[:, None, :] - b[None]) ** 2).sum(-1)
    nn = d2.argmin(1)
    m = d2[np.arange(len(a)), nn]
    inl = m < dist_th * dist_th
    k = int(inl.sum())
    return k, k / len(a), (float(np.sqrt(m[inl].sum() / k)) if k else 0.0), np.stack([np.nonzero(inl)[0], nn[inl]], 1).astype(np.int32)


def repeatability_f64(k1, k2, T, threshold):
    a, b = np.asarray(k1, dtype=np.float64), np.asarray(k2, dtype=np.float64)
    if len(a) == 0:
        return 0.0
    if len(b) == 0:
        return 0.0
    p = a @ T[:3, :3].T + T[:3, 3]
    d2 = ((p[:, None, :] - b[None]) ** 2).sum(-1).min(1)
    return float((d2 <= threshold * threshold).mean())


def metrics_f64(T, T_gt):
    rte = float(np.linalg.norm(T[:3, 3] - T_gt[:3, 3]))
    c = (np.trace(T[:3, :3].T @ T_gt[:3, :3]) - 1.0) / 2.0
    rre = float(np.arccos(np.clip(c, -1.0, 1.0)) * 180.0 / np.pi)
    return rte, rre, int(not (rte > 2.0 or rre > 5.0))


def register_f64(f1, f2, k1, k2, T_gt=None, seed=0, pair_id=0, H=10000, dist_th=0.5, repeat_th=0.5):
    corr, _, _ = match_f64(f1, f2)
    tab = ransac_f64(k1, k2, corr, seed, pair_id, H, dist_th)
    bt = best_rule(tab["count"], tab["err2"])
    T = np.eye(4)
    status = (STATUS_FEW_CORR if len(corr) < 3 else 0) | (STATUS_NO_MODEL if bt < 0 else 0)
    if bt >= 0:
        T[:3, :3], T[:3, 3] = tab["R"][bt], tab["t"][bt]
    inl, fit, rmse, cset = final_eval(k1, k2, T, dist_th) if bt >= 0 else (0, 0.0, 0.0, np.zeros((0, 2), np.int32))
    out = dict(corr=corr, table=tab, best_t=bt, T=T, inliers=inl, fitness=fit, inlier_rmse=rmse, correspondence_set=cset,
               status=status)
    if T_gt is not None:
        out["rte"], out["rre"], out["success"] = metrics_f64(T, T_gt)
        out["repeatability"] = repeatability_f64(k1, k2, T_gt, repeat_th)
    return out


# ------------------------------------------------------------------ seeded cases
# name -> (n keypoints, first seed, pairs, outlier share, position noise [m], hypotheses).  Every pair of every case is solved
# by the restatement under the reference's success rule (checked below, on the CPU).
PLANTED_CASES = {
    "n128_out30": dict(n=128, seed=100, pairs=8, outliers=0.30, noise=0.05, H=10000),
    "n128_out60": dict(n=128, seed=200, pairs=8, outliers=0.60, noise=0.05, H=10000),
    "n256_out50": dict(n=256, seed=300, pairs=8, outliers=0.50, noise=0.08, H=10000),
    "n256_n2_200": dict(n=256, seed=400, pairs=4, outliers=0.40, noise=0.05, H=4000, n2=200),
}


def planted_case(name):
    c = PLANTED_CASES[name]
    return [planted_pair(c["n"], c["seed"] + i, c["outliers"], c["noise"], n2=c.get("n2")) for i in range(c["pairs"])]


def edge_pairs():
    """name -> (f1, f2, k1, k2, T_gt): the degenerate ends of the input space"""
    out = {}
    f1, f2, k1, k2, T = planted_pair(64, 900, 0.0, noise=0.0)
    for m in (0, 1, 2, 3):
        out[f"n_corr_{m}"] = (f1[:m], f2, k1[:m], k2, T)
    out["identical_keypoints"] = (f1, f2, np.ones_like(k1), np.ones_like(k2) * 2, T)
    line = np.linspace(-50, 50, 64, dtype=np.float32)[:, None] * np.array([[1.0, 0.5, 0.1]], np.float32)
    out["collinear"] = (f1, f1.copy(), line, line + np.float32(1.0), T)
    out["n1_ne_n2"] = planted_pair(128, 901, 0.3, n2=100)
    out["no_accepted_hypothesis"] = (f1, f1.copy(), k1, k1 * np.float32(2.0), T)      # every edge doubles: the edge check fails
    g1, g2, h1, h2, Tg = planted_pair(64, 902, 0.2)
    g1[5:9] = g1[4]                                                                    # duplicate descriptors on both sides
    g2[20:23] = g2[19]
    out["duplicate_descriptors"] = (g1, g2, h1, h2, Tg)
    return out


# ------------------------------------------------------------------ tests
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


def test_new_symbols_declared_and_exported(built):
    from egonn_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "egonn_hip.h")).read()
    declared = set(re.findall(r"\b(egonn_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.egonn_registration_scratch_bytes(4, 256, 10000) == 4 * 40 * 16
    assert lib.egonn_registration_scratch_bytes(4, 257, 10000) == -1 and lib.egonn_registration_scratch_bytes(4, 128, 0) == -1
    # 64-row x 32-column tiles: (cdiv(n, 64) + cdiv(n, 32)) * n partial minima per pair, a double and an int32 each
    assert lib.egonn_match_mutual_scratch_bytes(3, 200) == 3 * (4 + 7) * 200 * 12
    assert lib.egonn_match_mutual_scratch_bytes(3, 200) == lib.egonn_match_candidates_scratch_bytes(3, 1, 200)
    assert lib.egonn_match_mutual_scratch_bytes(3, 257) == -1 and lib.egonn_match_mutual_scratch_bytes(-1, 128) == -1


def test_argument_checks_need_no_gpu(built):
    """the up-front checks return the library's invalid status before anything is launched"""
    from egonn_amd import _lib
    lib = _lib.load()
    one = 16        # non-null, aligned, never dereferenced: every call below fails its argument check first
    need = lib.egonn_match_mutual_scratch_bytes(1, 128)
    assert need == (2 + 4) * 128 * 12

    def match(feat1=one, feat2=one, n_max=128, dim=128, corr=one, scratch=one, nbytes=need):
        return lib.egonn_match_mutual(feat1, feat2, one, one, 1, n_max, dim, corr, one, scratch, nbytes, None)
    # shape, width, null pointers, 16-byte alignment, then scratch size and 8-byte alignment: all before the first HIP call
    for kw, word in ((dict(n_max=257), b"n_max"), (dict(dim=30), b"width 30"), (dict(feat1=None), b"null"),
                     (dict(feat2=None), b"null"), (dict(corr=None), b"null"), (dict(scratch=None), b"null"),
                     (dict(feat1=one + 4), b"16-byte aligned"), (dict(feat2=one + 8), b"16-byte aligned"),
                     (dict(nbytes=need - 1), b"scratch needs"), (dict(scratch=one + 4), b"8-byte aligned")):
        assert match(**kw) == 1, kw
        assert word in lib.egonn_last_error() and b"match_mutual" in lib.egonn_last_error(), (kw, lib.egonn_last_error())
    assert match(n_max=257, dim=30, feat1=None, scratch=None) == 1 and b"n_max" in lib.egonn_last_error()     # the order
    assert match(dim=30, feat1=None, scratch=None) == 1 and b"width" in lib.egonn_last_error()
    assert match(feat1=one + 4, scratch=None) == 1 and b"null" in lib.egonn_last_error()
    assert match(feat1=one + 4, nbytes=0) == 1 and b"16-byte" in lib.egonn_last_error()
    assert lib.egonn_ransac_pairs(one, one, one, one, one, one, None, 1, 128, 0, 0, 0.5, one, 1 << 20, None, None, None) == 1
    assert lib.egonn_ransac_pairs(one, one, one, one, one, one, None, 1, 128, 100, 0, 0.5, None, 0, None, None, None) == 1
    assert lib.egonn_ransac_pairs(one, one, one, one, one, one, None, 1, 128, 1000, 0, 0.5, one, 8, None, None, None) == 1
    assert lib.egonn_registration_finish(one, one, one, one, one, one, None, 1, 128, -5, 0, 0.5, one, 1 << 20, None, 0.5, one, one,
                                         one, one, None, None, None, None, None, None, None, None) == 1
    assert lib.egonn_registration_finish(one, one, one, one, one, one, None, 1, 128, 100, 0, 0.5, one, 1 << 20, None, 0.5, None,
                                         one, one, one, None, None, None, None, None, None, None, None) == 1


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_registration_has_no_cpu_path(built):
    import egonn_amd
    from egonn_amd import registration
    f1, f2, k1, k2, T = planted_pair(32, 1, 0.0)
    t = torch.from_numpy
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        egonn_amd.get_ransac_result(t(f1), t(f2), t(k1), t(k2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        egonn_amd.calculate_repeatability(t(k1), t(k2), T, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        registration.register_pairs(t(f1)[None], t(f2)[None], t(k1)[None], t(k2)[None])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        egonn_amd.evaluate_local([{"keypoints": t(k1), "features": t(f1)}], [{"keypoints": t(k2), "features": t(f2)}], [0], T[None])


def test_draw_is_the_documented_function():
    ts = np.arange(0, 3000, 7)
    for seed, pid, n in ((0, 0, 128), (12345, 63, 256), (2 ** 63 + 5, 4095, 3), (MASK, 2 ** 30 - 1, 77)):
        for slot in range(3):
            got = draw(seed, pid, ts, slot, n)
            want = [draw_scalar(seed, pid, int(t), slot, n) for t in ts]
            assert got.tolist() == want
            assert got.min() >= 0 and got.max() < n
    d = draw(7, 3, np.arange(200000), 1, 128)
    counts = np.bincount(d, minlength=128)
    assert counts.min() > 1300 and counts.max() < 1830           # 1562.5 +- 6.8 sigma: a uniform draw
    assert (draw(7, 3, np.arange(1000), 1, 128) != draw(8, 3, np.arange(1000), 1, 128)).mean() > 0.9


def test_kabsch_recovers_planted_transforms():
    rng = np.random.default_rng(0)
    S = rng.uniform(-50, 50, size=(200, 3, 3))
    R0 = np.stack([rot_zyx(*rng.uniform(-3, 3, 3)) for _ in range(200)])
    t0 = rng.uniform(-20, 20, size=(200, 3))
    Q = np.einsum("hij,hkj->hki", R0, S) + t0[:, None]
    R, t = kabsch(S, Q)
    assert np.abs(R - R0).max() < 1e-9 and np.abs(t - t0).max() < 1e-8
    assert np.allclose(np.linalg.det(R), 1.0)
    # a mirrored target: the reflection correction keeps det = +1
    Qm = Q * np.array([1.0, 1.0, -1.0])
    Rm, _ = kabsch(S, Qm)
    assert np.allclose(np.linalg.det(Rm), 1.0)


def test_matching_sets_are_recorded_and_inside_the_restatement_cap():
    """every operand set of tests/match_data.py: its regenerated inputs hash to what tests/golden/match_parent.npz recorded,
    the recorded result (the parent commit's kernel on an MI355X) passes the float64 restatement's check, and the restatement
    alone stays inside the cap of the GPU tests (rows within match_band of a tie <= 1 %; exact duplicates have gap 0 and are
    decided by the lowest-index rule, not excused)"""
    from tests import match_data as D
    sets = [(name, D.dense_of(*s), s) for name, s in D.index_sets().items()] + [(n, s, s) for n, s in D.dense_sets().items()]
    assert len(sets) == 15
    for name, (F1, F2, n1, n2), hashed in sets:
        corr, n_corr = D.recorded(name, hashed)
        assert corr.shape == (len(F1), F1.shape[1], 2) and n_corr.shape == (len(F1),)
        excused, total, unchecked = D.check_matching(D.rows_of(F1, F2, n1, n2), corr, n_corr)
        assert excused <= D.EXCUSED_ROW_CAP * total and unchecked == 0, (name, excused, total, unchecked)


def test_one_distance_loop_in_the_library():
    """the fp64 distance loop of the matching operator exists in one kernel file"""
    csrc = os.path.join(REPO, "egonn_amd", "csrc")
    holders = [f for f in sorted(os.listdir(csrc)) if f.endswith(".hip") and "fma(d, d, acc" in open(os.path.join(csrc, f)).read()]
    assert holders == ["match.hip"]


def test_mutual_matching_rules():
    f1, f2, _, _, _ = edge_pairs()["duplicate_descriptors"]
    corr, _, _ = match_f64(f1, f2)
    d2 = ((f1.astype(np.float64)[:, None] - f2.astype(np.float64)[None]) ** 2).sum(-1)
    assert (np.diff(corr[:, 0]) > 0).all()
    for i, j in corr:
        assert j == d2[i].argmin() and i == d2[:, j].argmin()
    # sources 4..8 share one descriptor: they share j, and only the lowest index can be mutual
    assert 4 in corr[:, 0] or d2[:, d2[4].argmin()].argmin() != 4
    assert not set(range(5, 9)) & set(corr[:, 0].tolist())
    # fewer than 3 mutual pairs: every (i, j(i))
    a = np.eye(4, dtype=np.float32)[[0, 0, 0, 1]]
    b = np.eye(4, dtype=np.float32)[[0, 1, 2]]
    corr, _, _ = match_f64(a, b)
    assert corr.tolist() == [[0, 0], [1, 0], [2, 0], [3, 1]]
    assert match_f64(a[:0], b)[0].shape == (0, 2)


@pytest.mark.parametrize("name", list(PLANTED_CASES))
def test_restatement_solves_planted_cases(name):
    c = PLANTED_CASES[name]
    for i, (f1, f2, k1, k2, T_gt) in enumerate(planted_case(name)):
        r = register_f64(f1, f2, k1, k2, T_gt, seed=0, pair_id=i, H=c["H"])
        assert r["success"] == 1 and r["rte"] <= 2.0 and r["rre"] <= 5.0, (name, i, r["rte"], r["rre"])
        assert r["status"] == 0 and r["inliers"] >= 0.3 * (1 - c["outliers"]) * len(k1)
        # the matching cap of the GPU test holds for the restatement alone: rows within the band of a tie <= 1 %
        _, g1, g2 = match_f64(f1, f2)
        band = match_band(f1, f2)
        assert band < 1e-12 and (g1 < band).mean() <= 0.01 and (g2 < band).mean() <= 0.01
        tab = r["table"]
        assert tab["near"].mean() <= 1e-4
        assert (tab["count"] >= 3).any() and (tab["count"] == -2).any()


def test_edge_cases():
    E = edge_pairs()
    for m in (0, 1, 2):
        r = register_f64(*E[f"n_corr_{m}"])
        assert len(r["corr"]) == m and r["status"] == STATUS_FEW_CORR | STATUS_NO_MODEL
        assert np.array_equal(r["T"], np.eye(4)) and r["inliers"] == 0 and (r["table"]["count"] == -1).all()
    r = register_f64(*E["n_corr_3"], H=2000)
    assert len(r["corr"]) == 3 and r["status"] == 0 and r["success"] == 1 and r["inliers"] == 3
    for name in ("identical_keypoints", "collinear"):
        r = register_f64(*E[name], H=2000)
        assert r["status"] == STATUS_NO_MODEL and (r["table"]["count"] == -1).all() and np.array_equal(r["T"], np.eye(4))
    r = register_f64(*E["no_accepted_hypothesis"], H=2000)
    assert r["status"] == STATUS_NO_MODEL and set(np.unique(r["table"]["count"]).tolist()) <= {-1, -2}
    assert (r["table"]["count"] == -2).any()
    r = register_f64(*E["n1_ne_n2"])
    assert r["success"] == 1 and len(E["n1_ne_n2"][0]) == 128 and len(E["n1_ne_n2"][1]) == 100
    r = register_f64(*E["duplicate_descriptors"])
    assert r["success"] == 1


def test_best_rule_and_final_evaluation():
    assert best_rule([-1, -2, 0, -3], [0, 0, 0, 0]) == -1
    assert best_rule([3, 5, 5, 5], [0.1, 0.3, 0.2, 0.2]) == 2
    f1, f2, k1, k2, T = planted_pair(128, 5, 0.25, noise=0.0)
    inl, fit, rmse, cs = final_eval(k1, k2, T)
    assert inl == 96 and fit == 0.75 and rmse < 1e-4 and len(cs) == 96
    assert repeatability_f64(k1, k2, T, 0.5) >= 0.75
    rte, rre, suc = metrics_f64(T, T)
    assert rte == 0.0 and rre < 1e-5 and suc == 1
    T2 = T.copy()
    T2[:3, :3] = T[:3, :3] @ rot_zyx(np.deg2rad(6.0), 0, 0)
    assert abs(metrics_f64(T2, T)[1] - 6.0) < 1e-9 and metrics_f64(T2, T)[2] == 0

"""GPU tests of Horn's closed form (egonn_amd/csrc/horn.h) at its edges (run with -m gpu on an MI355X), through its two callers.

Through ICP: one round (max_iteration = 1) from the identity on a spacing-2 lattice target and a source that is the target moved
back by a small rigid motion (at most 0.1 rad on a cloud of radius 3.5 m plus 0.25 m: every point stays within 0.7 m of its
partner and more than 1.3 m from any other target, which the brute-force oracle of tests/icp_search_data.py confirms), so
the correspondences are the planted ones and T_1 is the rigid fit alone.  The yardstick is icp_step_f64 (Kabsch by SVD in
float64, tests/test_icp_host.py) on the oracle's correspondences, the measure is box_displacement and the bar is BAND = 1e-8 m.
Cases: a full 3-D set, a planar one, three points, a pure translation, no motion, and a collinear set, where the rotation about
the line is free: there U has to be a proper rotation whose summed squared residual is Kabsch's.

Through spectral_verify: 3, 4, 64 and 128 all-inlier correspondences of dyadic keypoints (exact in float32) under the
identity, exact half turns about x, y, z and (1, 1, 0) (the quaternion's w is 0), a half turn about (1, 2, 2) / 3 and a turn by
pi - 1e-6 (both rounded into float32), and planar keypoints under the in-plane and the normal half turn.  The yardstick is
tests/spectral_ref.py (Kabsch by SVD) on the same float32 inputs; the device's error against the planted pose may be 4 x the
restatement's own and never has to be below 16 * 2^-53 times the largest coordinate (another, equally valid operation order).

Measured on an MI355X (the tests print them):
  MEASURED_FIT_DIFF     5.86e-14 m: the largest box displacement between the device's T_1 and icp_step_f64 over the five
                        determined cases (full 5.9e-14, planar 4.3e-14, three points 3.5e-14, translation and identity 0);
                        collinear: summed squared residual 0.0078125000000000278 against Kabsch's 0.007812499999999889
  spectral              largest error against the planted pose as a displacement of the keypoints' box: device 2.93e-14 m,
                        restatement 6.59e-14 m on the inputs that are exact in float32; device 1.75e-06 m, restatement 1.75e-06 m
                        on the two that are rounded into float32 (the rounding of the keypoints, the same for both)
The test asserts BAND >= 100 x the value it measures and BAND >= 100 x MEASURED_FIT_DIFF."""
import math

import numpy as np
import pytest
import torch

from tests import icp_search_data as data
from tests import pose_graph_ref as pg_ref
from tests import spectral_ref
from tests.test_icp_host import BAND, box_displacement, icp_step_f64, kabsch_f64

pytestmark = pytest.mark.gpu

MEASURED_FIT_DIFF = 5.86e-14  # metres, as printed by test_horn_through_icp on an MI355X
MAX_DIST = 1.0


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
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _motion(rotvec, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = pg_ref.exp_so3(rotvec), t
    return T


def _lattice(nx, ny, nz):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    return (g - (np.array([nx, ny, nz]) - 1) / 2.0) * 2.0


# ------------------------------------------------------------------ Horn through ICP
FULL, PLANE, THREE = _lattice(3, 3, 3), _lattice(3, 3, 1) + np.array([0.0, 0.0, 1.0]), np.array([[0.0, 0, 0], [2.0, 0, 0], [0, 2.0, 0]])
LINE = _lattice(3, 1, 1)
ICP_CASES = {                                            # name -> (target, motion that takes the source onto it, scale of the source)
    "full": (FULL, _motion([0.03, -0.05, 0.07], [0.125, -0.0625, 0.1875]), 1.0),
    "planar": (PLANE, _motion([0.06, 0.02, -0.07], [-0.125, 0.25, 0.0625]), 1.0),
    "three_points": (THREE, _motion([-0.04, 0.08, 0.03], [0.0625, 0.125, -0.25]), 1.0),
    "translation": (FULL, _motion([0.0, 0.0, 0.0], [0.25, -0.125, 0.1875]), 1.0),
    "identity": (FULL, _motion([0.0, 0.0, 0.0], [0.0, 0.0, 0.0]), 1.0),
    "collinear": (LINE, _motion([0.02, 0.05, -0.08], [0.125, 0.0625, -0.125]), 1.0 - 1.0 / 32),
}


def _icp_case(name):
    tgt, M, scale = ICP_CASES[name]
    src = (tgt * scale - M[:3, 3]) @ M[:3, :3]           # M src = scale * tgt
    return src, tgt, M


def _one_round(gpu, names):
    srcs, tgts = [_icp_case(n)[0] for n in names], [_icp_case(n)[1] for n in names]
    so, to = np.cumsum([0] + [len(s) for s in srcs]), np.cumsum([0] + [len(t) for t in tgts])
    out = gpu.icp_pairs(_cu(np.concatenate(srcs)), _cu(so.astype(np.int64)), _cu(np.concatenate(tgts)), _cu(to.astype(np.int64)), None,
                        MAX_DIST, 1, True)
    torch.cuda.synchronize()
    r = {k: _np(v) for k, v in out.items() if not k.startswith("_")}
    assert r["T_trace"].shape == (len(names), 2, 4, 4)
    return r, so


def test_horn_through_icp(gpu):
    names = list(ICP_CASES)
    r, so = _one_round(gpu, names)
    worst = 0.0
    for p, name in enumerate(names):
        src, tgt, M = _icp_case(name)
        assert max(np.linalg.norm(src, axis=1).max(), np.linalg.norm(tgt, axis=1).max()) <= 4.0 and math.acos(min(1.0, (np.trace(M[:3, :3]) - 1) / 2)) <= 0.1
        o = data.oracle(src, tgt, np.eye(4), MAX_DIST)
        assert np.array_equal(o["j"], np.arange(len(src))), name        # the nearest target is the planted partner
        assert r["eval_trace"][p, 0, 0] == len(src) and np.array_equal(r["T_trace"][p, 0], np.eye(4)) and r["iterations"][p] == 1
        T1 = r["T_trace"][p, 1]
        R = T1[:3, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and np.linalg.det(R) > 0 and np.array_equal(T1[3], [0.0, 0.0, 0.0, 1.0]), name
        want = icp_step_f64(src, tgt, np.eye(4), o["j"])
        res = lambda T: float((((src @ T[:3, :3].T + T[:3, 3]) - tgt) ** 2).sum())      # noqa: E731
        if name == "collinear":                              # the rotation about the line is free: the residual is what is determined
            print(f"[fit edges] collinear: residual device {res(T1):.17g}, Kabsch {res(want):.17g}")
            assert res(want) > 1e-3 and res(T1) <= res(want) * (1.0 + 1e-12)
            continue
        d = box_displacement(T1, want)
        print(f"[fit edges] {name}: T_1 against icp_step_f64 on the box {d:.3e} m, against the planted motion {box_displacement(T1, M):.3e} m")
        assert d <= BAND, (name, d)
        assert box_displacement(want, M) <= 1e-10               # the yardstick finds the planted motion
        worst = max(worst, d)
    print("MEASURED_FIT_DIFF =", worst)
    assert BAND >= 100.0 * worst and BAND >= 100.0 * MEASURED_FIT_DIFF


def test_kabsch_yardstick_on_the_collinear_case():
    """the collinear case has a residual that no rotation removes (the source is 1/32 shorter): what the device is compared on"""
    src, tgt, M = _icp_case("collinear")
    U = kabsch_f64(src, tgt)
    res = float((((src @ U[:3, :3].T + U[:3, 3]) - tgt) ** 2).sum())
    assert abs(res - 8.0 / 1024.0) <= 1e-12 and abs(np.linalg.det(U[:3, :3]) - 1.0) <= 1e-12


# ------------------------------------------------------------------ Horn through spectral_verify
N_MAX = 128
COUNTS = (3, 4, 64, 128)
T_PLANT = np.array([3.5, -7.25, 1.125])


def _half_turn(axis):
    a = np.asarray(axis, np.float64)
    return 2.0 * np.outer(a, a) / (a @ a) - np.eye(3)


ROTATIONS = {                                            # name -> (R, exact in float32, planar keypoints)
    "identity": (np.eye(3), True, False),
    "half_x": (np.diag([1.0, -1.0, -1.0]), True, False),
    "half_y": (np.diag([-1.0, 1.0, -1.0]), True, False),
    "half_z": (np.diag([-1.0, -1.0, 1.0]), True, False),
    "half_110": (_half_turn([1.0, 1.0, 0.0]), True, False),
    "half_122": (_half_turn([1.0, 2.0, 2.0]), False, False),
    "pi_minus_1e-6": (pg_ref.exp_so3(np.array([2.0, -1.0, 2.0]) / 3.0 * (math.pi - 1e-6)), False, False),
    "planar_in_plane": (np.diag([1.0, -1.0, -1.0]), True, True),
    "planar_normal": (np.diag([-1.0, -1.0, 1.0]), True, True),
}


# The sets of 3 and 4 keypoints are fixed, well-spread figures, the larger ones random.  A rigid fit's rounding error is the
# float64 rounding of the coordinates times norm / gap of Horn's 4 x 4 matrix (the gap of its two largest eigenvalues is
# 2 (s2 + s3) of the cross-covariance's singular values, the norm s1 + s2 + s3), for Kabsch by SVD as for Horn by Jacobi.  On a
# thin figure that factor is large and the two routes, both within it, scatter around each other by more than the rule's 4 x
# from case to case (the numpy restatement of horn.h shows it: on a triangle with gap / norm = 0.065 Kabsch is off by 2.7e-13 m
# and Horn by 2.8e-14 m under one half turn, 6.1e-14 m and 5.8e-13 m under another).  The comparison is about the half turn,
# where w = 0, not about thin figures, so every set has to have gap / norm >= MIN_GAP; _spectral_cases asserts it.
FIGURE = np.array([[-32.0, -24.0, 4.0], [32.0, -20.0, -8.0], [-4.0, 30.0, 12.0], [6.0, -2.0, -34.0]])
MIN_GAP = 0.25


def _gap(k):
    a = k - k.mean(0)
    sv = np.linalg.svd(a.T @ a)[1]
    return 2.0 * (sv[1] + sv[2]) / sv.sum()


def _keypoints(n, seed, planar):
    """n dyadic keypoints (multiples of 1/8 inside +-34 m, exact in float32), at least 3 m apart"""
    if n <= len(FIGURE):
        k = FIGURE[:n].copy()
        if planar:
            k[:, 2] = 2.5
        return k
    rng = np.random.default_rng(seed)
    cells = rng.permutation(16 * 16 * (1 if planar else 16))[:n]
    ijk = np.stack([cells % 16, (cells // 16) % 16, cells // 256], 1).astype(np.float64) - 8.0
    k = ijk * 4.0 + rng.integers(0, 9, (n, 3)) / 8.0
    if planar:
        k[:, 2] = 2.5
    return k


def _spectral_cases():
    cases = []
    for name, (R, exact, planar) in ROTATIONS.items():
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(R) - 1.0) <= 1e-15
        for n in COUNTS:
            k1 = _keypoints(n, 100 + n, planar)
            assert _gap(k1) >= MIN_GAP, (name, n, _gap(k1))
            k2 = k1 @ R.T + T_PLANT
            if exact:
                assert np.array_equal(k2.astype(np.float32).astype(np.float64), k2)
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = R, T_PLANT
            cases.append((name, n, exact, k1.astype(np.float32), k2.astype(np.float32), T))
            assert np.array_equal(k1.astype(np.float32).astype(np.float64), k1)
    return cases


def _box_err(T, Tp, C):
    c = np.array([[x, y, z] for x in (-C, C) for y in (-C, C) for z in (-C, C)])
    d = (c @ T[:3, :3].T + T[:3, 3]) - (c @ Tp[:3, :3].T + Tp[:3, 3])
    return float(np.sqrt((d * d).sum(1)).max())


def test_horn_through_spectral_verify(gpu):
    cases = _spectral_cases()
    P = len(cases)
    kp1, kp2 = np.zeros((P, N_MAX, 3), np.float32), np.zeros((P, N_MAX, 3), np.float32)
    corr, cnt = np.full((P, N_MAX, 2), -1, np.int32), np.zeros(P, np.int32)
    for i, (_, n, _, k1, k2, _) in enumerate(cases):
        kp1[i, :n], kp2[i, :n], cnt[i] = k1, k2, n
        corr[i, :n] = np.arange(n)[:, None]
    out = gpu.spectral_verify(_cu(kp1), _cu(kp2), _cu(corr), _cu(cnt), _cu(cnt), _cu(cnt))
    torch.cuda.synchronize()
    T_dev, status, inliers = _np(out["T"]), _np(out["status"]), _np(out["inliers"])
    worst = {True: [0.0, 0.0], False: [0.0, 0.0]}
    for i, (name, n, exact, k1, k2, Tp) in enumerate(cases):
        want = spectral_ref.spectral_f64(k1, k2, corr[i, :n], N_MAX)
        assert want["status"] == 0 and want["inliers"] == n, (name, n)
        assert status[i] == 0 and inliers[i] == n, (name, n, status[i], inliers[i])
        C = float(max(np.abs(k1).max(), np.abs(k2).max()))
        e_dev, e_ref = _box_err(T_dev[i], Tp, C), _box_err(want["T"], Tp, C)
        worst[exact] = [max(worst[exact][0], e_dev), max(worst[exact][1], e_ref)]
        R = T_dev[i, :3, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and np.linalg.det(R) > 0, (name, n)
        assert e_dev <= max(4.0 * e_ref, 16.0 * 2.0 ** -53 * C), (name, n, e_dev, e_ref)
    print(f"[fit edges] spectral_verify against the planted pose: exact inputs device {worst[True][0]:.2e} m, restatement "
          f"{worst[True][1]:.2e} m; rounded inputs device {worst[False][0]:.2e} m, restatement {worst[False][1]:.2e} m")

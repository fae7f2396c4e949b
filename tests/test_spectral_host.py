"""Host-side checks of the spectral geometric verification (no GPU needed): the entry points are declared and exported, every
argument check answers before anything is launched, the float64 restatement (tests/spectral_ref.py) gives the numbers that
can be written out by hand, and the conditions tests/test_gpu_spectral.py relies on hold on the restatement alone: no decision
of any pair it compares sits within 1e-6 of its threshold, the planted relocalisation is ranked as planted, and the method
solves 5, 8 and 13 planted inliers among 128 correspondences for 20 seeds each."""
import os
import re

import numpy as np
import pytest

from tests import spectral_ref as ref
from tests.test_registration_host import STATUS_FEW_CORR, STATUS_NO_MODEL, edge_pairs, match_f64
from tests.test_relocalize_host import PLANTED_M, WEAK_OF, planted_case

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["egonn_spectral_verify", "egonn_spectral_verify_scratch_bytes"]
MARGIN = 1e-6


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
    import egonn_amd
    assert egonn_amd.spectral_verify is egonn_amd.registration.spectral_verify and "spectral_verify" in egonn_amd.__all__
    sb = lib.egonn_spectral_verify_scratch_bytes
    assert sb(5, 128) == 0 and sb(1 << 20, 1) == 0                     # M lives in LDS
    assert sb(5, 129) == 5 * 129 * 129 * 4 and sb(4096, 256) == 512 * 256 * 256 * 4 and sb(0, 256) == 0
    assert sb(-1, 128) == -1 and sb(1, 0) == -1 and sb(1, 257) == -1 and sb((1 << 20) + 1, 128) == -1


def test_argument_checks_need_no_gpu(built):
    """the up-front checks return the library's invalid status before anything is launched"""
    from egonn_amd import _lib
    lib = _lib.load()
    one = 16        # non-null, aligned, never dereferenced: every call below fails its argument check first
    need = lib.egonn_spectral_verify_scratch_bytes(2, 256)
    nan = float("nan")

    def call(kp1=one, kp2=one, n1=one, n2=one, corr=one, n_corr=one, P=2, n_max=256, d_thr=0.6, iterations=32, seed_ratio=0.5,
             dist_th=0.5, T_gt=None, repeat_th=0.5, scratch=one, nbytes=need):
        return lib.egonn_spectral_verify(kp1, kp2, n1, n2, corr, n_corr, P, n_max, d_thr, iterations, seed_ratio, dist_th, T_gt,
                                         repeat_th, scratch, nbytes, *([one] * 14), None)
    cases = [(dict(kp1=None), b"null"), (dict(kp2=None), b"null"), (dict(n1=None), b"null"), (dict(n2=None), b"null"),
             (dict(corr=None), b"null"), (dict(n_corr=None), b"null"), (dict(P=-1), b"bad shape"), (dict(n_max=0), b"bad shape"),
             (dict(n_max=257), b"bad shape"), (dict(d_thr=0.0), b"d_thr"), (dict(d_thr=-1.0), b"d_thr"), (dict(d_thr=nan), b"d_thr"),
             (dict(dist_th=0.0), b"distance threshold"), (dict(dist_th=-0.5), b"distance threshold"),
             (dict(dist_th=nan), b"distance threshold"), (dict(iterations=0), b"iterations"), (dict(seed_ratio=0.0), b"seed_ratio"),
             (dict(seed_ratio=1.5), b"seed_ratio"), (dict(seed_ratio=nan), b"seed_ratio"),
             (dict(T_gt=one, repeat_th=-1.0), b"repeatability"), (dict(nbytes=need - 1), b"scratch needs"),
             (dict(scratch=None), b"scratch needs"), (dict(scratch=one + 4), b"8-byte aligned")]
    for kw, word in cases:
        assert call(**kw) == 1, kw
        assert word in lib.egonn_last_error() and b"spectral_verify" in lib.egonn_last_error(), (kw, lib.egonn_last_error())
    assert call(n_max=257, kp1=None, d_thr=0.0) == 1 and b"bad shape" in lib.egonn_last_error()          # the order
    assert call(kp1=None, d_thr=0.0, scratch=None) == 1 and b"null" in lib.egonn_last_error()
    assert call(d_thr=0.0, scratch=None) == 1 and b"d_thr" in lib.egonn_last_error()
    assert call(P=0, scratch=None, nbytes=0) == 0                       # nothing to do, nothing launched, no scratch needed


def test_python_surface_refuses_unknown_methods(built):
    import egonn_amd
    from egonn_amd import registration
    with pytest.raises(ValueError, match="method"):
        registration.check_method("register_pairs", "icp")
    with pytest.raises(ValueError, match="verify_method"):
        egonn_amd.LoopDetector(verify_method="icp", device="cpu")
    assert registration.check_method("x", "spectral") == "spectral" and registration.METHODS == ("ransac", "spectral")


def test_output_table_follows_the_c_prototypes():
    """registration.PAIR_OUTPUTS yields, per method, the pointer order of its entry point in include/egonn_hip.h from the first
    output onwards, and verify_candidates' per-pair keys rename exactly the table's rows that it keeps"""
    from egonn_amd import registration, relocalize
    header = open(os.path.join(REPO, "include", "egonn_hip.h")).read()
    c_name = {"correspondence_set": "corr_set"}         # the one name Python spells out (Open3D's attribute)
    for method, entry, first in (("ransac", "egonn_registration_finish", "T"), ("spectral", "egonn_spectral_verify", "eigenvalue")):
        args = re.search(r"\bint " + entry + r"\((.*?)\);", header, re.S).group(1)
        params = [re.search(r"(\w+)\s*$", a).group(1) for a in args.split(",")]
        assert params[-1] == "stream"
        rows = registration.pair_outputs(method)
        names = [r[0] for r in rows]
        assert [c_name.get(n, n) for n in names] == params[params.index(first):-1], method
        assert len(set(names)) == len(names) and all(r[4] in (None, method) for r in rows)
        keys = relocalize.pair_keys(method)
        assert set(keys) | set(relocalize._NOT_KEPT) == set(names) and not set(keys) & set(relocalize._NOT_KEPT)
        assert {n: k for n, k in keys.items() if n != k} == {"status": "pair_status"} and len(set(keys.values())) == len(keys)
    assert [r[0] for r in registration.PAIR_OUTPUTS if r[3]] == ["rte", "rre", "success", "repeatability"]
    assert {r[0] for r in registration.PAIR_OUTPUTS if r[4] == "ransac"} == {"best_t"}
    assert {r[0] for r in registration.PAIR_OUTPUTS if r[4] == "spectral"} == {"eigenvalue", "score", "weights", "n_seeds"}


# ------------------------------------------------------------------ the restatement on numbers that can be written out
def _identity_corr(m):
    return np.stack([np.arange(m), np.arange(m)], 1).astype(np.int32)


@pytest.mark.parametrize("m", [3, 7, 64])
def test_identical_sets_give_the_complete_graph(m):
    rng = np.random.default_rng(m)
    p = rng.uniform(-50, 50, (m, 3)).astype(np.float32)
    r = ref.spectral_f64(p, p, _identity_corr(m), 128, np.eye(4))
    assert np.array_equal(r["M"], 1.0 - np.eye(m))
    assert abs(r["eigenvalue"] - (m - 1)) <= 1e-12 and abs(r["score"] - (m - 1) / 127) <= 1e-14
    assert np.allclose(r["weights"][:m], 1 / np.sqrt(m), rtol=0, atol=1e-15) and (r["weights"][m:] == 0).all()
    assert r["n_seeds"] == m and r["inliers"] == m and r["status"] == 0 and r["inlier_rmse"] <= 1e-12
    assert np.allclose(r["T"], np.eye(4), rtol=0, atol=1e-12) and r["success"] == 1


def test_two_rigid_groups_the_larger_one_wins():
    """10 correspondences moved by one pose and 4 by another: inside a group every distance is kept (M = 1), across the groups
    none is (the second pose turns by 90 degrees and shifts by 40 m, so every cross pair changes its length by far more than
    d_thr): M is block diagonal, its top eigenvalue 10 - 1, the eigenvector uniform on the group of 10"""
    from egonn_amd.synth import rot_zyx
    rng = np.random.default_rng(5)
    p = rng.uniform(-30, 30, (14, 3))
    T1, T2 = np.eye(4), np.eye(4)
    T1[:3, :3], T1[:3, 3] = rot_zyx(0.3, 0.01, -0.02), [4.0, -2.0, 0.5]
    T2[:3, :3], T2[:3, 3] = rot_zyx(0.3 + np.pi / 2, 0.0, 0.0), [40.0, 30.0, 0.0]
    q = p @ T1[:3, :3].T + T1[:3, 3]
    q[10:] = p[10:] @ T2[:3, :3].T + T2[:3, 3]
    r = ref.spectral_f64(p.astype(np.float32), q.astype(np.float32), _identity_corr(14), 64, T1)
    assert (r["M"][:10, 10:] == 0).all() and (r["M"][:10, :10] + np.eye(10) > 1 - 1e-6).all()
    assert abs(r["eigenvalue"] - 9.0) < 1e-4 and r["seeds"].tolist() == [True] * 10 + [False] * 4 and r["n_seeds"] == 10
    assert np.allclose(r["weights"][:10], 1 / np.sqrt(10), atol=1e-6) and np.abs(r["weights"][10:]).max() < 1e-9
    assert r["inliers"] == 10 and r["success"] == 1 and r["rte"] < 1e-4 and r["rre"] < 1e-4


@pytest.mark.parametrize("m", [0, 1, 2])
def test_fewer_than_three_correspondences(m):
    f1, f2, k1, k2, T = edge_pairs()[f"n_corr_{m}"]
    corr = match_f64(f1, f2)[0]
    assert len(corr) == m
    r = ref.spectral_f64(k1, k2, corr, 64, T)
    assert r["status"] == STATUS_FEW_CORR | STATUS_NO_MODEL and r["inliers"] == 0 and np.array_equal(r["T"], np.eye(4))
    assert r["n_seeds"] == m and np.isfinite([r["eigenvalue"], r["score"], r["inlier_rmse"], r["rte"], r["rre"]]).all()
    assert r["eigenvalue"] == 0.0 if m < 2 else 0.0 <= r["eigenvalue"] <= 1.0


@pytest.mark.parametrize("name", ["identical_keypoints", "collinear"])
def test_degenerate_sets_have_no_model(name):
    f1, f2, k1, k2, T = edge_pairs()[name]
    corr = match_f64(f1, f2)[0]
    r = ref.spectral_f64(k1, k2, corr, 64, T)
    m = len(corr)
    assert m >= 3 and r["status"] == STATUS_NO_MODEL and r["inliers"] == 0 and np.array_equal(r["T"], np.eye(4))
    assert abs(r["eigenvalue"] - (m - 1)) < 1e-6 and r["n_seeds"] == m            # every distance is kept: the complete graph
    assert np.isfinite(r["weights"]).all() and np.isfinite([r["score"], r["inlier_rmse"], r["fitness"], r["rte"], r["rre"]]).all()


def test_zero_matrix_has_no_model():
    """every pair of correspondences changes its length by more than d_thr: M = 0, the first product M v vanishes"""
    p = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0], [0, 0, 10]], np.float32)
    r = ref.spectral_f64(p, p * np.float32(3.0), _identity_corr(4), 64, np.eye(4))
    assert not r["M"].any() and r["eigenvalue"] == 0.0 and r["status"] == STATUS_NO_MODEL and r["inliers"] == 0
    assert np.allclose(r["weights"][:4], 0.5) and r["n_seeds"] == 4


# ------------------------------------------------------------------ what the GPU tests rely on
def test_no_compared_decision_sits_on_its_threshold():
    """every pair whose sets the GPU test compares with this restatement decides at least 1e-6 away from both thresholds"""
    for key, make in (("sweep", ref.sweep_cases), ("registration", ref.planted_registration_cases), ("high", ref.high_outlier_cases)):
        for name, r in ref.solved(key, make).items():
            assert r["seed_margin"] > MARGIN and r["residual_margin"] > MARGIN, (name, r["seed_margin"], r["residual_margin"])
    for name, r in ref.solved("sweep", ref.sweep_cases).items():            # the consistent set is unique: the gap is wide
        m = int(name[1:].split("_")[0])
        assert m < 3 or (r["gap"] > 1.0 and r["status"] == 0 and r["success"] == 1), (name, r["gap"], r["status"])
    for name, r in ref.solved("registration", ref.planted_registration_cases).items():
        assert r["success"] == 1 and r["gap"] > 1.0, name


def test_planted_relocalization_is_ranked_as_planted():
    c = planted_case()
    res = {k: ref.spectral_f64(*v[:3], 64, v[3]) for k, v in ref.planted_relocalization_cases().items()}
    for (q, m), r in res.items():
        assert r["seed_margin"] > MARGIN and r["residual_margin"] > MARGIN, (q, m)
    for q in range(PLANTED_M):
        order = sorted(c["nn"][q], key=lambda m: (-res[(q, int(m))]["inliers"], res[(q, int(m))]["inlier_rmse"]))
        assert order[0] == q and res[(q, q)]["success"] == 1 and res[(q, q)]["inliers"] > max(
            res[(q, int(m))]["inliers"] for m in c["nn"][q] if m != q), q
        if q == WEAK_OF:
            assert order[1] == PLANTED_M and res[(q, PLANTED_M)]["success"] == 1


def test_high_outlier_ratios_are_solved():
    """20 seeds x {5, 8, 13} planted inliers of 128 (96 %, 94 % and 90 % outliers): rotation error under 5 degrees, translation
    error under 2 m and at most one planted inlier lost, for every seed"""
    res = ref.solved("high", ref.high_outlier_cases)
    for name, n_max, k1, k2, corr, T, good in ref.high_outlier_cases():
        r = res[name]
        lost = int((good & ~r.get("fit_inliers", np.zeros(len(good), bool))).sum())
        assert r["success"] == 1 and r["rre"] < 5.0 and r["rte"] < 2.0 and lost <= 1, (name, r["rte"], r["rre"], lost)

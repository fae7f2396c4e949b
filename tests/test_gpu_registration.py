"""GPU tests of the keypoint-set registration (run with -m gpu on an MI355X) against the float64 restatement of
tests/test_registration_host.py: matching entry by entry, the RANSAC table hypothesis by hypothesis, the selection, the
planted poses, determinism / batch / chunking / graph invariances, the descriptor path end to end and the argument checks.

Measured difference between the device's and the restatement's transformed coordinates (test_band_measurement: the device
returns one transform per pair and run, the winner's, so the measurement covers the winning hypothesis of every pair of
every committed case under BAND_SEEDS different seeds; the device transform and the restatement's SVD transform of the
same triple are applied to every source keypoint): MEASURED_COORD_DIFF below.  BAND (1e-9 m, tests/test_registration_host.py) must
be >= 100 x that and <= 1e-6 m; the test asserts both."""
import numpy as np
import pytest
import torch

from tests.match_data import EXCUSED_ROW_CAP, check_matching as _check_matching, dense_sets, recorded
from tests.test_registration_host import (BAND, PLANTED_CASES, STATUS_CLIPPED, STATUS_FEW_CORR, STATUS_NO_MODEL, best_rule,
                                          edge_pairs, final_eval, hypothesis_transform_f64, metrics_f64, pad_batch,
                                          planted_case, planted_pair, ransac_f64, repeatability_f64)

pytestmark = pytest.mark.gpu

BAND_SEEDS = 8
MEASURED_COORD_DIFF = 5.791e-13   # metres, as printed by test_band_measurement on an MI355X (28 pairs x BAND_SEEDS = 224 winners)
BOX_RADIUS = 114.0            # metres: farthest corner of the +-80 m x +-80 m x +-10 m box from its centre
ROT_TOL = BAND / BOX_RADIUS   # radians: a rotation difference that moves no point of the box by more than BAND
EXCUSED_HYP_CAP = 1e-4        # share of P x H per case
# rre goes through acos near 1: at angle a its error is eps / sin(a), and an exact identity gives sqrt(2 eps) = 1.5e-8 rad
RRE_ATOL_DEG = 1e-5


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


def _run(gpu, pairs, H, seed=0, pids=None, n_max=None, debug=True, with_gt=True):
    F1, F2, K1, K2, n1, n2 = pad_batch(pairs, n_max)
    gt = np.stack([p[4] for p in pairs]) if with_gt else None
    out = gpu.register_pairs(_cu(F1), _cu(F2), _cu(K1), _cu(K2), n1=_cu(n1), n2=_cu(n2), T_gt=None if gt is None else _cu(gt),
                             ransac_max_it=H, seed=seed, pair_ids=None if pids is None else _cu(np.asarray(pids, np.int32)),
                             debug=debug)
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in out.items() if k != "_keep"}


_CACHE = {}


def _case(gpu, name):
    """device outputs of a planted case + the restatement's table of every pair on the device's correspondences"""
    if name not in _CACHE:
        pairs, H = planted_case(name), PLANTED_CASES[name]["H"]
        out = _run(gpu, pairs, H)
        tabs = [ransac_f64(p[2], p[3], out["corr"][i, :out["n_corr"][i]], 0, i, H) for i, p in enumerate(pairs)]
        _CACHE[name] = (pairs, H, out, tabs)
    return _CACHE[name]


def _check_table(name, out, tabs, H):
    """hyp_count equal and hyp_err2 close for every hypothesis the restatement does not mark near a decision"""
    excused = 0
    for i, tab in enumerate(tabs):
        ok = ~tab["near"]
        excused += int(tab["near"].sum())
        bad = np.nonzero(ok & (out["hyp_count"][i] != tab["count"]))[0]
        assert len(bad) == 0, (name, i, bad[:8], out["hyp_count"][i][bad[:8]], tab["count"][bad[:8]])
        # each inlier's d^2 moves by at most 2 * 0.5 * BAND when the transformed point moves by BAND
        tol = np.maximum(tab["count"], 0) * BAND + 1e-12 * tab["err2"]
        assert (np.abs(out["hyp_err2"][i] - tab["err2"])[ok] <= tol[ok]).all(), (name, i)
    share = excused / (len(tabs) * H)
    print(f"[registration] {name}: excused hypotheses {excused} of {len(tabs) * H} ({share:.2e})")
    assert share <= EXCUSED_HYP_CAP
    return excused


def _check_selection(pairs, out, tabs):
    for i, (p, tab) in enumerate(zip(pairs, tabs)):
        bt = best_rule(out["hyp_count"][i], out["hyp_err2"][i])          # of the DEVICE's own table: exact
        assert out["best_t"][i] == bt, i
        T = out["T"][i]
        assert np.array_equal(T[3], [0, 0, 0, 1])
        if bt < 0:
            assert np.array_equal(T, np.eye(4)) and out["inliers"][i] == 0 and out["fitness"][i] == 0 and out["inlier_rmse"][i] == 0
            assert out["status"][i] & STATUS_NO_MODEL and (out["correspondence_set"][i] == -1).all()
            continue
        assert not out["status"][i] & STATUS_NO_MODEL
        if not tab["near"][bt]:
            assert np.linalg.norm(T[:3, :3] - tab["R"][bt]) / np.sqrt(2) <= ROT_TOL, i       # = the angle, for small angles
            assert np.abs(T[:3, 3] - tab["t"][bt]).max() <= BAND, i
        assert abs(np.linalg.det(T[:3, :3]) - 1) < 1e-12
        # the final evaluation, restated at the device's T
        a = p[2].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        d = np.sqrt(((a[:, None] - p[3].astype(np.float64)[None]) ** 2).sum(-1).min(1)) if len(p[3]) else np.ones(len(a))
        if len(a) and np.abs(d - 0.5).min() <= BAND:
            continue                                                      # a keypoint on the threshold: either count is right
        inl, fit, rmse, cset = final_eval(p[2], p[3], T)
        assert out["inliers"][i] == inl and out["fitness"][i] == fit, i
        assert abs(out["inlier_rmse"][i] - rmse) <= 1e-9 * max(rmse, 1e-3)
        assert np.array_equal(out["correspondence_set"][i, :inl], cset) and (out["correspondence_set"][i, inl:] == -1).all()


def _check_metrics(pairs, out):
    for i, p in enumerate(pairs):
        rte, rre, suc = metrics_f64(out["T"][i], p[4])
        assert abs(out["rte"][i] - rte) <= 1e-9 and abs(out["rre"][i] - rre) <= RRE_ATOL_DEG, i
        if abs(rte - 2.0) > 1e-9 and abs(rre - 5.0) > RRE_ATOL_DEG:
            assert out["success"][i] == suc
        assert abs(out["repeatability"][i] - repeatability_f64(p[2], p[3], p[4], 0.5)) <= 1e-12, i


# ------------------------------------------------------------------ 1. matching
@pytest.mark.parametrize("name", list(PLANTED_CASES))
def test_matching_equals_restatement(gpu, name):
    pairs = planted_case(name)
    F1, F2, _, _, n1, n2 = pad_batch(pairs)
    corr, n_corr = gpu.match_mutual(_cu(F1), _cu(F2), _cu(n1), _cu(n2))
    assert corr.dtype == torch.int32 and n_corr.dtype == torch.int32
    excused, total, unchecked = _check_matching(pairs, _np(corr), _np(n_corr))
    print(f"[registration] {name}: excused matching rows {excused} of {total}, unchecked pairs {unchecked}")
    assert excused <= EXCUSED_ROW_CAP * total and unchecked == 0
    # what the parent commit's one-workgroup-per-pair kernel gave on these inputs (tests/golden/match_parent.npz)
    gold, gold_n = recorded(name, dense_sets()[name])
    assert np.array_equal(_np(n_corr), gold_n) and np.array_equal(_np(corr), gold)


def test_edge_pairs_equal_recorded_parent(gpu):
    F1, F2, n1, n2 = dense_sets()["edge_pairs"]
    corr, n_corr = gpu.match_mutual(_cu(F1), _cu(F2), _cu(n1), _cu(n2))
    gold, gold_n = recorded("edge_pairs", (F1, F2, n1, n2))
    assert np.array_equal(_np(n_corr), gold_n) and np.array_equal(_np(corr), gold)


# the dense addressing at the smallest shapes where its index arithmetic can go wrong: P = 3 pairs, two row tiles / two column
# tiles with a one-row remainder (n_max = 65 = 64 + 1 with D = 4, n_max = 33 = 32 + 1 with D = 8)
@pytest.mark.parametrize("n_max,D", [(65, 4), (33, 8)])
def test_dense_addressing_small_shapes(gpu, n_max, D):
    rng = np.random.default_rng(n_max)
    F1, F2 = (rng.standard_normal((3, n_max, D)).astype(np.float32) for _ in range(2))
    for counts in ((65, 33), (1, 65), (0, 5)):
        n1 = np.array([min(counts[0], n_max)] * 3, np.int32)
        n2 = np.array([min(counts[1], n_max)] * 3, np.int32)
        n1[1], n2[1] = n2[1], n1[1]                                        # the middle pair the other way round
        corr, n_corr = (_np(x) for x in gpu.match_mutual(_cu(F1), _cu(F2), _cu(n1), _cu(n2)))
        pairs = [(F1[p, :n1[p]], F2[p, :n2[p]]) for p in range(3)]
        excused, total, unchecked = _check_matching(pairs, corr, n_corr)
        assert excused == 0 and unchecked == 0, (counts, excused, total, unchecked)
        # pair 1 of the batch equals the same pair run alone: the p / k and p addressing cannot cross pairs
        one, one_n = (_np(x) for x in gpu.match_mutual(_cu(F1[1:2]), _cu(F2[1:2]), _cu(n1[1:2]), _cu(n2[1:2])))
        assert np.array_equal(one[0], corr[1]) and one_n[0] == n_corr[1]


def test_match_mutual_chunks_change_no_bit(gpu):
    """registration.match_mutual issues at most `chunk_pairs` pairs per call on one scratch buffer: P = 5 in chunks of 2"""
    pairs = planted_case("n128_out30")[:5]
    F1, F2, _, _, n1, n2 = (_cu(x) for x in pad_batch(pairs))
    whole, whole_n = gpu.match_mutual(F1, F2, n1, n2)
    parts, parts_n = gpu.match_mutual(F1, F2, n1, n2, chunk_pairs=2)
    assert torch.equal(whole, parts) and torch.equal(whole_n, parts_n) and int(whole_n.min()) >= 3


# ------------------------------------------------------------------ 2. per-hypothesis parity, and the band it rests on
def test_band_measurement(gpu):
    worst, n = 0.0, 0
    for name in PLANTED_CASES:
        pairs, H = planted_case(name), PLANTED_CASES[name]["H"]
        for seed in range(BAND_SEEDS):
            out = _case(gpu, name)[2] if seed == 0 else _run(gpu, pairs, H, seed=seed, debug=False)
            for i, p in enumerate(pairs):
                bt = int(out["best_t"][i])
                assert bt >= 0
                R, t = hypothesis_transform_f64(p[2], p[3], out["corr"][i, :out["n_corr"][i]], seed, i, bt)
                s = p[2].astype(np.float64)
                dev = s @ out["T"][i][:3, :3].T + out["T"][i][:3, 3]
                worst = max(worst, float(np.abs(dev - (s @ R.T + t)).max()))
                n += 1
    print(f"[registration] largest device-vs-restatement transformed-coordinate difference over {n} winning hypotheses: "
          f"{worst:.3e} m")
    assert 100 * worst <= BAND <= 1e-6
    assert 100 * MEASURED_COORD_DIFF <= BAND


@pytest.mark.parametrize("name", list(PLANTED_CASES))
def test_every_hypothesis_equals_restatement(gpu, name):
    pairs, H, out, tabs = _case(gpu, name)
    assert out["hyp_count"].shape == (len(pairs), H) and out["hyp_err2"].dtype == np.float64
    _check_table(name, out, tabs, H)
    assert (out["hyp_count"] >= 3).any() and (out["hyp_count"] == -2).any() and (out["hyp_count"] == -3).any()


# ------------------------------------------------------------------ 3. selection and final evaluation
@pytest.mark.parametrize("name", list(PLANTED_CASES))
def test_selection_and_final_evaluation(gpu, name):
    pairs, H, out, tabs = _case(gpu, name)
    _check_selection(pairs, out, tabs)


# ------------------------------------------------------------------ 4. planted poses
@pytest.mark.parametrize("name", list(PLANTED_CASES))
def test_planted_poses_are_recovered(gpu, name):
    pairs, H, out, tabs = _case(gpu, name)
    assert (out["status"] == 0).all()
    assert (out["success"] == 1).all() and (out["rte"] <= 2.0).all() and (out["rre"] <= 5.0).all(), (out["rte"], out["rre"])
    _check_metrics(pairs, out)


def test_edge_cases(gpu):
    E = edge_pairs()
    names = list(E)
    pairs = [E[k] for k in names]
    H = 2000
    out = _run(gpu, pairs, H, n_max=128)
    excused, _, unchecked = _check_matching(pairs, out["corr"], out["n_corr"])
    assert excused == 0 and unchecked == 0
    tabs = [ransac_f64(p[2], p[3], out["corr"][i, :out["n_corr"][i]], 0, i, H) for i, p in enumerate(pairs)]
    _check_table("edge cases", out, tabs, H)
    _check_selection(pairs, out, tabs)
    _check_metrics(pairs, out)
    st = dict(zip(names, out["status"].tolist()))
    for m in (0, 1, 2):
        assert st[f"n_corr_{m}"] == STATUS_FEW_CORR | STATUS_NO_MODEL and out["n_corr"][names.index(f"n_corr_{m}")] == m
    assert st["n_corr_3"] == 0 and out["success"][names.index("n_corr_3")] == 1
    for k in ("identical_keypoints", "collinear", "no_accepted_hypothesis"):
        assert st[k] == STATUS_NO_MODEL
    assert st["n1_ne_n2"] == 0 and st["duplicate_descriptors"] == 0
    # counts outside [0, n_max] are clipped on the device and reported
    F1, F2, K1, K2, n1, n2 = pad_batch(pairs[-2:], 128)
    big = gpu.register_pairs(_cu(F1), _cu(F2), _cu(K1), _cu(K2), n1=_cu(np.array([1000, -4], np.int32)), n2=_cu(n2),
                             ransac_max_it=500)
    torch.cuda.synchronize()
    assert (_np(big["status"]) & STATUS_CLIPPED).all() and _np(big["n_corr"])[1] == 0 and np.isfinite(_np(big["T"])).all()


# ------------------------------------------------------------------ 5. determinism and invariances
def test_determinism_and_invariances(gpu):
    pairs = [planted_pair(128, 700 + i, 0.2 + 0.05 * (i % 7)) for i in range(64)]
    H = 2000
    keys = ("T", "inliers", "fitness", "inlier_rmse", "correspondence_set", "best_t", "status", "corr", "n_corr", "rte", "rre",
            "success", "repeatability", "hyp_count", "hyp_err2")
    a, b = _run(gpu, pairs, H), _run(gpu, pairs, H)
    for k in keys:
        assert np.array_equal(a[k], b[k]), k                               # bitwise-equal reruns
    # a pair alone equals the pair inside the batch of 64 (the draws take the pair's id, not its position)
    for i in (0, 17, 63):
        one = _run(gpu, [pairs[i]], H, pids=[i])
        for k in keys:
            assert np.array_equal(one[k][0], a[k][i]), (k, i)
    # another chunking of the hypotheses (grid of 4 instead of 8 workgroups per pair): the same prefix table
    half = _run(gpu, pairs[:8], H // 2)
    assert np.array_equal(half["hyp_count"], a["hyp_count"][:8, :H // 2])
    assert np.array_equal(half["hyp_err2"], a["hyp_err2"][:8, :H // 2])
    # H not a multiple of the workgroup: the tail lanes stay out of the table and of the selection
    odd = _run(gpu, pairs[:8], 777)
    assert np.array_equal(odd["hyp_count"], a["hyp_count"][:8, :777])
    assert [best_rule(c, e) for c, e in zip(odd["hyp_count"], odd["hyp_err2"])] == odd["best_t"].tolist()
    # another seed: another table
    other = _run(gpu, pairs[:8], H, seed=1)
    assert (other["hyp_count"] != a["hyp_count"][:8]).mean() > 0.2
    # replay inside a captured graph (one stream, no parallel branches) equals the eager result
    F1, F2, K1, K2, n1, n2 = (_cu(x) for x in pad_batch(pairs))
    gt = _cu(np.stack([p[4] for p in pairs]))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = gpu.register_pairs(F1, F2, K1, K2, n1=n1, n2=n2, T_gt=gt, ransac_max_it=H, debug=True)
    for k in keys:
        out[k].zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in keys:
        assert np.array_equal(_np(out[k]), a[k]), k


# ------------------------------------------------------------------ 6. end to end behind the descriptor path
def test_end_to_end_from_scans(gpu):
    from egonn_amd.synth import lidar_scan, seeded_state_dict
    from tests.test_registration_host import rot_zyx
    mp = gpu.ModelParams(model="egonn", coordinates="cartesian", quantization_step=0.1)
    model = gpu.model_factory(mp)
    sd = seeded_state_dict(7, {k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to("cuda:0").eval()
    pc = lidar_scan(2, n_points=20000).astype(np.float64)
    T_gt = np.eye(4)
    T_gt[:3, :3], T_gt[:3, 3] = rot_zyx(np.deg2rad(10.0), 0.0, 0.0), [2.0, 1.0, 0.0]
    pc2 = pc @ T_gt[:3, :3].T + T_gt[:3, 3]
    ex = gpu.DescriptorExtractor(model, n_k=128)
    y = ex.extract([torch.from_numpy(pc.astype(np.float32)), torch.from_numpy(pc2.astype(np.float32))])
    kp, desc, cnt = y["keypoints"], y["descriptors"], y["count"].to(torch.int32)
    H = 4000
    out = gpu.register_pairs(desc[0:1], desc[1:2], kp[0:1], kp[1:2], n1=cnt[0:1], n2=cnt[1:2], T_gt=_cu(T_gt[None]),
                             ransac_max_it=H, debug=True)
    torch.cuda.synchronize()
    assert out["T"].shape == (1, 4, 4) and out["T"].dtype == torch.float64 and out["inliers"].dtype == torch.int32
    assert out["fitness"].dtype == torch.float64 and out["correspondence_set"].shape == (1, 128, 2)
    assert out["hyp_count"].shape == (1, H) and out["success"].dtype == torch.int32
    o = {k: _np(v) for k, v in out.items() if k != "_keep"}
    for k in ("T", "fitness", "inlier_rmse", "rte", "rre", "repeatability", "hyp_err2"):
        assert np.isfinite(o[k]).all(), k
    assert not o["status"][0] & (STATUS_CLIPPED | STATUS_FEW_CORR)
    n1, n2 = int(cnt[0]), int(cnt[1])
    pair = (_np(desc[0])[:n1], _np(desc[1])[:n2], _np(kp[0])[:n1], _np(kp[1])[:n2], T_gt)
    excused, total, unchecked = _check_matching([pair], o["corr"], o["n_corr"])
    print(f"[registration] end to end: excused matching rows {excused} of {total}, unchecked pairs {unchecked}")
    tabs = [ransac_f64(pair[2], pair[3], o["corr"][0, :o["n_corr"][0]], 0, 0, H)]
    _check_table("end to end", o, tabs, H)
    _check_selection([pair], o, tabs)
    _check_metrics([pair], o)
    print(f"[registration] end to end (seeded weights): n_corr {o['n_corr'][0]}, inliers {o['inliers'][0]}, "
          f"rte {o['rte'][0]:.3f} m, rre {o['rre'][0]:.3f} deg, repeatability {o['repeatability'][0]:.3f}")
    # the one-pair surface with the reference's names gives the same answer
    r = gpu.get_ransac_result(desc[0, :n1], desc[1, :n2], kp[0, :n1], kp[1, :n2], ransac_max_it=H)
    assert np.array_equal(r.transformation, o["T"][0]) and len(r.correspondence_set) == o["inliers"][0]
    assert r.fitness == o["fitness"][0] and r.inlier_rmse == o["inlier_rmse"][0]
    assert gpu.calculate_repeatability(kp[0, :n1], kp[1, :n2], T_gt, 0.5) == o["repeatability"][0]


def test_evaluate_local_bookkeeping(gpu):
    """evaluate_local against the same bookkeeping done by hand on register_pairs' outputs; the 20 m gate drops a query"""
    pairs = planted_case("n128_out30")
    q = [{"keypoints": torch.from_numpy(p[2]), "features": torch.from_numpy(p[0])} for p in pairs]
    m = [{"keypoints": torch.from_numpy(p[3]), "features": torch.from_numpy(p[1])} for p in pairs][::-1]
    nn = np.arange(len(pairs))[::-1].copy()[:, None]
    gt = np.stack([p[4] for p in pairs])
    gt[1, :3, 3] += 10.0                                                   # one failure by construction
    dist = np.full((len(pairs), 1), 5.0)
    dist[2] = 25.0                                                         # beyond the 20 m gate: skipped
    res = gpu.evaluate_local(q, m, nn, gt, n_k=(128, 64), euclid_dist=dist, ransac_max_it=3000)
    assert set(res) == {128, 64}
    keep = [i for i in range(len(pairs)) if i != 2]
    out = _run(gpu, [pairs[i][:4] + (gt[i],) for i in keep], 3000, pids=keep)
    suc = out["success"].astype(bool)
    r = res[128]
    assert suc.sum() == len(keep) - 1 and r["success"] == suc.mean()
    assert r["rte"] == out["rte"][suc].mean() and r["rre"] == out["rre"][suc].mean()
    assert r["success_inliers"] == out["inliers"][suc].mean() and r["failure_inliers"] == out["inliers"][~suc].mean()
    assert r["repeatability"] == out["repeatability"].mean() == r["repeatability_refined"]
    # one batched device measurement divided by the pairs: a positive time, and by definition no per-pair spread
    assert r["t_ransac"] > 0 and r["t_ransac_sd"] == 0.0
    assert 0.0 <= res[64]["success"] <= 1.0 and set(res[64]) == set(r)


# ------------------------------------------------------------------ 7. argument checks
def test_argument_checks(gpu):
    from egonn_amd._lib import EgonnError, load
    z = lambda *s: torch.zeros(s, device="cuda")                           # noqa: E731
    for f, k, kw in ((z(1, 257, 128), z(1, 257, 3), {}), (z(1, 64, 30), z(1, 64, 3), {}),
                     (z(1, 64, 128), z(1, 64, 3), {"ransac_max_it": 0}), (z(1, 64, 128), z(1, 64, 3), {"ransac_max_it": -7})):
        with pytest.raises(EgonnError) as e:
            gpu.register_pairs(f, f, k, k, **kw)
        assert e.value.code == 1                                           # EGONN_STATUS_INVALID, nothing launched
    lib = load()
    f, k, n = z(1, 64, 128), z(1, 64, 3), torch.zeros(1, dtype=torch.int32, device="cuda")
    c = torch.zeros((1, 64, 2), dtype=torch.int32, device="cuda")
    s = torch.zeros(64, dtype=torch.int64, device="cuda")
    P = lambda t: t.data_ptr()                                             # noqa: E731
    nb = lib.egonn_match_mutual_scratch_bytes(1, 64)
    ms = torch.zeros(nb // 8, dtype=torch.int64, device="cuda")
    assert nb == (1 + 2) * 64 * 12
    assert lib.egonn_match_mutual(P(f), None, P(n), P(n), 1, 64, 128, P(c), P(n), P(ms), nb, None) == 1
    assert lib.egonn_match_mutual(P(f), P(f), P(n), P(n), 1, 64, 128, None, P(n), P(ms), nb, None) == 1
    assert lib.egonn_match_mutual(P(f), P(f), P(n), P(n), 1, 64, 128, P(c), P(n), None, nb, None) == 1
    assert lib.egonn_match_mutual(P(f), P(f), P(n), P(n), 1, 64, 128, P(c), P(n), P(ms), nb - 1, None) == 1
    assert lib.egonn_ransac_pairs(P(k), P(k), P(n), P(n), None, P(n), None, 1, 64, 100, 0, 0.5, P(s), 512, None, None, None) == 1
    assert lib.egonn_ransac_pairs(P(k), P(k), P(n), P(n), P(c), P(n), None, 1, 64, 100, 0, 0.5, None, 512, None, None, None) == 1
    assert lib.egonn_ransac_pairs(P(k), P(k), P(n), P(n), P(c), P(n), None, 1, 64, 10000, 0, 0.5, P(s), 512, None, None, None) == 1
    assert lib.egonn_registration_finish(P(k), P(k), P(n), P(n), P(c), P(n), None, 1, 64, 100, 0, 0.5, P(s), 512, None, 0.5, None,
                                         P(n), P(s), P(s), None, None, None, None, None, None, None, None) == 1
    assert lib.egonn_registration_finish(P(k), P(k), P(n), P(n), None, None, None, 1, 64, 0, 0, 0.5, None, 0, None, 0.5, None,
                                         None, None, None, None, None, None, None, None, None, None, None) == 1
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 8. one tail behind both methods (csrc/pair_eval.h)
TAIL_KEYS = ("T", "inliers", "fitness", "inlier_rmse", "correspondence_set", "rte", "rre", "success")
TAIL_H = 500


def _pad_clipped(pairs, n_max):
    """pad_batch to n_max rows; a pair with more rows keeps its raw counts, which the device clips and reports"""
    F1, F2, K1, K2, _, _ = pad_batch([tuple(x[:n_max] for x in p[:4]) for p in pairs], n_max)
    return F1, F2, K1, K2, np.array([len(p[2]) for p in pairs], np.int32), np.array([len(p[3]) for p in pairs], np.int32)


def _both_methods(gpu, pairs, n_max):
    F1, F2, K1, K2, n1, n2 = (_cu(x) for x in _pad_clipped(pairs, n_max))
    gt = _cu(np.stack([p[4] for p in pairs]))
    out = {m: gpu.register_pairs(F1, F2, K1, K2, n1=n1, n2=n2, T_gt=gt, ransac_max_it=TAIL_H, method=m) for m in ("ransac", "spectral")}
    rep = gpu.registration.repeatability_pairs(K1, K2, gt, 0.5, n1, n2)
    torch.cuda.synchronize()
    return {m: {k: _np(v) for k, v in o.items() if not k.startswith("_")} for m, o in out.items()}, _np(rep), _np(n1), _np(n2)


@pytest.mark.parametrize("n_max", [128, 256])
def test_repeatability_is_one_tail_behind_three_entry_points(gpu, n_max):
    """register_pairs by RANSAC (256 lanes), by the spectral check (128 lanes at n_max 128, 256 beyond) and repeatability_pairs
    (no correspondences) reach the same pair_tail: the same bits, counts of 0 and 1 and a count clipped at n_max included"""
    pairs = list(edge_pairs().values()) + planted_case("n256_n2_200")
    out, rep, n1, _ = _both_methods(gpu, pairs, n_max)
    assert 0 in n1 and 1 in n1 and (n1 > n_max).any() == (n_max == 128)
    assert ((out["ransac"]["status"] & STATUS_CLIPPED) != 0).tolist() == (n1 > n_max).tolist()
    assert rep.dtype == np.float64 and rep.tobytes() == out["ransac"]["repeatability"].tobytes()
    assert rep.tobytes() == out["spectral"]["repeatability"].tobytes()
    want = [repeatability_f64(p[2][:n_max], p[3][:n_max], p[4], 0.5) for p in pairs]
    assert np.abs(rep - want).max() <= 1e-12


def _modelless_edge_pairs():
    """names of the edge pairs that both float64 restatements end without a model (FEW_CORR or NO_MODEL): chosen on the CPU"""
    from tests.spectral_ref import spectral_f64
    from tests.test_registration_host import match_f64, register_f64
    none = STATUS_FEW_CORR | STATUS_NO_MODEL
    names = []
    for name, (f1, f2, k1, k2, T) in edge_pairs().items():
        a = register_f64(f1, f2, k1, k2, T, H=TAIL_H)
        b = spectral_f64(k1, k2, match_f64(f1, f2)[0], 128, T)
        if a["status"] & none and b["status"] & none:
            names.append(name)
    return names


def test_modelless_pairs_end_alike_in_both_methods(gpu):
    """without a model the shared outputs do not depend on the method: identity, 0 inliers, the metrics of the identity"""
    E, names = edge_pairs(), _modelless_edge_pairs()
    print(f"[registration] pairs without a model in both restatements: {names}")
    assert len(names) >= 2
    out, _, _, _ = _both_methods(gpu, [E[k] for k in names], 128)
    for m in out:
        assert ((out[m]["status"] & (STATUS_FEW_CORR | STATUS_NO_MODEL)) != 0).all(), m
    for k in TAIL_KEYS:
        assert out["ransac"][k].dtype == out["spectral"][k].dtype and out["ransac"][k].tobytes() == out["spectral"][k].tobytes(), k
    assert np.array_equal(out["ransac"]["T"], np.broadcast_to(np.eye(4), (len(names), 4, 4))) and not out["ransac"]["inliers"].any()

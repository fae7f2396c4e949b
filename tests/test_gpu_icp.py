"""GPU tests of the ICP refinement (run with -m gpu on an MI355X) against the float64 restatement of tests/test_icp_host.py:
the downsample voxel by voxel, every round of every committed case teacher-forced from the device's trace, the free-running
result, the invariances (runs, batch, graph), the edges and evaluate_local end to end.

Measured on an MI355X (test_band_measurement / test_free_running print them):
  MEASURED_COORD_DIFF  largest displacement of a point of the +-114 m box between the device's T_k+1 and icp_step_f64 on the
                       device's correspondences under the device's T_k, over every round of every committed case.  (The
                       restatement transforms the source in the device's operation order, so under the same T_k the
                       transformed coordinates themselves are equal; the rigid fit is where the two routes differ.)
  MEASURED_FREE_DIFF   the same displacement between the device's final T and the free-running restatement's.
BAND (tests/test_icp_host.py) must be >= 100 x MEASURED_COORD_DIFF and <= 1e-6 m; FREE_TOL must be >= 10 x
MEASURED_FREE_DIFF and <= 1 mm.  The tests assert these inequalities on the values they measure."""
import numpy as np
import pytest
import torch

from tests.test_icp_host import (BAND, ICP_CASES, ICP_EMPTY, ICP_FEW_CORR, ICP_MAX_ITER, ICP_RANGE, NEAR_ROW_CAP, box_displacement,
                                 downsample_f64, evaluate_f64, icp_case, icp_case_result, icp_f64, icp_step_f64, stop_rule)

pytestmark = pytest.mark.gpu

MEASURED_COORD_DIFF = 2.188e-13   # metres, as printed by test_band_measurement on an MI355X (84 rounds of the 6 cases)
MEASURED_FREE_DIFF = 3.143e-13    # metres, the largest value printed by test_free_running on an MI355X
FREE_TOL = 1e-6               # metres: tolerance on the final T as a displacement of the box; <= 1 mm = 1/100 of the voxel edge
MAX_DIST = 1.2
SMALL = [n for n in ICP_CASES if n != "scan_50k"]


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


def _offsets(clouds):
    off = np.zeros(len(clouds) + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in clouds])
    return off


def _cat(clouds, dtype):
    return np.concatenate([np.asarray(c, dtype).reshape(-1, 3) for c in clouds]) if clouds else np.zeros((0, 3), dtype)


def _downsample(gpu, clouds, voxel=0.1, crop=None):
    out = gpu.voxel_downsample(_cu(_cat(clouds, np.float32)), _cu(_offsets(clouds)), voxel, crop)
    torch.cuda.synchronize()
    off = _np(out["offsets"])
    pts, cnt = _np(out["points"]), _np(out["counts"])
    return [pts[off[c]:off[c + 1]] for c in range(len(clouds))], [cnt[off[c]:off[c + 1]] for c in range(len(clouds))], \
        _np(out["status"]), off


def _icp(gpu, srcs, tgts, T_init=None, max_iteration=200, debug=True, max_dist=MAX_DIST):
    """srcs / tgts: lists of (n,3) float64 clouds -> numpy dict (corr split per pair)"""
    so, to = _offsets(srcs), _offsets(tgts)
    out = gpu.icp_pairs(_cu(_cat(srcs, np.float64)), _cu(so), _cu(_cat(tgts, np.float64)), _cu(to),
                        None if T_init is None else _cu(np.asarray(T_init, np.float64)), max_dist, max_iteration, debug)
    torch.cuda.synchronize()
    r = {k: _np(v) for k, v in out.items() if not k.startswith("_")}
    if debug:
        r["corr"] = [r["corr"][so[p]:so[p + 1]] for p in range(len(srcs))]
    return r


def _check_downsample(pts_dev, cnt_dev, raw, voxel, crop=None):
    q, cnt, _, st = downsample_f64(raw, voxel, crop)
    assert st == 0 and len(pts_dev) == len(q), (len(pts_dev), len(q))
    assert np.array_equal(cnt_dev, cnt)
    if len(q):
        bound = (cnt + 1) * 2.0 ** -53 * np.abs(np.asarray(raw, np.float64)).max()
        assert (np.abs(pts_dev - q).max(1) <= bound).all(), np.abs(pts_dev - q).max()
    return bool(np.array_equal(pts_dev, q))


# ------------------------------------------------------------------ 1. downsample
def test_downsample_matches_restatement(gpu):
    clouds = []
    for name in ICP_CASES:
        c = icp_case(name)
        clouds += [c["raw_src"], c["raw_tgt"]]
    pts, cnt, status, off = _downsample(gpu, clouds)
    assert (status == 0).all() and off[0] == 0
    same = [_check_downsample(pts[i], cnt[i], clouds[i], 0.1) for i in range(len(clouds))]
    print("clouds whose means equal the restatement's bit for bit:", sum(same), "of", len(same))
    assert off[-1] == sum(len(p) for p in pts) and (np.diff(off) == [len(downsample_f64(c)[0]) for c in clouds]).all()
    # dense voxels (many points per mean) and a cloud in a batch equals the cloud alone
    rng = np.random.default_rng(3)
    dense = [rng.uniform(-1, 1, size=(n, 3)).astype(np.float32) * np.float32(s) for n, s in ((5000, 1.0), (1, 1.0), (3000, 80.0))]
    pts, cnt, status, _ = _downsample(gpu, dense, 0.5)
    for i in range(3):
        _check_downsample(pts[i], cnt[i], dense[i], 0.5)
    assert max(c.max() for c in cnt) > 10
    alone, cnt_alone, _, _ = _downsample(gpu, dense[2:3], 0.5)
    assert np.array_equal(alone[0], pts[2]) and np.array_equal(cnt_alone[0], cnt[2])


def test_downsample_where_the_sort_loops_wrap(gpu):
    """clouds of exactly one tile of the 64-bit segmented sort (2048 keys) less one, one tile, one tile and a key, and of 9 and
    11 tiles (16 385 and 20 481 points: the scatter kernel sums the histogram rows of a cloud's earlier tiles eight at a time,
    8 rows fill one round, 10 need a second), many points per voxel, and a crop that drops a share of every cloud: the
    dropped points carry the key ~0 and must sort behind every kept point of their own cloud.  The voxel means are sums in
    input order: a sort that was not stable would move them beyond the bound of _check_downsample."""
    rng = np.random.default_rng(16385)
    sizes = (2047, 2048, 2049, 16385, 20481)
    clouds = [rng.uniform(-2, 2, size=(n, 3)).astype(np.float32) for n in sizes]
    crop = (-1.2, 1.6, None, 1.5, float("nan"), None)
    pts, cnt, status, off = _downsample(gpu, clouds, 0.5, crop)
    assert (status == 0).all() and off[0] == 0 and off[-1] == sum(len(p) for p in pts)
    for i, n in enumerate(sizes):
        _check_downsample(pts[i], cnt[i], clouds[i], 0.5, crop)
        assert 0.3 * n < cnt[i].sum() < 0.7 * n                  # a share of the cloud is cropped away, a share is kept
    assert cnt[0].max() > 3 and cnt[3].max() > 30                # many points per voxel
    for i in (3, 4):                                             # in the batch = alone, bit for bit
        alone, cnt_alone, st, _ = _downsample(gpu, clouds[i:i + 1], 0.5, crop)
        assert st.tolist() == [0] and np.array_equal(alone[0], pts[i]) and np.array_equal(cnt_alone[0], cnt[i])


def test_downsample_where_the_block_scan_wraps(gpu):
    """one cloud of 65 537 points is 257 workgroups: in the one-workgroup scan of their head counts a thread owns two counters.
    And a batch of (256, 0, 512, 255, 1) points: every cloud boundary lies on a multiple of 256 or one short of it and the
    total is exactly four workgroups, so the end of the last cloud lies behind the last workgroup's counter"""
    rng = np.random.default_rng(65537)
    big = rng.uniform(-40, 40, size=(65537, 3)).astype(np.float32)
    pts, cnt, status, off = _downsample(gpu, [big], 0.5)
    assert status.tolist() == [0] and off.tolist() == [0, len(pts[0])] and len(pts[0]) > 40000
    _check_downsample(pts[0], cnt[0], big, 0.5)
    clouds = [rng.uniform(-2, 2, size=(n, 3)).astype(np.float32) for n in (256, 0, 512, 255, 1)]
    pts, cnt, status, off = _downsample(gpu, clouds, 0.5)
    assert (status == 0).all() and off[0] == 0 and off[-1] == sum(len(p) for p in pts) and len(pts[1]) == 0
    for i, c in enumerate(clouds):
        _check_downsample(pts[i], cnt[i], c, 0.5)
    assert np.array_equal(pts[4], clouds[4].astype(np.float64)) and cnt[4].tolist() == [1]


def test_downsample_edges(gpu):
    p = np.array([[0.0, 0, 0], [0.04, 0.04, 0.04], [0.06, 0, 0], [1.0, 1.0, 1.0], [-0.3, 5, 5], [0.5, 0.2, 0.1]], np.float32)
    # crop: the point exactly on min_x (0.0) is dropped, the one exactly on max_x (1.0) is kept; NaN / None = no bound
    crop = (0.0, 1.0, None, None, float("nan"), None)
    pts, cnt, status, off = _downsample(gpu, [p, p[:0], p[3:4], p], crop=crop)
    assert status.tolist() == [0, 0, 0, 0] and np.diff(off).tolist() == [len(pts[0]), 0, 1, len(pts[0])]
    _check_downsample(pts[0], cnt[0], p, 0.1, crop)
    assert cnt[0].sum() == 4 and (pts[0] == 1.0).all(1).any() and not (pts[0] == 0.0).all(1).any()
    assert np.array_equal(pts[2], p[3:4].astype(np.float64)) and cnt[2].tolist() == [1]          # single point: itself
    assert np.array_equal(pts[3], pts[0])
    # everything cropped away: an empty cloud
    pts, _, status, off = _downsample(gpu, [p], crop=(10.0, None, None, None, None, None))
    assert len(pts[0]) == 0 and off.tolist() == [0, 0] and status.tolist() == [0]
    # no points at all
    pts, _, status, off = _downsample(gpu, [p[:0]])
    assert off.tolist() == [0, 0] and status.tolist() == [0]
    # an index beyond 21 bits: RANGE, nothing written for that cloud, its neighbours untouched
    far = np.array([[0, 0, 0], [0.1 * 2 ** 21 + 1, 0, 0]], np.float32)
    pts, cnt, status, off = _downsample(gpu, [p, far, p[3:]])
    assert status.tolist() == [0, ICP_RANGE, 0] and len(pts[1]) == 0
    _check_downsample(pts[0], cnt[0], p, 0.1)
    _check_downsample(pts[2], cnt[2], p[3:], 0.1)
    nan = np.array([[0, 0, 0], [np.nan, 0, 0]], np.float32)
    assert _downsample(gpu, [nan])[2].tolist() == [ICP_RANGE]


# ------------------------------------------------------------------ 2. every round, teacher-forced from the device's trace
_TF = {}


def _teacher_forced(gpu, name):
    if name in _TF:
        return _TF[name]
    c = icp_case(name)
    src, tgt = c["src"], c["tgt"]
    dev = _icp(gpu, [src], [tgt], c["T_init"][None], c["max_iteration"])
    K = int(dev["iterations"][0])
    rec = dict(dev=dev, K=K, coord_diff=0.0, excused=0, rows=0)
    prev = None
    for k in range(K + 1):
        Tk = dev["T_trace"][0, k]
        ev = evaluate_f64(src, tgt, Tk, MAX_DIST)
        near = (ev["gap"] <= BAND) | (ev["thr"] <= BAND)
        assert near.mean() <= NEAR_ROW_CAP, (name, k, near.mean())
        rec["excused"] += int(near.sum())
        rec["rows"] += len(src)
        # the device's j(i) under T_k: one evaluation (no round) started from T_k
        one = _icp(gpu, [src], [tgt], Tk[None], 0)
        j_dev = one["corr"][0]
        assert np.array_equal(j_dev[~near], ev["j"][~near]), (name, k, int((j_dev != ev["j"])[~near].sum()))
        n_dev, sum_dev, stop_dev = dev["eval_trace"][0, k]
        assert abs(n_dev - ev["n_corr"]) <= near.sum() and one["eval_trace"][0, 0, 0] == n_dev, (name, k, n_dev, ev["n_corr"])
        if near.sum() == 0:
            assert n_dev == ev["n_corr"] and abs(sum_dev - ev["sum_d2"]) <= 1e-12 * max(ev["sum_d2"], 1.0)
        stop, bit, near_stop = stop_rule(k, ev, prev, c["max_iteration"])
        assert not near_stop and bool(stop_dev) == stop, (name, k, stop_dev, stop)
        if not stop:
            T_next = icp_step_f64(src, tgt, Tk, j_dev)
            d = box_displacement(T_next, dev["T_trace"][0, k + 1])
            rec["coord_diff"] = max(rec["coord_diff"], d)
            assert d <= BAND, (name, k, d)
        else:
            assert k == K and int(dev["status"][0]) == bit
            assert np.array_equal(dev["T"][0], Tk) and not dev["T_trace"][0, k + 1:].any()
        prev = ev
    _TF[name] = rec
    return rec


@pytest.mark.parametrize("name", list(ICP_CASES))
def test_every_round_teacher_forced(gpu, name):
    rec = _teacher_forced(gpu, name)
    print(name, "rounds", rec["K"], "largest T_k+1 difference on the box [m]", rec["coord_diff"], "excused rows", rec["excused"],
          "of", rec["rows"])
    assert rec["excused"] <= NEAR_ROW_CAP * rec["rows"]


def test_band_measurement(gpu):
    worst = max(_teacher_forced(gpu, name)["coord_diff"] for name in ICP_CASES)
    print("MEASURED_COORD_DIFF =", worst)
    assert BAND >= 100.0 * worst and BAND >= 100.0 * MEASURED_COORD_DIFF and BAND <= 1e-6


# ------------------------------------------------------------------ 3. the free-running result
@pytest.mark.parametrize("name", list(ICP_CASES))
def test_free_running(gpu, name):
    c, ref = icp_case(name), icp_case_result(name)
    dev = _teacher_forced(gpu, name)["dev"]
    d = box_displacement(dev["T"][0], ref["T"])
    print(name, "MEASURED_FREE_DIFF candidate [m]", d, "iterations", int(dev["iterations"][0]), ref["iterations"], "fitness",
          dev["fitness"][0], ref["fitness"], "rmse", dev["inlier_rmse"][0], ref["rmse"])
    assert 10.0 * MEASURED_FREE_DIFF <= FREE_TOL <= 1e-3 and 10.0 * d <= FREE_TOL
    assert not any(ref["near_stop"]) and int(dev["iterations"][0]) == ref["iterations"] and int(dev["status"][0]) == ref["status"]
    n = len(c["src"])
    assert abs(dev["fitness"][0] - ref["fitness"]) * n <= max(ref["near_rows"]) * n + 1e-6
    assert abs(dev["inlier_rmse"][0] - ref["rmse"]) <= 1e-9
    # the point of it: nearer to the planted pose than the init
    from tests.test_icp_host import pose_error
    r0, t0 = pose_error(c["T_init"], c["T_planted"])
    r1, t1 = pose_error(dev["T"][0], c["T_planted"])
    assert r1 < r0 and t1 < t0


# ------------------------------------------------------------------ 4. invariances
def _batch16():
    names = [SMALL[i % len(SMALL)] for i in range(16)]
    cs = [icp_case(n) for n in names]
    return names, [c["src"] for c in cs], [c["tgt"] for c in cs], np.stack([c["T_init"] for c in cs])


KEYS = ("T", "fitness", "inlier_rmse", "iterations", "status", "T_trace", "eval_trace")


def test_runs_and_batches_are_bitwise_equal(gpu):
    names, srcs, tgts, T0 = _batch16()
    a = _icp(gpu, srcs, tgts, T0)
    b = _icp(gpu, srcs, tgts, T0)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    assert all(np.array_equal(x, y) for x, y in zip(a["corr"], b["corr"]))
    assert len(set(a["iterations"].tolist())) > 1                    # pairs stop at different rounds inside one call
    for pos in (0, 3, 11, 15):                                       # alone == inside the batch of 16, at any position
        one = _icp(gpu, srcs[pos:pos + 1], tgts[pos:pos + 1], T0[pos:pos + 1])
        for k in KEYS:
            assert np.array_equal(one[k][0], a[k][pos]), (k, pos)
        assert np.array_equal(one["corr"][0], a["corr"][pos])
    # the same pair at another batch position (positions 0 and 5 hold the same case)
    assert names[0] == names[5]
    for k in KEYS:
        assert np.array_equal(a[k][0], a[k][5]), k
    # and it is the single-pair run of the teacher-forced test
    dev = _teacher_forced(gpu, names[0])["dev"]
    assert np.array_equal(dev["T"][0], a["T"][0]) and dev["iterations"][0] == a["iterations"][0]


EDGE_SIZES = (300, 0, 256, 257, 1)     # source points: an empty pair between two others, exactly one workgroup, one point more, one point


def edge_batch():
    """One pair per EDGE_SIZES entry, the smallest shapes at which the flat grid's indexing can go wrong: 400 points spread over
    the target of scan_8k, and as sources their first n points moved off by a small rigid motion (so every source point has its
    correspondence and the loop runs)."""
    tgt = icp_case("scan_8k")["tgt"][::20][:400]
    a = 0.004
    M = np.array([[np.cos(a), -np.sin(a), 0.0, 0.05], [np.sin(a), np.cos(a), 0.0, -0.03], [0.0, 0.0, 1.0, 0.02], [0.0, 0.0, 0.0, 1.0]])
    T0 = np.stack([np.linalg.inv(M)] * len(EDGE_SIZES))
    T0[3, :3, 3] += 0.01                                               # not every pair from the same start
    return [tgt[:n] @ M[:3, :3].T + M[:3, 3] for n in EDGE_SIZES], [tgt] * len(EDGE_SIZES), T0


def test_edge_sizes_in_one_batch_equal_the_pair_alone(gpu):
    srcs, tgts, T0 = edge_batch()
    a = _icp(gpu, srcs, tgts, T0)
    assert a["status"][1] == ICP_EMPTY and a["status"][4] == ICP_FEW_CORR and (a["iterations"][[0, 2, 3]] >= 1).all()
    for pos in range(len(srcs)):                                       # each alone is also the single-pair batch
        one = _icp(gpu, srcs[pos:pos + 1], tgts[pos:pos + 1], T0[pos:pos + 1])
        for k in KEYS:
            assert np.array_equal(one[k][0], a[k][pos]), (k, pos)
        assert np.array_equal(one["corr"][0], a["corr"][pos]), pos


def test_graph_replay_equals_eager(gpu):
    _, srcs, tgts, T0 = _batch16()
    srcs, tgts, T0 = srcs[:4], tgts[:4], T0[:4]
    eager = _icp(gpu, srcs, tgts, T0, max_iteration=40)
    s, so = _cu(_cat(srcs, np.float64)), _cu(_offsets(srcs))
    t, to = _cu(_cat(tgts, np.float64)), _cu(_offsets(tgts))
    ti = _cu(T0)
    gpu.icp_pairs(s, so, t, to, ti, MAX_DIST, 40, True)               # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = gpu.icp_pairs(s, so, t, to, ti, MAX_DIST, 40, True)
    for k in KEYS:
        out[k].zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in KEYS:
        assert np.array_equal(_np(out[k]), eager[k]), k
    assert np.array_equal(_np(out["corr"]), np.concatenate(eager["corr"]))


def test_default_init_and_zero_rounds(gpu):
    c = icp_case("converged_init_5k")
    src = c["src"] @ c["T_init"][:3, :3].T + c["T_init"][:3, 3]       # moved close to the target: identity is a fair init
    a = _icp(gpu, [src], [c["tgt"]], None)
    b = _icp(gpu, [src], [c["tgt"]], np.eye(4)[None])
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    assert a["status"][0] == 0 and a["iterations"][0] >= 1
    z = _icp(gpu, [c["src"]], [c["tgt"]], c["T_init"][None], max_iteration=0)
    ev = evaluate_f64(c["src"], c["tgt"], c["T_init"], MAX_DIST)
    assert np.array_equal(z["T"][0], c["T_init"]) and z["iterations"][0] == 0 and z["status"][0] == ICP_MAX_ITER
    assert z["T_trace"].shape == (1, 1, 4, 4) and np.array_equal(z["T_trace"][0, 0], c["T_init"])
    near = int(((ev["gap"] <= BAND) | (ev["thr"] <= BAND)).sum())
    assert abs(z["fitness"][0] * len(c["src"]) - ev["n_corr"]) <= near + 1e-6 and abs(z["inlier_rmse"][0] - ev["rmse"]) <= 1e-9
    assert np.array_equal(z["corr"][0] >= 0, ev["j"] >= 0) or near > 0


# ------------------------------------------------------------------ 5. edges
def test_edges(gpu):
    c = icp_case("scan_8k")
    src, tgt, T0 = c["src"], c["tgt"], c["T_init"]
    e = np.zeros((0, 3))
    r = _icp(gpu, [src, e, src, e], [tgt, tgt, e, e], np.stack([T0] * 4))
    assert r["status"].tolist()[1:] == [ICP_EMPTY] * 3 and r["status"][0] == 0
    for p in (1, 2, 3):
        assert np.array_equal(r["T"][p], T0) and r["fitness"][p] == 0.0 and r["inlier_rmse"][p] == 0.0 and r["iterations"][p] == 0
    alone = _icp(gpu, [src], [tgt], T0[None])
    assert np.array_equal(alone["T"][0], r["T"][0])                  # empty neighbours change nothing
    assert _icp(gpu, [e], [e], None)["status"].tolist() == [ICP_EMPTY]
    # farther apart than max_dist: no correspondence, FEW_CORR with T = init; a source far outside the target's grid
    far = np.eye(4)
    far[:3, 3] = [500.0, 0.0, 300.0]
    r = _icp(gpu, [src, src[:50] * 1e-3], [tgt, tgt[:40] * 1e-3 + 5.0], np.stack([far, np.eye(4)]))
    assert r["status"].tolist() == [ICP_FEW_CORR, ICP_FEW_CORR] and r["iterations"].tolist() == [0, 0]
    assert np.array_equal(r["T"][0], far) and np.array_equal(r["T"][1], np.eye(4)) and (r["fitness"] == 0).all()
    assert (r["corr"][0] == -1).all() and (r["corr"][1] == -1).all()
    # exactly two correspondences: still FEW_CORR, with their evaluation
    two = _icp(gpu, [np.array([[0.0, 0, 0], [10.0, 0, 0], [50.0, 50, 0]])], [np.array([[0.1, 0, 0], [10.0, 0.2, 0], [0.0, 90, 0]])])
    assert two["status"][0] == ICP_FEW_CORR and two["fitness"][0] == 2 / 3 and two["corr"][0].tolist() == [0, 1, -1]
    assert abs(two["inlier_rmse"][0] - np.sqrt((0.01 + 0.04) / 2)) < 1e-15
    # a round limit too small for a far init
    f = icp_case("far_init_7k")
    cut = _icp(gpu, [f["src"]], [f["tgt"]], f["T_init"][None], max_iteration=3)
    ref = icp_f64(f["src"], f["tgt"], f["T_init"], MAX_DIST, 3)
    assert cut["status"][0] == ICP_MAX_ITER == ref["status"] and cut["iterations"][0] == 3
    assert box_displacement(cut["T"][0], ref["T"]) <= FREE_TOL
    full = _teacher_forced(gpu, "far_init_7k")["dev"]
    assert np.array_equal(cut["T_trace"][0], full["T_trace"][0, :4])   # the first rounds do not depend on the limit
    # a tie between two target points goes to the lowest index; the threshold is strict
    tie = _icp(gpu, [np.array([[0.0, 0, 0], [5.0, 0, 0]])], [np.array([[0.0, 0.5, 0], [0.0, -0.5, 0], [5.0, 1.0, 0]])],
               max_iteration=0, max_dist=1.0)
    assert tie["corr"][0].tolist() == [0, -1] and tie["fitness"][0] == 0.5


def test_icp_single_pair_wrapper(gpu):
    c = icp_case("scan_8k")
    T, fit, rmse = gpu.icp(c["raw_src"], c["raw_tgt"], c["T_init"])
    dev = _teacher_forced(gpu, "scan_8k")["dev"]
    assert T.shape == (4, 4) and T.dtype == np.float64 and isinstance(fit, float) and isinstance(rmse, float)
    # the wrapper downsamples on the device: equal to the run on the restatement's downsample up to the means' rounding
    assert box_displacement(T, dev["T"][0]) <= FREE_TOL and abs(fit - dev["fitness"][0]) <= 1e-3
    with pytest.raises(NotImplementedError):
        gpu.icp(c["raw_src"], c["raw_tgt"], point2plane=True)


# ------------------------------------------------------------------ 6. evaluate_local end to end
def test_evaluate_local_refined(gpu):
    from egonn_amd.synth import planted_scan_pair
    from tests.test_registration_host import metrics_f64, planted_case
    pairs = planted_case("n128_out30")[:4]
    q = [{"keypoints": torch.from_numpy(p[2]), "features": torch.from_numpy(p[0])} for p in pairs]
    m = [{"keypoints": torch.from_numpy(p[3]), "features": torch.from_numpy(p[1])} for p in pairs]
    gt = np.stack([p[4] for p in pairs])
    qc, mc = [], []
    for i, T in enumerate(gt):                       # clouds that move by the pair's T_gt (ZYX angles of its rotation)
        R = T[:3, :3]
        ypr = (np.arctan2(R[1, 0], R[0, 0]), -np.arcsin(R[2, 0]), np.arctan2(R[2, 1], R[2, 2]))
        s, t, Tp, _ = planted_scan_pair(40 + i, 6000, translation=T[:3, 3], yaw_pitch_roll=ypr)
        assert np.abs(Tp - T).max() < 1e-9
        qc.append(s)
        mc.append(t)
    gt[1, :3, 3] += 10.0                             # one failure against T_gt; ICP from there finds nothing to hold on to
    nn = np.arange(4)[:, None]
    crop = (-80, 80, -80, 80, -30.0, None)     # the planted motions reach 20 m: a z bound that keeps every cloud populated
    res = gpu.evaluate_local(q, m, nn, gt, n_k=(128,), ransac_max_it=3000, query_clouds=qc, map_clouds=mc, crop=crop)
    plain = gpu.evaluate_local(q, m, nn, gt, n_k=(128,), ransac_max_it=3000)
    base = {'rre', 'rte', 'repeatability', 'success', 'success_inliers', 'failure_inliers', 'repeatability_refined', 't_ransac',
            't_ransac_sd'}
    new = {'rre_refined', 'rte_refined', 'success_refined', 'success_inliers_refined', 'failure_inliers_refined'}
    assert set(plain[128]) == base and set(res[128]) == base | new
    for k in base - {'t_ransac', 'repeatability_refined'}:
        assert res[128][k] == plain[128][k], k
    # the same numbers by hand: T_refined from the public calls (bitwise reproducible), T_estimated from register_pairs
    ref = gpu.refine_pairs(qc, mc, torch.from_numpy(gt), crop)
    T_ref = _np(ref["T"])
    from tests.test_registration_host import pad_batch, repeatability_f64
    F1, F2, K1, K2, n1, n2 = pad_batch([p[:4] for p in pairs])
    reg = gpu.register_pairs(_cu(F1), _cu(F2), _cu(K1), _cu(K2), n1=_cu(n1), n2=_cu(n2), T_gt=_cu(gt), ransac_max_it=3000,
                             pair_ids=_cu(np.arange(4, dtype=np.int32)))
    T_est, inl = _np(reg["T"]), _np(reg["inliers"])
    mets = [metrics_f64(T_est[i], T_ref[i]) for i in range(4)]
    suc = np.array([x[2] for x in mets], bool)
    r = res[128]
    assert r["success_refined"] == suc.mean()
    assert abs(r["rte_refined"] - np.mean([x[0] for x, s in zip(mets, suc) if s])) < 1e-9
    assert abs(r["rre_refined"] - np.mean([x[1] for x, s in zip(mets, suc) if s])) < 1e-5
    assert r["success_inliers_refined"] == (inl[suc].mean() if suc.any() else 0.0)
    assert r["failure_inliers_refined"] == (inl[~suc].mean() if (~suc).any() else 0.0)
    rep = [repeatability_f64(p[2], p[3], T_ref[i], 0.5) for i, p in enumerate(pairs)]
    assert abs(r["repeatability_refined"] - np.mean(rep)) < 1e-12
    # ICP did its work where it could: the undisturbed pairs end nearer than a centimetre-scale box displacement of T_gt
    st = _np(ref["status"])
    assert (st[[0, 2, 3]] == 0).all() and max(box_displacement(T_ref[i], gt[i]) for i in (0, 2, 3)) < 1.0

"""GPU tests of the training-tuple path (csrc/tuples.hip, egonn_amd/tuples.py).  Oracles: tests/golden/tuples_ref.npz (outputs
of the reference's own find_neighbours_ndx / filter_query_elements / relative_pose / in_sorted_array, written by
tests/golden/make_golden_tuples.py) and the numpy restatements of tests/tuples_data.py, which tests/test_tuples_host.py pins
to that fixture.  Only the fixture and numpy are read here.

Bounds.  Radius join, masks, gather: equality, no excused rows (the fixture script asserts that the fp64 rule reproduces every
reference row).  Relative poses, local-frame set: max |device - reference| <= 4 * d0, d0 = the deviation of the numpy
restatement of the device formula from the reference on the same set, stored in the fixture (1.14e-13 at |t| <= 200 m); the
factor covers the summation order of three-term dot products.  UTM set: the device's largest error against the same formula
in numpy longdouble must not exceed the reference's own (1.17e-9: np.linalg.inv(m2) @ m1 cancels digits there).
End to end: bitwise against `registration.refine_pairs` pair by pair, which DESIGN.md §3.7 guarantees for a pair alone and
inside a batch."""
import numpy as np
import pytest
import torch

from tests import tuples_data as D

pytestmark = pytest.mark.gpu
GUARD = -7


@pytest.fixture(scope="module")
def fx():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    g.build()
    return D.load_fixture()


def _host(nb):
    return nb["offsets"].cpu().numpy(), nb["indices"].cpu().numpy(), nb["counts"].cpu().numpy()


def _assert_rows(nb, off, idx, tag):
    o, i, c = _host(nb)
    assert o.dtype == np.int64 and i.dtype == np.int32 and c.dtype == np.int32, tag
    assert np.array_equal(c, np.diff(off)), (tag, "counts")
    assert np.array_equal(o, off), (tag, "offsets")
    for r, (got, want) in enumerate(zip(D.rows_of(o, i), D.rows_of(off, idx))):
        assert np.array_equal(got, want), (tag, "row", r)
    assert int(nb["status"]) == 0, tag


# ----------------------------------------------------------------------------- radius join
@pytest.mark.parametrize("rows", D.TRAJECTORY_ROWS)
def test_radius_join_equals_the_reference_on_trajectories(fx, rows):
    """1, 63, 65, 257 and 1150 rows: below / above a wave of 64 and a tile of 256, several workgroups; all three radii in ONE
    count sweep; every row equal to the reference's sorted query_radius row"""
    from egonn_amd import radius_neighbors
    xy = fx[f"traj{rows}_xy"]
    out = radius_neighbors(xy, None, list(D.TRAJECTORY_RADII))
    assert len(out) == 3 and all(o["indices"].is_cuda and o["offsets"].is_cuda for o in out)
    for o, r in zip(out, D.TRAJECTORY_RADII):
        _assert_rows(o, *D.fixture_rows(fx, f"traj{rows}_r{int(r)}"), (rows, r))


def test_radius_join_boundary_self_and_foreign_reference(fx):
    from egonn_amd import radius_neighbors, count_within
    # 1136 pairs exactly at distance 5 on the lattice: <= keeps them all, as the reference does
    _assert_rows(radius_neighbors(fx["lattice_xy"], None, D.LATTICE_RADIUS), *D.fixture_rows(fx, "lattice_r5"), "lattice")
    # 40 scans at one position: exclude_self drops j == i only, 39 remain per row
    st = fx["stationary_xy"]
    both = radius_neighbors(st, None, [D.STATIONARY_RADIUS, D.STATIONARY_RADIUS], exclude_self=[True, False])
    _assert_rows(both[0], *D.fixture_rows(fx, "stationary_r1_noself"), "stationary, no self")
    _assert_rows(both[1], *D.fixture_rows(fx, "stationary_r1"), "stationary")
    assert (both[0]["counts"] == 39).all() and (both[1]["counts"] == 40).all()
    # radius 0: identical positions are neighbours (0 <= 0), distinct ones are not
    zero = radius_neighbors(st, None, 0.0, exclude_self=True)
    assert (zero["counts"] == 39).all()
    tr = fx["traj65_xy"]
    _assert_rows(radius_neighbors(tr, None, 0.0), np.arange(66, dtype=np.int64), np.arange(65, dtype=np.int32), "radius 0")
    # a query set against a different reference set (300 x 500, the float32-rounded map of filter_query_elements)
    map32 = fx["filter_map_xy"].astype(np.float32).astype(np.float64)
    q = fx["filter_query_xy"]
    _assert_rows(radius_neighbors(q, map32, D.FILTER_RADIUS), *D.fixture_rows(fx, "filter"), "foreign reference")
    cnt = count_within(q, map32, D.FILTER_RADIUS)
    assert cnt.is_cuda and cnt.dtype == torch.int32 and np.array_equal(cnt.cpu().numpy(), np.diff(fx["filter_off"]))


def test_radius_join_nan_and_empty_reference(fx):
    from egonn_amd import radius_neighbors, count_within
    xy = fx["traj257_xy"].copy()
    xy[5, 0] = np.nan
    xy[200, 1] = np.nan
    for r in (2.0, 50.0):
        off, idx = D.radius_rows(xy, xy, r)
        nb = radius_neighbors(xy, None, r)
        _assert_rows(nb, off, idx, ("nan", r))
        got = nb["indices"].cpu().numpy()
        assert off[6] == off[5] and off[201] == off[200] and 5 not in got and 200 not in got
    empty = radius_neighbors(xy, np.zeros((0, 2)), 3.0)
    assert empty["indices"].numel() == 0 and not empty["offsets"].any() and empty["offsets"].shape == (258,)
    assert not count_within(xy, np.zeros((0, 2)), 3.0).any()
    none = radius_neighbors(np.zeros((0, 2)), xy, 3.0)
    assert none["offsets"].tolist() == [0] and none["indices"].numel() == 0


def test_radius_fill_capacity_and_reproducibility(fx):
    """a capacity one short: the status bit is set, nothing is written at or past the capacity (a guard region behind it stays
    as it was), what fits is right; offsets that are not the scan of the counts are reported; two runs give the same bits"""
    from egonn_amd import _lib, radius_neighbors
    from egonn_amd.tuples import STATUS_BAD_OFFSETS, STATUS_CAPACITY
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    xy = torch.from_numpy(fx["traj1150_xy"]).to(dev)
    a, b = radius_neighbors(xy, None, 10.0), radius_neighbors(xy, None, 10.0)
    assert torch.equal(a["indices"], b["indices"]) and torch.equal(a["offsets"], b["offsets"])
    total = a["indices"].numel()
    n = xy.shape[0]

    def fill(offsets, capacity):
        buf = torch.full((total + 64,), GUARD, dtype=torch.int32, device=dev)
        status = torch.full((), 99, dtype=torch.int32, device=dev)
        _lib.call(dev, lib.egonn_radius_fill, xy.data_ptr(), n, xy.data_ptr(), n, 10.0, 0, offsets.data_ptr(), buf.data_ptr(), capacity,
                  status.data_ptr())
        return buf, int(status)
    buf, st = fill(a["offsets"], total)
    assert st == 0 and torch.equal(buf[:total], a["indices"]) and (buf[total:] == GUARD).all()
    buf, st = fill(a["offsets"], total - 1)
    assert st & STATUS_CAPACITY
    assert torch.equal(buf[: total - 1], a["indices"][: total - 1]) and (buf[total - 1:] == GUARD).all()
    short = a["offsets"].clone()
    short[n // 2:] -= 1                                   # row n/2 - 1 loses a slot: its last hit must not spill into the next row
    buf, st = fill(short, total)
    assert st & STATUS_BAD_OFFSETS and (buf[total - 1:] == GUARD).all()
    lo = int(a["offsets"][n // 2])
    assert torch.equal(buf[: lo - 1], a["indices"][: lo - 1]) and torch.equal(buf[lo - 1: total - 1], a["indices"][lo:])


# ----------------------------------------------------------------------------- pair masks
@pytest.fixture(scope="module")
def mask_index(fx):
    from egonn_amd.tuples import TrainingTuple, TupleIndex
    pos, non = D.rows_of(fx["mask_pos_off"], fx["mask_pos_idx"]), D.rows_of(fx["mask_non_off"], fx["mask_non_idx"])
    return TupleIndex({i: TrainingTuple(i, i, "", pos[i], non[i], np.eye(4)) for i in range(80)})


@pytest.mark.parametrize("B", D.MASK_BATCHES)
def test_pair_masks_equal_the_reference(fx, mask_index, B):
    pm, nm = mask_index.masks(fx[f"mask{B}_labels"])
    assert pm.is_cuda and nm.is_cuda and pm.dtype == torch.bool and nm.dtype == torch.bool and pm.shape == nm.shape == (B, B)
    assert np.array_equal(pm.cpu().numpy(), fx[f"mask{B}_pos"]) and np.array_equal(nm.cpu().numpy(), fx[f"mask{B}_neg"])


def test_pair_masks_label_out_of_range(fx, mask_index):
    from egonn_amd.tuples import STATUS_BAD_INDEX
    labels = np.array([3, 80, -1, 4, 79], dtype=np.int32)
    pm, nm, status = mask_index.masks_u8(labels)
    want_p, want_n = D.pair_masks(labels, fx["mask_pos_off"], fx["mask_pos_idx"], fx["mask_non_off"], fx["mask_non_idx"])
    assert int(status) == STATUS_BAD_INDEX
    assert np.array_equal(pm.cpu().numpy().astype(bool), want_p) and np.array_equal(nm.cpu().numpy().astype(bool), want_n)
    assert not pm[1].any() and not pm[:, 2].any() and not nm[1].any() and not nm[:, 2].any() and bool(pm[0, 3])
    assert int(mask_index.masks_u8(labels[[0, 3, 4]])[2]) == 0, "the status word is cleared by every call"


def test_pair_masks_replay_in_a_graph(fx, mask_index):
    """one memset and one launch on one stream (no parallel branches): captured, then replayed on changed labels"""
    first, second = fx["mask33_labels"], np.ascontiguousarray(fx["mask33_labels"][::-1])
    tables = [fx[k] for k in ("mask_pos_off", "mask_pos_idx", "mask_non_off", "mask_non_idx")]
    labels = torch.from_numpy(first).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = mask_index.masks_u8(labels)                 # warm-up on the side stream; its tensors become the graph's outputs
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mask_index.masks_u8(labels, out=out)
    for lab in (first, second):
        labels.copy_(torch.from_numpy(lab))
        out[0].fill_(9), out[1].fill_(9)
        graph.replay()
        torch.cuda.synchronize()
        want_p, want_n = D.pair_masks(lab, *tables)
        assert np.array_equal(out[0].cpu().numpy(), want_p.astype(np.uint8)) and np.array_equal(out[1].cpu().numpy(), want_n.astype(np.uint8))
        assert int(out[2]) == 0
    assert not np.array_equal(fx["mask33_pos"], fx["mask33_pos"][::-1, ::-1]), "the replay saw different labels"


# ----------------------------------------------------------------------------- relative poses
def test_relative_poses_local_frame_within_four_d0(fx):
    from egonn_amd import relative_poses
    poses, ia, ib = fx["poses_local"], fx["poses_local_ia"], fx["poses_local_ib"]
    neg, st = relative_poses(poses, ia, ib, True, return_status=True)
    plain = relative_poses(poses, ia, ib, negate_translation=False)
    assert neg.is_cuda and neg.dtype == torch.float64 and neg.shape == (200, 4, 4) and not st.any()
    neg, plain = neg.cpu().numpy(), plain.cpu().numpy()
    for got, key in ((neg, "neg"), (plain, "plain")):
        err, d0 = np.abs(got - fx[f"poses_local_ref_{key}"]).max(), float(fx[f"poses_local_d0_{key}"])
        print(f"relative poses, local set, {key}: device vs reference {err:.3e}, d0 {d0:.3e}")
        assert err <= 4 * d0
    assert np.array_equal(neg[:, :3, :3], plain[:, :3, :3]) and np.array_equal(neg[:, :3, 3], -plain[:, :3, 3])
    assert np.array_equal(neg[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (200, 1)))
    again = relative_poses(poses, ia, ib, True).cpu().numpy()
    assert np.array_equal(neg, again)


def test_relative_poses_utm_no_worse_than_the_reference(fx):
    from egonn_amd import relative_poses
    poses, ia, ib = fx["poses_utm"], fx["poses_utm_ia"], fx["poses_utm_ib"]
    truth_neg, _ = D.relative_poses(poses, ia, ib, True, dtype=np.longdouble)
    truth_plain, _ = D.relative_poses(poses, ia, ib, False, dtype=np.longdouble)
    for flag, truth, key in ((True, truth_neg, "neg"), (False, truth_plain, "plain")):
        got = relative_poses(poses, ia, ib, flag).cpu().numpy()
        dev_err = float(np.abs(got - truth).max())
        ref_err = float(np.abs(fx[f"poses_utm_ref_{key}"] - truth).max())
        print(f"relative poses, UTM set, {key}: device vs longdouble {dev_err:.3e}, reference vs longdouble {ref_err:.3e}")
        assert dev_err <= ref_err


def test_relative_poses_status_bits():
    from egonn_amd import relative_poses
    from egonn_amd.tuples import POSE_BAD_INDEX, POSE_BAD_ROW, POSE_SINGULAR
    poses = np.tile(np.eye(4), (5, 1, 1))
    poses[:, :3, 3] = np.arange(15).reshape(5, 3)
    poses[1, 3, 3] = 1.0 + 1e-12                          # last row not exactly 0 0 0 1
    poses[2, :3, :3] = [[1, 2, 3], [2, 4, 6], [0, 0, 1]]  # rank 2
    poses[3, 3, 0] = 1e-300
    poses[4, :3, :3] = np.nan
    ia, ib = [0, 0, 2, 0, 5, 0, 3, 0, -1], [1, 2, 0, 0, 0, 7, 0, 4, 0]
    out, st = relative_poses(poses, ia, ib, True, return_status=True)
    want, want_st = D.relative_poses(poses, ia, ib, True)
    assert st.tolist() == want_st.tolist() == [POSE_BAD_ROW, POSE_SINGULAR, 0, 0, POSE_BAD_INDEX, POSE_BAD_INDEX, POSE_BAD_ROW,
                                               POSE_SINGULAR, POSE_BAD_INDEX]
    out = out.cpu().numpy()
    for p, s in enumerate(want_st):
        assert np.array_equal(out[p], np.eye(4)) == (s != 0 or p == 3), p
    assert np.array_equal(out[2], want[2])                # a singular R_a is no obstacle: only R_b is inverted
    empty = relative_poses(poses, [], [], True)
    assert empty.shape == (0, 4, 4)


# ----------------------------------------------------------------------------- cloud gather
def _toy_bank():
    from egonn_amd import CloudBank
    sizes = [5, 0, 300, 1, 64, 1000, 17]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pts = np.random.default_rng(8).normal(size=(int(off[-1]), 3))
    bank = CloudBank()
    bank.points = torch.from_numpy(pts).cuda()
    bank.host_offsets = off.tolist()
    return bank, pts, off


def test_gather_equals_numpy():
    bank, pts, off = _toy_bank()
    rng = np.random.default_rng(9)
    for pick in ([5], [1], [2, 2, 1, 6, 0, 2], rng.integers(0, 7, size=130).tolist()):
        g = bank.gather(pick)
        want_pts, want_off = D.gather(pts, off, pick)
        assert int(g["status"]) == 0 and g["offsets"].dtype == torch.int64 and g["points"].dtype == torch.float64
        assert np.array_equal(g["offsets"].cpu().numpy(), want_off), pick
        assert np.array_equal(g["points"].cpu().numpy(), want_pts.reshape(-1, 3)), pick
    # a larger capacity than needed: the tail is not touched
    g = bank.gather([4, 0], capacity=100)
    assert g["offsets"].tolist() == [0, 64, 69] and np.array_equal(g["points"][:69].cpu().numpy(), np.concatenate([pts[306:370], pts[:5]]))


def test_gather_overflow_and_bad_pick_leave_empty_offsets():
    from egonn_amd.tuples import STATUS_BAD_INDEX, STATUS_CAPACITY
    bank, pts, off = _toy_bank()
    g = bank.gather([2, 5, 0], capacity=1304)             # 300 + 1000 + 5 = 1305: one short
    assert int(g["status"]) == STATUS_CAPACITY and g["offsets"].tolist() == [0, 0, 0, 0]
    pick = torch.tensor([0, 7, 3], dtype=torch.int32).cuda()
    g = bank.gather(pick, capacity=64)
    assert int(g["status"]) == STATUS_BAD_INDEX and g["offsets"].tolist() == [0, 0, 0, 0]
    g = bank.gather(torch.tensor([0, -1], dtype=torch.int32).cuda(), capacity=64)
    assert int(g["status"]) == STATUS_BAD_INDEX and g["offsets"].tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        bank.gather([0, 7])                               # host picks are checked before the launch
    # the ICP sees empty clouds
    from egonn_amd import icp_pairs
    from egonn_amd.registration import ICP_EMPTY
    ok = bank.gather([2, 5])
    bad = bank.gather([2, 5], capacity=10)
    r = icp_pairs(bad["points"], bad["offsets"], ok["points"], ok["offsets"], max_iteration=2)
    assert r["status"].tolist() == [ICP_EMPTY, ICP_EMPTY]


# ----------------------------------------------------------------------------- evaluation set
def test_filter_query_elements_keeps_the_references_queries(fx):
    from egonn_amd import EvaluationTuple, filter_query_elements, generate_evaluation_set
    map_set = [EvaluationTuple(i, f"m{i}", p) for i, p in enumerate(fx["filter_map_xy"])]
    query_set = [EvaluationTuple(i, f"q{i}", p) for i, p in enumerate(fx["filter_query_xy"])]
    kept = filter_query_elements(query_set, map_set, D.FILTER_RADIUS)
    assert [e.timestamp for e in kept] == np.flatnonzero(fx["filter_kept"]).tolist()
    assert all(e is query_set[e.timestamp] for e in kept)
    es = generate_evaluation_set(map_set, query_set, D.FILTER_RADIUS)
    assert es.map_set is map_set and [e.timestamp for e in es.query_set] == [e.timestamp for e in kept]
    assert filter_query_elements([], map_set, 1.0) == [] and filter_query_elements(query_set, [], 1.0) == []


# ----------------------------------------------------------------------------- end to end
POS_TH, NEG_TH = 2.0, 2.6          # 6 scans over 5 m: a non-negative radius of 10 m would leave no negatives in a batch


@pytest.fixture(scope="module")
def e2e(fx):
    """the synthetic sequence, its bank, the generator at 16 pairs per call, and the pair-by-pair reference, computed once.
    The planted poses are proper scan -> world poses, so the relative pose is taken without MulRan's sign fix."""
    from egonn_amd import CloudBank, generate_training_tuples, refine_pairs, relative_poses
    from egonn_amd.tuples import MULRAN_CROP
    raws, planted, gps = D.planted_sequence()
    bank = CloudBank().add(raws)
    tuples, stats = generate_training_tuples(gps, bank, POS_TH, NEG_TH, negate_translation=False)
    clouds = [D.zero_filtered(r) for r in raws]
    po, pi = D.radius_rows(gps[:, :2, 3], gps[:, :2, 3], POS_TH, exclude_self=True)
    ia = np.repeat(np.arange(6), np.diff(po)).astype(np.int32)
    T_init = relative_poses(gps, ia, pi, negate_translation=False)
    ref = []
    for p, (a, b) in enumerate(zip(ia, pi)):
        r = refine_pairs([clouds[a]], [clouds[b]], T_init[p: p + 1], MULRAN_CROP)
        ref.append((r["T"][0].cpu().numpy(), float(r["fitness"][0]), float(r["inlier_rmse"][0]), int(r["status"][0])))
    return dict(raws=raws, planted=planted, gps=gps, bank=bank, tuples=tuples, stats=stats, clouds=clouds, ia=ia, ib=pi, po=po,
                T_init=T_init.cpu().numpy(), ref=ref)


def _pose_of(tuples, a, b):
    return tuples[int(a)].positives_poses[int(b)]


def test_end_to_end_neighbours_and_bank(e2e):
    from egonn_amd import CloudBank
    gps, tuples, bank = e2e["gps"], e2e["tuples"], e2e["bank"]
    xy = gps[:, :2, 3]
    po, pi = D.radius_rows(xy, xy, POS_TH, exclude_self=True)
    no, ni = D.radius_rows(xy, xy, NEG_TH)
    assert sorted(tuples) == list(range(6))
    for i in range(6):
        t = tuples[i]
        assert t.positives.dtype == np.int32 and t.non_negatives.dtype == np.int32 and t.id == i
        assert np.array_equal(t.positives, pi[po[i]: po[i + 1]]) and np.array_equal(t.non_negatives, ni[no[i]: no[i + 1]])
        assert i not in t.positives and i in t.non_negatives and np.array_equal(t.pose, gps[i])
        assert sorted(t.positives_poses) == t.positives.tolist()
    assert len(bank) == 6 and not any(bank.status) and all(0 < s < 6000 for s in bank.sizes())
    # chunking does not change the bank: one scan per chunk gives the same resident clouds
    one = CloudBank(chunk_points=7000).add(e2e["raws"])
    assert one.host_offsets == bank.host_offsets and torch.equal(one.points[: one.n_points], bank.points[: bank.n_points])


def test_end_to_end_refinement_is_bitwise_the_pairwise_icp(e2e):
    stats, tuples = e2e["stats"], e2e["tuples"]
    assert stats["pairs"] == len(e2e["ref"]) == int(e2e["po"][-1]) >= 10
    for p, (a, b) in enumerate(zip(e2e["ia"], e2e["ib"])):
        T, fit, rmse, st = e2e["ref"][p]
        assert np.array_equal(_pose_of(tuples, a, b), T), (a, b)
        assert stats["fitness_per_pair"][p] == fit and stats["inlier_rmse_per_pair"][p] == rmse and stats["status_per_pair"][p] == st
    fits = np.array([r[1] for r in e2e["ref"]])
    assert stats["fitness"] == {"min": fits.min(), "mean": fits.mean(), "max": fits.max()}
    assert sum(stats["status_counts"].values()) == stats["pairs"] and stats["pose_status_counts"] == {0: stats["pairs"]}
    assert 0.0 < stats["fitness"]["min"] <= 1.0 and 0.0 < stats["inlier_rmse"]["max"] < 1.2


@pytest.mark.parametrize("pairs_per_call", [1, 5])
def test_end_to_end_chunk_size_does_not_change_a_bit(e2e, pairs_per_call):
    from egonn_amd import generate_training_tuples
    tuples, stats = generate_training_tuples(e2e["gps"], e2e["bank"], POS_TH, NEG_TH, pairs_per_call=pairs_per_call,
                                             negate_translation=False)
    for a, b in zip(e2e["ia"], e2e["ib"]):
        assert np.array_equal(_pose_of(tuples, a, b), _pose_of(e2e["tuples"], a, b)), (a, b)
    for k in ("fitness_per_pair", "inlier_rmse_per_pair", "status_per_pair"):
        assert np.array_equal(stats[k], e2e["stats"][k]), k


def test_end_to_end_refinement_moves_towards_the_planted_pose(e2e):
    planted = e2e["planted"]
    for p, (a, b) in enumerate(zip(e2e["ia"], e2e["ib"])):
        truth = np.linalg.inv(planted[b]) @ planted[a]
        d_init = np.linalg.norm(e2e["T_init"][p] - truth)
        d_ref = np.linalg.norm(_pose_of(e2e["tuples"], a, b) - truth)
        print(f"pair ({a},{b}): |T_init - planted| {d_init:.4f}, |T_refined - planted| {d_ref:.4f}")
        assert d_ref < d_init, (a, b)


def test_end_to_end_without_refinement_returns_the_initial_pose(e2e):
    from egonn_amd import generate_training_tuples
    tuples, stats = generate_training_tuples(e2e["gps"], None, POS_TH, NEG_TH, refine=False, negate_translation=False)
    for p, (a, b) in enumerate(zip(e2e["ia"], e2e["ib"])):
        assert np.array_equal(_pose_of(tuples, a, b), e2e["T_init"][p])
    assert stats["fitness"] == {"min": 1.0, "mean": 1.0, "max": 1.0} and stats["pairs"] == len(e2e["ia"])
    loaded, _ = generate_training_tuples(e2e["gps"], lambda i: e2e["raws"][i], POS_TH, NEG_TH, negate_translation=False)
    for a, b in zip(e2e["ia"], e2e["ib"]):                # a callable instead of a bank: the bank is filled from it
        assert np.array_equal(_pose_of(loaded, a, b), _pose_of(e2e["tuples"], a, b))


def test_end_to_end_training_step_from_the_tuples(e2e):
    """tuples -> BatchSampler -> TrainingSet -> one EgoNNTrainStep at batch 4; the same step fed hand-built masks (the numpy
    rule) and T_gt (the pairwise ICP results) gives the same bits"""
    from egonn_amd import BatchSampler, CartesianQuantizer, EgoNNTrainStep, TrainBatcher, TrainingSet
    from egonn_amd import local_loss as L
    from tests.test_gpu_local_loss_batch import LOCAL, _model
    tuples, clouds, gps = e2e["tuples"], e2e["clouds"], e2e["gps"]
    sampler = BatchSampler(tuples, batch_size=4, seed=2)
    make_batcher = lambda: TrainBatcher(CartesianQuantizer(0.4), aug_mode=1, seed=5, rot_max=0.1, trans_max=0.2)   # noqa: E731
    ts = TrainingSet(tuples, lambda i: clouds[i], make_batcher(), sampler)
    batches = list(sampler)
    sampler.epoch = 0                                     # the set below draws the same epoch again
    got = list(ts)
    assert len(got) == len(batches) >= 1
    labels = batches[0]
    batch, pm, nm, local = got[0]
    assert len(labels) == 4 and batch["batch_size"] == 4 and batch["coords"].is_cuda
    assert pm.dtype == torch.bool and nm.dtype == torch.bool and pm.shape == nm.shape == (4, 4) and pm.is_cuda
    xy = gps[:, :2, 3]
    po, pi = D.radius_rows(xy, xy, POS_TH, exclude_self=True)
    no, ni = D.radius_rows(xy, xy, NEG_TH)
    want_p, want_n = D.pair_masks(labels, po, pi, no, ni)
    assert want_n.any(axis=1).all() and want_p.any(axis=1).all(), "every row of the sampled batch has a positive and a negative"
    assert np.array_equal(pm.cpu().numpy(), want_p) and np.array_equal(nm.cpu().numpy(), want_n)
    assert local["T_gt"].shape == (2, 4, 4) and len(local["len_batch"]) == 2

    # the same inputs by hand
    hb = make_batcher()
    dev = torch.device("cuda", torch.cuda.current_device())

    def cat(ids):
        off = np.concatenate([[0], np.cumsum([len(clouds[i]) for i in ids])]).astype(np.int64)
        return torch.from_numpy(np.concatenate([clouds[i] for i in ids])).to(dev), off
    pts, off = cat(labels)
    hand_batch = hb(pts, off, labels, draw=0, set_id=0)
    anchors, positives = labels[0::2], labels[1::2]
    pair_of = {(int(a), int(b)): p for p, (a, b) in enumerate(zip(e2e["ia"], e2e["ib"]))}
    T_hand = torch.from_numpy(np.stack([e2e["ref"][pair_of[(a, b)]][0] for a, b in zip(anchors, positives)])).float()
    hand_local = hb.local(*cat(anchors), *cat(positives), positives, T_hand, draw=0)
    assert torch.equal(hand_batch["coords"], batch["coords"]) and torch.equal(hand_local["T_gt"], local["T_gt"])

    def step(b, p, n, loc):
        model = _model()
        gl, ll, stats = EgoNNTrainStep(model, torch.optim.SGD(model.parameters(), lr=0.0),
                                       local_loss_fn=L.BatchedKeypointCorrLoss(**LOCAL))(b, p, n, loc)
        grads = {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}
        return gl, ll, stats, grads
    gl, ll, stats, grads = step(batch, pm, nm, local)
    assert np.isfinite(float(gl)) and np.isfinite(float(ll))
    gl_h, ll_h, stats_h, grads_h = step(hand_batch, torch.from_numpy(want_p), torch.from_numpy(want_n), hand_local)
    assert torch.equal(gl, gl_h) and torch.equal(ll, ll_h) and set(stats) == set(stats_h) and set(grads) == set(grads_h)
    for k in stats:
        a, b = torch.as_tensor(stats[k]), torch.as_tensor(stats_h[k])
        assert torch.equal(a, b) or (bool(torch.isnan(a).all()) and bool(torch.isnan(b).all())), k
    for k in grads:
        assert torch.equal(grads[k], grads_h[k]), k

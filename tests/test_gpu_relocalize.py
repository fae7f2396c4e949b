"""GPU tests of the relocalisation layer (run with -m gpu on an MI355X): both addressings of the matching operator
(egonn_match_candidates by index, egonn_match_mutual on host-gathered operands) against each other bit for bit, against the
results recorded from the parent commit's one-workgroup-per-pair kernel (tests/golden/match_parent.npz) and against the float64
restatement; invalid candidates, the whole of verify_candidates against register_pairs on host-gathered
operands and against the float64 restatement of the pick rule (tests/test_relocalize_host.py), the planted relocalisation,
the batch / order / chunk / graph invariances, the descriptor path end to end, the ICP refinement and the metrics."""
import ctypes

import numpy as np
import pytest
import torch

from tests.match_data import EXCUSED_ROW_CAP, check_matching, dense_of, gather_host as _gather_host, index_sets, recorded, rows_of
from tests.test_registration_host import metrics_f64, planted_pair
from tests.test_relocalize_host import (BAD_INDEX, NO_CANDIDATE, PLANTED_H, PLANTED_K, PLANTED_M, UNVERIFIED, WEAK_OF, match_status,
                                        pair_id, pick_f64, planted_case, planted_map_poses, planted_solved, pose_product_f64)

pytestmark = pytest.mark.gpu

PAIR_KEYS = ("T", "inliers", "fitness", "inlier_rmse", "best_t", "pair_status", "match_status", "corr", "n_corr", "pair_ids", "rte",
             "rre", "success")
QUERY_KEYS = ("best_rank", "best_index", "reranked", "T_rel", "pose", "safe_pick", "best_inliers", "status", "best_rte", "best_rre",
              "best_success")


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


def _match(qf, qn, bank, bn, nn, M):
    """egonn_match_candidates itself: `bank` may be longer than M rows (a guard region behind the map)"""
    from egonn_amd import _lib
    lib = _lib.load()
    Q, n_max, D = qf.shape
    k = nn.shape[1]
    corr = torch.full((Q * k, n_max, 2), -7, dtype=torch.int32, device="cuda")
    n_corr = torch.full((Q * k,), -7, dtype=torch.int32, device="cuda")
    status = torch.full((Q * k,), -7, dtype=torch.int32, device="cuda")
    nb = lib.egonn_match_candidates_scratch_bytes(Q, k, n_max)
    assert nb > 0
    scratch = torch.empty(nb // 8 + 1, dtype=torch.int64, device="cuda")
    _lib.call(qf.device, lib.egonn_match_candidates, qf.data_ptr(), qn.data_ptr(), bank.data_ptr(), bn.data_ptr(), nn.data_ptr(), Q, k,
              M, n_max, D, corr.data_ptr(), n_corr.data_ptr(), status.data_ptr(), scratch.data_ptr(), nb)
    torch.cuda.synchronize()
    return _np(corr), _np(n_corr), _np(status)


def _check_match(gpu, name):
    """set `name` of tests/match_data.py: egonn_match_candidates == gpu.match_mutual on host-gathered operands == the parent
    commit's recorded result, bit for bit, and the float64 restatement inside its caps; -> (corr, n_corr)"""
    qf, qn, bf, bn, nn = index_sets()[name]
    M = len(bf)
    corr, n_corr, status = _match(_cu(qf), _cu(qn), _cu(bf), _cu(bn), _cu(nn), M)
    F1, F2, n1, n2 = dense_of(qf, qn, bf, bn, nn)
    want, want_n = gpu.match_mutual(_cu(F1), _cu(F2), _cu(n1), _cu(n2))
    assert np.array_equal(n_corr, _np(want_n)), (n_corr, _np(want_n))
    assert np.array_equal(corr, _np(want))
    assert status.tolist() == [match_status(int(i), M) for i in nn.reshape(-1)]
    gold, gold_n = recorded(name, (qf, qn, bf, bn, nn))
    assert np.array_equal(n_corr, gold_n), (name, n_corr, gold_n)
    assert np.array_equal(corr, gold), name
    excused, total, unchecked = check_matching(rows_of(F1, F2, n1, n2), corr, n_corr)
    print(f"[relocalize] {name}: excused matching rows {excused} of {total}, unchecked pairs {unchecked}")
    assert excused <= EXCUSED_ROW_CAP * total and unchecked == 0
    return corr, n_corr


# ------------------------------------------------------------------ 1. matching: both addressings, the recorded parent, float64
def test_matching_planted_case_and_shapes(gpu):
    corr, n_corr = _check_match(gpu, "planted")
    assert (n_corr >= 3).all() and n_corr.shape == (PLANTED_M * PLANTED_K,)
    _check_match(gpu, "planted_shared_entries")          # one map entry used by several queries and twice in one row
    _check_match(gpu, "planted_q1_k1")
    _check_match(gpu, "planted_q5_k3")


def test_matching_largest_tile(gpu):
    """n_max = 256, D = 256 (the largest LDS tile), counts 256 / 200 (no multiple of the 64-row or the 32-column tile), both ways"""
    corr, n_corr = _check_match(gpu, "largest_tile")
    assert (n_corr >= 3).all() and corr[0, : n_corr[0], 0].max() > 192 and corr[0, : n_corr[0], 1].max() > 192


def test_matching_small_and_short_sets(gpu):
    _check_match(gpu, "n_max_8_dim_4")
    # counts 0, 1, 2, 3 on either side against everything: the "fewer than 3 mutual" branch and the empty pair
    corr, n_corr = _check_match(gpu, "counts_0_to_3")
    n_corr = n_corr.reshape(5, 5)
    assert (n_corr[3] == 0).all() and (n_corr[:, 4] == 0).all()
    assert n_corr[0, 0] == 1 and n_corr[1, 0] == 2 and n_corr[2, 0] == 3 and n_corr[4, 1] == 64 and n_corr[4, 2] == 64
    _check_match(gpu, "clipped_counts")                  # counts outside [0, n_max] are clipped


def test_matching_lowest_index_merge(gpu):
    """edge_pairs()['duplicate_descriptors'] moved so that its ties span the tiles of the kernel (tests/match_data.py): the merge
    must keep the lower tile's index on the tie, as a single ascending scan does."""
    corr, n_corr = _check_match(gpu, "ties_across_row_tiles")
    got = corr[0, : n_corr[0]]
    assert not set(range(64, 70)) & set(got[:, 0].tolist()) and 40 not in got[:, 1]       # a duplicate in a later tile never wins
    # the mirrored arrangement: the candidate's copies of one row sit in column tiles 0 and 2
    _check_match(gpu, "ties_across_column_tiles")


# ------------------------------------------------------------------ 2. invalid indices
def test_invalid_indices_read_nothing(gpu):
    c = planted_case()
    M = 5
    bank = c["map_feat"][:M]
    nn = np.array([[2, -1, M, -7]], np.int32)
    qf, qn, bn = _cu(c["q_feat"][2:3]), _cu(np.full(1, 64, np.int32)), _cu(np.full(M, 64, np.int32))
    corr, n_corr, status = _match(qf, qn, _cu(bank), bn, _cu(nn), M)
    assert status.tolist() == [0, NO_CANDIDATE, NO_CANDIDATE | BAD_INDEX, NO_CANDIDATE | BAD_INDEX]
    assert n_corr[1:].tolist() == [0, 0, 0] and (corr[1:] == -1).all()
    want, want_n = gpu.match_mutual(qf, _cu(bank[2:3]))
    assert n_corr[0] == int(want_n[0]) > 3 and np.array_equal(corr[0], _np(want[0]))
    # a guard region of NaNs behind the map: index M would land in it, index -7 in front of the map
    guard = torch.full((M + 8, 64, 128), float("nan"), device="cuda")
    guard[:M] = _cu(bank)
    corr_g, n_corr_g, status_g = _match(qf, qn, guard, bn, _cu(nn), M)
    assert np.array_equal(corr_g, corr) and np.array_equal(n_corr_g, n_corr) and np.array_equal(status_g, status)


# ------------------------------------------------------------------ the planted case on the device
def _planted_inputs(utm):
    c = planted_case()
    poses = planted_map_poses(PLANTED_M + 1, utm=utm)
    poses[PLANTED_M] = poses[WEAK_OF]                       # the weak twin was taken at the same place
    T_gt = c["T_planted"][c["nn"]]                          # (6, 4, 4, 4): the planted pose of the candidate
    return c, poses, T_gt


def _kmap(gpu, c, poses, M=None):
    M = M or len(poses)
    km = gpu.KeypointMap(n_k=64, dim=128, global_dim=8)
    km.add({"global": torch.eye(8)[:M], "keypoints": torch.from_numpy(c["map_kp"][:M]),
            "descriptors": torch.from_numpy(c["map_feat"][:M])}, poses[:M])
    return km


def _verify(gpu, c, km, nn, T_gt, rows=slice(None), **kw):
    kw.setdefault("ransac_max_it", PLANTED_H)
    q = np.arange(PLANTED_M, dtype=np.int32)[rows]
    r = gpu.verify_candidates(_cu(c["q_feat"][rows]), _cu(c["q_kp"][rows]), None, km, _cu(np.asarray(nn, np.int32)),
                              query_ids=_cu(q), T_gt=None if T_gt is None else _cu(T_gt), **kw)
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in r.items() if not k.startswith("_")}


_RUNS = {}


def _planted_run(gpu, utm=False):
    if utm not in _RUNS:
        c, poses, T_gt = _planted_inputs(utm)
        _RUNS[utm] = (c, poses, T_gt, _verify(gpu, c, _kmap(gpu, c, poses), c["nn"], T_gt))
    return _RUNS[utm]


def _check_pick(r, nn, M, poses, min_inliers=0):
    """the per-query outputs == the restated pick rule and pose product on the device's per-pair tables, bitwise"""
    for q in range(len(nn)):
        p = pick_f64(nn[q], M, r["T"][q], r["inliers"][q], r["inlier_rmse"][q], r["pair_status"][q], poses, min_inliers,
                     r.get("rte", [None] * len(nn))[q], r.get("rre", [None] * len(nn))[q], r.get("success", [None] * len(nn))[q])
        for key, want in p.items():
            assert np.array_equal(r[key][q], want), (q, key, r[key][q], want)


# ------------------------------------------------------------------ 3. the whole of verify_candidates
@pytest.mark.parametrize("utm", [False, True])
def test_verify_candidates_equals_register_pairs_and_restated_pick(gpu, utm):
    c, poses, T_gt = _planted_inputs(utm)
    nn = c["nn"].copy()
    nn[5, 3], nn[4, 1], nn[1] = -1, 99, [-1, -5, 7, -1]      # a missing, a bad and an all-invalid row (M = 7)
    M, seed, H = PLANTED_M + 1, 3, 777
    T_gt = T_gt.copy()
    T_gt[(nn < 0) | (nn >= M)] = np.eye(4)
    qid = np.arange(10, 10 + PLANTED_M, dtype=np.int32)
    km = _kmap(gpu, c, poses)
    r = gpu.verify_candidates(_cu(c["q_feat"]), _cu(c["q_kp"]), None, km, _cu(nn), query_ids=_cu(qid), T_gt=_cu(T_gt), seed=seed,
                              ransac_max_it=H, min_inliers=5)
    torch.cuda.synchronize()
    r = {k: _np(v) for k, v in r.items() if not k.startswith("_")}
    assert set(PAIR_KEYS + QUERY_KEYS) <= set(r) and r["T"].shape == (6, 4, 4, 4) and r["corr"].shape == (6, 4, 64, 2)
    pids = np.array([[pair_id(qid[q], nn[q, c4]) for c4 in range(PLANTED_K)] for q in range(PLANTED_M)], np.int32)
    assert np.array_equal(r["pair_ids"], pids)
    assert np.array_equal(r["match_status"], np.vectorize(lambda i: match_status(int(i), M))(nn))
    n64 = np.full(PLANTED_M, 64, np.int32)
    F1, F2, K1, K2, n1, n2 = _gather_host(c["q_feat"], c["q_kp"], n64, c["map_feat"], c["map_kp"], np.full(M, 64, np.int32), nn)
    want = gpu.register_pairs(_cu(F1), _cu(F2), _cu(K1), _cu(K2), n1=_cu(n1), n2=_cu(n2), T_gt=_cu(T_gt.reshape(-1, 4, 4)),
                              ransac_max_it=H, seed=seed, pair_ids=_cu(pids.reshape(-1)))
    torch.cuda.synchronize()
    for mine, theirs in (("T", "T"), ("inliers", "inliers"), ("fitness", "fitness"), ("inlier_rmse", "inlier_rmse"),
                         ("best_t", "best_t"), ("pair_status", "status"), ("corr", "corr"), ("n_corr", "n_corr"), ("rte", "rte"),
                         ("rre", "rre"), ("success", "success")):
        w = _np(want[theirs])
        assert np.array_equal(r[mine], w.reshape(r[mine].shape)), mine
    _check_pick(r, nn, M, poses, min_inliers=5)
    assert r["status"][1] == NO_CANDIDATE | BAD_INDEX | UNVERIFIED and r["best_index"][1] == -1 and r["safe_pick"][1] == 0
    assert np.array_equal(r["pose"][1], np.eye(4)) and (r["reranked"][1] == -1).all()
    assert r["status"][5] == NO_CANDIDATE and r["status"][4] == NO_CANDIDATE | BAD_INDEX and r["best_index"][4] == 4
    assert (r["best_index"][[0, 2, 3, 5]] == [0, 2, 3, 5]).all()
    # min_inliers just above the best count leaves a query unverified: the restated rule again, on the device's tables
    hi = gpu.verify_candidates(_cu(c["q_feat"]), _cu(c["q_kp"]), None, km, _cu(nn), query_ids=_cu(qid), seed=seed, ransac_max_it=H,
                               min_inliers=int(r["best_inliers"].max()) + 1)
    torch.cuda.synchronize()
    hi = {k: _np(v) for k, v in hi.items() if not k.startswith("_")}
    assert "rte" not in hi and "best_rte" not in hi and np.array_equal(hi["T"], r["T"])
    assert (hi["best_index"] == -1).all() and (hi["status"] & UNVERIFIED).all() and np.array_equal(hi["safe_pick"], np.clip(nn[:, 0], 0, M - 1))
    _check_pick(hi, nn, M, poses, min_inliers=int(r["best_inliers"].max()) + 1)


# ------------------------------------------------------------------ 4. planted relocalisation
@pytest.mark.parametrize("utm", [False, True])
def test_planted_relocalization(gpu, utm):
    from egonn_amd import _lib
    c, poses, T_gt, r = _planted_run(gpu, utm)
    solved = planted_solved()[1]
    assert np.array_equal(r["best_index"], np.arange(PLANTED_M)) and np.array_equal(r["best_rank"], np.arange(PLANTED_M) % PLANTED_K)
    assert np.array_equal(r["reranked"][:, 0], c["truth"]) and r["reranked"][WEAK_OF, 1] == PLANTED_M and (r["status"] == 0).all()
    assert (r["best_success"] == 1).all() and np.array_equal(r["best_inliers"], [solved[(q, q)]["inliers"] for q in range(PLANTED_M)])
    q_poses = np.stack([poses[q] @ c["T_planted"][q] for q in range(PLANTED_M)])
    for q in range(PLANTED_M):
        rte, rre, suc = metrics_f64(r["pose"][q], q_poses[q])
        assert suc == 1 and rte <= 2.0 and rre <= 5.0, (q, rte, rre)
    # recall@n on the reranked and on the original lists (positions offset by a common float64 origin, as recall_at_k does)
    origin = poses[:, :2, 3].mean(0)
    mp, qp = _cu((poses[:, :2, 3] - origin).astype(np.float32)), _cu((q_poses[:, :2, 3] - origin).astype(np.float32))
    dist = np.linalg.norm(q_poses[:, None, :2, 3] - poses[None, :, :2, 3], axis=-1)           # (6, 7) float64
    radius = 25.0                                           # planted translations reach 20 m; map entries lie > 150 m apart
    assert np.abs(dist - radius).min() > 1.0
    lib, rad = _lib.load(), _cu(np.array([radius], np.float32))
    for lists, first_hit in ((r["reranked"], np.zeros(PLANTED_M, int)),
                             (c["nn"], (np.take_along_axis(dist, c["nn"].astype(np.int64), 1) <= radius).argmax(1))):
        tp = torch.zeros((1, PLANTED_K), dtype=torch.int32, device="cuda")
        _lib.call(tp.device, lib.egonn_recall_counts, _cu(lists.astype(np.int32)).data_ptr(), qp.data_ptr(), mp.data_ptr(), PLANTED_M,
                  PLANTED_K, 2, rad.data_ptr(), 1, tp.data_ptr())
        want = [(first_hit <= n).sum() for n in range(PLANTED_K)]
        assert _np(tp)[0].tolist() == want, (_np(tp), want)
    assert want[0] < PLANTED_M                              # the original lists: the true place at rank 0 for some queries only


# ------------------------------------------------------------------ 5. invariances
def test_invariances(gpu):
    c, poses, T_gt, full = _planted_run(gpu)
    km = _kmap(gpu, c, poses)
    again = _verify(gpu, c, km, c["nn"], T_gt)
    for k in PAIR_KEYS + QUERY_KEYS:
        assert np.array_equal(again[k], full[k]), k                                   # two runs
    for q in range(PLANTED_M):                                                        # one query at a time, the same ids
        one = _verify(gpu, c, km, c["nn"][q:q + 1], T_gt[q:q + 1], rows=slice(q, q + 1))
        for k in PAIR_KEYS + QUERY_KEYS:
            assert np.array_equal(one[k][0], full[k][q]), (k, q)
    perm = np.array([2, 0, 3, 1])                                                     # a permuted candidate row
    pr = _verify(gpu, c, km, c["nn"][:, perm], T_gt[:, perm])
    for k in PAIR_KEYS:
        assert np.array_equal(pr[k], full[k][:, perm]), k
    for k in ("best_index", "T_rel", "pose", "best_inliers", "status", "best_rte", "best_rre", "best_success"):
        assert np.array_equal(pr[k], full[k]), k
    assert np.array_equal(pr["reranked"][:, 0], full["reranked"][:, 0])
    ch = _verify(gpu, c, km, c["nn"], T_gt, chunk_pairs=8)                            # 24 pairs in chunks of 2 queries
    ch1 = _verify(gpu, c, km, c["nn"], T_gt, chunk_pairs=1)                           # one query per chunk at the least
    for k in PAIR_KEYS + QUERY_KEYS:
        assert np.array_equal(ch[k], full[k]) and np.array_equal(ch1[k], full[k]), k


def test_graph_replay_on_changed_inputs(gpu):
    """the whole sequence captured once (egonn_graph_begin / egonn_graph_end) on preallocated buffers, replayed on a changed
    nn_index and changed query descriptors, equals the eager call on them"""
    from egonn_amd import _lib
    lib = _lib.load()
    c, poses, T_gt = _planted_inputs(False)
    km = _kmap(gpu, c, poses)
    rng = np.random.default_rng(9)
    f2 = c["q_feat"] + 0.01 * rng.standard_normal(c["q_feat"].shape).astype(np.float32)
    f2 = (f2 / np.linalg.norm(f2, axis=-1, keepdims=True)).astype(np.float32)
    nn2 = c["nn"][:, ::-1].copy()
    nn2[0, 0] = -1
    gt2 = c["T_planted"][np.clip(nn2, 0, PLANTED_M)]
    qf, qk, qn = _cu(c["q_feat"]), _cu(c["q_kp"]), _cu(np.full(PLANTED_M, 64, np.int32))
    nn, gt, qid = _cu(c["nn"]), _cu(T_gt), _cu(np.arange(PLANTED_M, dtype=np.int32))
    kw = dict(query_ids=qid, T_gt=gt, ransac_max_it=PLANTED_H)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        out = gpu.verify_candidates(qf, qk, qn, km, nn, **kw)                         # eager once: every buffer exists now
        st.synchronize()
        g = ctypes.c_void_p()
        _lib.check(lib.egonn_graph_begin(st.cuda_stream))
        try:
            gpu.verify_candidates(qf, qk, qn, km, nn, out=out, **kw)
        finally:
            rc = lib.egonn_graph_end(st.cuda_stream, ctypes.byref(g))
        _lib.check(rc)
        qf.copy_(_cu(f2))
        nn.copy_(_cu(nn2))
        gt.copy_(_cu(gt2))
        for k in PAIR_KEYS + QUERY_KEYS:
            out[k].fill_(-3)
        _lib.check(lib.egonn_graph_launch(g, st.cuda_stream))
        st.synchronize()
    got = {k: _np(out[k]) for k in PAIR_KEYS + QUERY_KEYS}
    lib.egonn_graph_destroy(g)
    torch.cuda.current_stream().wait_stream(st)
    c2 = dict(c, q_feat=f2)
    want = _verify(gpu, c2, km, nn2, gt2)
    for k in PAIR_KEYS + QUERY_KEYS:
        assert np.array_equal(got[k], want[k]), k
    assert want["match_status"][0, 0] == NO_CANDIDATE and (want["best_index"][1:] == np.arange(1, PLANTED_M)).all()
    with pytest.raises(ValueError, match="other shapes"):
        gpu.verify_candidates(qf[:3], qk[:3], qn[:3], km, nn[:3], out=out)


# ------------------------------------------------------------------ 6. the descriptor path end to end
def test_end_to_end_from_scans(gpu):
    from egonn_amd.synth import lidar_scan, seeded_state_dict
    from tests.test_gpu_registration import BAND, ROT_TOL
    mp = gpu.ModelParams(model="egonn", coordinates="cartesian", quantization_step=0.1)
    model = gpu.model_factory(mp)
    sd = seeded_state_dict(7, {k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to("cuda:0").eval()
    scans = [torch.from_numpy(lidar_scan(20 + i, n_points=6000)) for i in range(4)]
    ex = gpu.DescriptorExtractor(model, n_k=128)
    poses = planted_map_poses(4, utm=True)
    km = gpu.KeypointMap(n_k=128, dim=model.local_descriptor_size, global_dim=model.global_descriptor_size)
    km.add(ex.extract(scans), poses)
    assert len(km) == 4 and km.descriptors.is_cuda
    H = 2000
    reloc = gpu.Relocalizer(ex, km, k=3, ransac_max_it=H)
    r = reloc.localize([s.clone() for s in scans])
    assert np.array_equal(_np(r["best_index"]), np.arange(4)) and np.array_equal(_np(r["nn_index"])[:, 0], np.arange(4))
    T = _np(r["T_rel"])
    for q in range(4):
        assert np.linalg.norm(T[q, :3, :3] - np.eye(3)) / np.sqrt(2) <= ROT_TOL and np.abs(T[q, :3, 3]).max() <= BAND, (q, T[q])
        assert np.array_equal(T[q, 3], [0, 0, 0, 1])
    assert np.abs(_np(r["pose"]) - poses).max() <= 1e-6                    # |t| ~ 4e6 m: the product rounds at 1e-9
    # the hand-made chain
    y = ex.extract(scans)
    nn, _ = gpu.retrieval.knn(y["global"], km.globals, 3)
    v = gpu.verify_candidates(y["descriptors"], y["keypoints"], y["count"], km, nn, ransac_max_it=H)
    torch.cuda.synchronize()
    assert torch.equal(nn, r["nn_index"])
    for k in ("T", "inliers", "fitness", "inlier_rmse", "best_t", "pair_status", "match_status", "corr", "n_corr", "pair_ids",
              "best_rank", "best_index", "reranked", "T_rel", "pose", "safe_pick", "best_inliers", "status"):
        assert torch.equal(v[k], r[k]), k
    # candidates from elsewhere, the scan itself at rank 2: reranked to rank 0
    own = np.array([[(q + 1) % 4, (q + 2) % 4, q] for q in range(4)], np.int32)
    r2 = reloc.localize(scans, nn_index=own)
    assert np.array_equal(_np(r2["reranked"])[:, 0], np.arange(4)) and (_np(r2["best_rank"]) == 2).all()
    assert np.array_equal(_np(r2["nn_index"]), own) and torch.equal(r2["T_rel"], r["T_rel"])      # pair ids: rank-free


# ------------------------------------------------------------------ 7. refinement
class _TableExtractor:
    """an extractor over precomputed descriptors (Relocalizer takes any object with `extract`): the rows `self.rows` of its
    tables, or, when that is None, the rows the "scans" name as integers"""

    def __init__(self, glob, kp, desc):
        self.glob, self.kp, self.desc, self.rows = _cu(glob), _cu(kp), _cu(desc), None

    def extract(self, scans):
        rows = [int(s) for s in scans] if self.rows is None else self.rows
        assert len(rows) == len(scans)
        i = torch.as_tensor(rows, device="cuda")
        return {"global": self.glob[i], "keypoints": self.kp[i], "descriptors": self.desc[i]}


def test_refinement(gpu):
    """Keypoints with 0.15 m noise per coordinate bound what a three-point RANSAC pose can reach; ICP averages thousands of
    points with 0.02 m noise, so it must end nearer the planted pose than its initialisation T_rel."""
    from egonn_amd.synth import planted_scan_pair
    n = 3
    pairs = [planted_pair(64, 7100 + m, 0.30, 0.15) for m in range(n)]
    qc, mc = [], []
    for i, p in enumerate(pairs):                        # clouds that move by the pair's planted pose (ZYX angles of its rotation)
        R = p[4][:3, :3]
        ypr = (np.arctan2(R[1, 0], R[0, 0]), -np.arcsin(R[2, 0]), np.arctan2(R[2, 1], R[2, 2]))
        s, t, Tp, _ = planted_scan_pair(60 + i, 5000, translation=p[4][:3, 3], yaw_pitch_roll=ypr)
        assert np.abs(Tp - p[4]).max() < 1e-9
        qc.append(s)
        mc.append(t)
    crop = (-80, 80, -80, 80, -30.0, None)
    poses = planted_map_poses(n)
    km = gpu.KeypointMap(n_k=64, dim=128, global_dim=8)
    km.add({"global": torch.eye(8)[:n], "keypoints": torch.from_numpy(np.stack([p[3] for p in pairs])),
            "descriptors": torch.from_numpy(np.stack([p[1] for p in pairs]))}, poses)
    km.clouds = gpu.CloudBank(crop=crop).add(mc)
    with pytest.raises(ValueError, match="kmap.clouds"):
        gpu.Relocalizer(None, gpu.KeypointMap(n_k=64, dim=128, global_dim=8), refine=True)
    # a fourth query without candidates: its tables are query 0's
    ex = _TableExtractor(np.eye(8, dtype=np.float32)[[0, 1, 2, 0]], np.stack([p[2] for p in pairs] + [pairs[0][2]]),
                         np.stack([p[0] for p in pairs] + [pairs[0][0]]))
    reloc = gpu.Relocalizer(ex, km, k=2, ransac_max_it=2000, refine=True)
    nn3 = np.array([[1, 0], [1, 2], [2, 0]], np.int32)
    ex.rows = [0, 1, 2]
    r = reloc.localize(qc, nn_index=nn3)
    assert np.array_equal(_np(r["best_index"]), np.arange(n)) and (_np(r["icp_status"]) == 0).all()
    # by hand on the same gathered operands
    pts = torch.cat([torch.from_numpy(np.ascontiguousarray(s)) for s in qc]).cuda()
    off = torch.tensor(np.concatenate([[0], np.cumsum([len(s) for s in qc])]), dtype=torch.int64).cuda()
    qd = gpu.voxel_downsample(pts, off, km.clouds.voxel_size, crop)
    g = km.clouds.gather(_np(r["safe_pick"]).tolist())
    icp = gpu.icp_pairs(qd["points"], qd["offsets"], g["points"], g["offsets"], r["T_rel"])
    torch.cuda.synchronize()
    assert torch.equal(icp["T"], r["T_icp"]) and torch.equal(icp["fitness"], r["icp_fitness"])
    assert torch.equal(icp["inlier_rmse"], r["icp_inlier_rmse"]) and torch.equal(icp["status"], r["icp_status"])
    T_icp, T_rel, refined = _np(r["T_icp"]), _np(r["T_rel"]), _np(r["pose_refined"])
    for q in range(n):
        assert np.array_equal(refined[q], pose_product_f64(poses[q], T_icp[q])), q
        e_icp, e_rel = np.linalg.norm(T_icp[q] - pairs[q][4]), np.linalg.norm(T_rel[q] - pairs[q][4])
        print(f"[relocalize] refinement query {q}: |T_rel - T_planted|_F {e_rel:.4f}, |T_icp - T_planted|_F {e_icp:.4f}, "
              f"fitness {_np(r['icp_fitness'])[q]:.3f}")
        assert e_icp < e_rel, (q, e_icp, e_rel)
    # an unverified query in the batch leaves the others' refined poses unchanged
    ex.rows = [0, 1, 2, 3]
    r4 = reloc.localize(qc + [qc[0]], nn_index=np.concatenate([nn3, [[-1, -1]]]).astype(np.int32))
    assert _np(r4["best_index"]).tolist() == [0, 1, 2, -1] and _np(r4["status"])[3] == NO_CANDIDATE | UNVERIFIED
    assert _np(r4["safe_pick"])[3] == 0 and int(g["status"]) == 0
    for k in ("pose_refined", "T_icp", "icp_fitness", "icp_inlier_rmse", "icp_status", "pose", "T_rel"):
        assert torch.equal(r4[k][:n], r[k]), k


# ------------------------------------------------------------------ 8. evaluate_relocalization
def test_evaluate_relocalization(gpu):
    c, poses, _ = _planted_inputs(False)
    _, solved = planted_solved()
    M = PLANTED_M + 1
    km = _kmap(gpu, c, poses)
    # global descriptors that retrieve exactly the planted lists: map entry m = e_m, query q = weights falling with the rank
    glob = np.zeros((PLANTED_M, 8), np.float32)
    for q in range(PLANTED_M):
        glob[q, c["nn"][q]] = [0.9, 0.8, 0.7, 0.6]
    ex = _TableExtractor(glob, c["q_kp"], c["q_feat"])
    reloc = gpu.Relocalizer(ex, km, k=PLANTED_K, ransac_max_it=PLANTED_H)
    q_poses = np.stack([poses[q] @ c["T_planted"][q] for q in range(PLANTED_M)])
    radius = (5, 25)
    res = gpu.evaluate_relocalization(reloc, list(range(PLANTED_M)), q_poses, radius=radius, batch_size=4)
    # the same from the restatement
    dist = np.linalg.norm(q_poses[:, None, :2, 3] - poses[None, :, :2, 3], axis=-1)
    assert min(np.abs(dist - r).min() for r in radius) > 1e-3
    reranked, inl, rte, rre = [], [], [], []
    for q in range(PLANTED_M):
        rows = [solved[(q, int(m))] for m in c["nn"][q]]
        p = pick_f64(c["nn"][q], M, [x["T"] for x in rows], [x["inliers"] for x in rows], [x["inlier_rmse"] for x in rows],
                     [x["status"] for x in rows], poses, 0, [x["rte"] for x in rows], [x["rre"] for x in rows],
                     [x["success"] for x in rows])
        assert p["best_success"] == 1
        reranked.append(p["reranked"])
        inl.append(p["best_inliers"])
        rte.append(p["best_rte"])
        rre.append(p["best_rre"])
    for name, lists in (("recall", c["nn"]), ("recall_reranked", np.stack(reranked))):
        for r in radius:
            hit = np.take_along_axis(dist, np.maximum(lists, 0).astype(np.int64), 1) <= r
            want = [float(hit[:, : n + 1].any(1).mean()) for n in range(PLANTED_K)]
            assert res[name][r] == want, (name, r, res[name][r], want)
    assert res["recall_reranked"][25] == [1.0] * PLANTED_K and res["recall"][25][0] < 1.0
    assert res["success"] == 1.0 and res["unverified"] == 0.0 and res["failure_inliers"] == 0.0
    assert res["success_inliers"] == float(np.mean(inl)) == 45.0
    assert abs(res["rte"] - np.mean(rte)) <= 1e-9 and abs(res["rre"] - np.mean(rre)) <= 1e-5
    # a threshold nobody reaches: every query unverified, a failure with 0 inliers; the retrieved lists are what they were
    none = gpu.evaluate_relocalization(gpu.Relocalizer(ex, km, k=PLANTED_K, ransac_max_it=PLANTED_H, min_inliers=64),
                                       list(range(PLANTED_M)), q_poses, radius=radius)
    assert none["unverified"] == 1.0 and none["success"] == 0.0 and none["failure_inliers"] == 0.0 and none["rte"] == 0.0
    assert none["recall"] == res["recall"]

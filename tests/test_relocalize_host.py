"""CPU tests of the relocalisation layer (egonn_match_candidates / egonn_gather_candidates / egonn_pick_candidates, KeypointMap)
and the home of its float64 restatement and of the planted case, which tests/test_gpu_relocalize.py imports.

Restated contract (egonn_amd/csrc/relocalize.hip):
  pair id        (query id * 1000003 + map index) mod 2^30: the id of the RANSAC draws of (query, map entry)
  match status   index -1 -> NO_CANDIDATE (1); index < -1 or >= M -> NO_CANDIDATE | BAD_INDEX (3); an empty pair either way
  order          valid candidates by most inliers, then lowest inlier_rmse, then lowest rank; invalid ones last in rank order
  winner         the head of the order if it is valid, has a model and inliers >= min_inliers, else UNVERIFIED (4)
  pose           map_pose[best] @ T as the affine product: ((a_r0 b_0c + a_r1 b_1c) + a_r2 b_2c) [+ a_r3], last row 0 0 0 1

The planted case: M = 6 map entries, entry m = the target side of planted_pair(64, 7000 + m, 0.30, 0.05) and query m its source
side; k = 4 candidates per query with the true entry at rank q % 4; entry 6 is the "weak" twin of entry WEAK_OF (same seed,
so the same source and pose, with 80 % outliers) and sits in that query's list."""
import os
import re

import numpy as np
import pytest
import torch

from tests.test_registration_host import STATUS_NO_MODEL, planted_pair, register_f64, rot_zyx

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_CANDIDATE, BAD_INDEX, UNVERIFIED = 1, 2, 4
NEW_SYMBOLS = ["egonn_match_candidates_scratch_bytes", "egonn_match_candidates", "egonn_gather_candidates",
               "egonn_pick_candidates"]
PLANTED_M, PLANTED_K, PLANTED_H, WEAK_OF = 6, 4, 1024, 2


# ------------------------------------------------------------------ restatement
def pair_id(query_id, map_index):
    return (int(query_id) * 1000003 + int(map_index)) % (1 << 30)


def match_status(index, M):
    return 0 if 0 <= index < M else (NO_CANDIDATE if index == -1 else NO_CANDIDATE | BAD_INDEX)


def pose_product_f64(A, B):
    """elementwise float64 in the stated order (Python floats: IEEE double operations, no contraction)"""
    out = np.zeros((4, 4))
    out[3, 3] = 1.0
    for r in range(3):
        for c in range(4):
            v = float(A[r, 0]) * float(B[0, c]) + float(A[r, 1]) * float(B[1, c])
            v = v + float(A[r, 2]) * float(B[2, c])
            if c == 3:
                v = v + float(A[r, 3])
            out[r, c] = v
    return out


def pick_f64(nn_row, M, T, inliers, rmse, reg_status, map_pose, min_inliers=0, rte=None, rre=None, success=None):
    """one query: -> dict with the fields of egonn_pick_candidates"""
    k = len(nn_row)
    valid = [0 <= int(i) < M for i in nn_row]
    order = sorted(range(k), key=lambda c: (0, -int(inliers[c]), float(rmse[c]), c) if valid[c] else (1, 0, 0.0, c))
    first = order[0]
    ok = valid[first] and not (int(reg_status[first]) & STATUS_NO_MODEL) and int(inliers[first]) >= min_inliers
    st = 0
    for i in nn_row:
        st |= match_status(int(i), M)
    out = dict(reranked=np.array([int(nn_row[c]) if valid[c] else -1 for c in order], np.int32),
               best_rank=first if ok else -1, best_index=int(nn_row[first]) if ok else -1,
               T_rel=np.array(T[first], dtype=np.float64) if ok else np.eye(4),
               pose=pose_product_f64(map_pose[int(nn_row[first])], T[first]) if ok else np.eye(4),
               safe_pick=int(nn_row[first]) if ok else min(max(int(nn_row[0]), 0), M - 1),
               best_inliers=int(inliers[first]) if ok else 0, status=st | (0 if ok else UNVERIFIED))
    if rte is not None:
        out.update(best_rte=float(rte[first]) if ok else -1.0, best_rre=float(rre[first]) if ok else -1.0,
                   best_success=int(success[first]) if ok else 0)
    return out


# ------------------------------------------------------------------ the planted case
def planted_map_poses(M, utm=False, seed=77):
    """rigid map poses: yaw anywhere, small pitch / roll, places 170 m apart along a line, local or UTM-sized"""
    rng = np.random.default_rng(seed)
    P = np.tile(np.eye(4), (M, 1, 1))
    for m in range(M):
        P[m, :3, :3] = rot_zyx(rng.uniform(-np.pi, np.pi), np.deg2rad(rng.uniform(-3, 3)), np.deg2rad(rng.uniform(-3, 3)))
        P[m, :3, 3] = np.array([150.0 * m, -80.0 * m, 0.0]) + rng.uniform(-5, 5, 3) + (np.array([3.5e5, 4.0e6, 0.0]) if utm else 0.0)
    return P


def planted_case():
    """-> dict: q_feat / q_kp (6, 64, .), map_feat / map_kp (7, 64, .), T_planted (7,4,4) (entry 6: that of WEAK_OF),
    nn (6, 4) int32, truth (6,) the true entry per query"""
    pairs = [planted_pair(64, 7000 + m, 0.30, 0.05) for m in range(PLANTED_M)]
    weak = planted_pair(64, 7000 + WEAK_OF, 0.80, 0.05)
    assert np.array_equal(weak[0], pairs[WEAK_OF][0]) and np.array_equal(weak[2], pairs[WEAK_OF][2])   # the same source
    assert np.array_equal(weak[4], pairs[WEAK_OF][4])                                                  # and the same pose
    entries = pairs + [weak]
    nn = np.zeros((PLANTED_M, PLANTED_K), np.int32)
    for q in range(PLANTED_M):
        others = [(q + 1) % PLANTED_M, (q + 2) % PLANTED_M, (q + 3) % PLANTED_M]
        if q == WEAK_OF:
            others[0] = PLANTED_M                                  # the weak twin among this query's candidates
        others.insert(q % PLANTED_K, q)
        nn[q] = others
    return dict(q_feat=np.stack([p[0] for p in pairs]), q_kp=np.stack([p[2] for p in pairs]),
                map_feat=np.stack([p[1] for p in entries]), map_kp=np.stack([p[3] for p in entries]),
                T_planted=np.stack([p[4] for p in entries]), nn=nn, truth=np.arange(PLANTED_M))


_SOLVED = {}


def planted_solved():
    """register_f64 of every (query, candidate) of the planted case with the pair-id rule, H = 1024, seed 0: computed once"""
    if not _SOLVED:
        c = planted_case()
        res = {}
        for q in range(PLANTED_M):
            for m in c["nn"][q]:
                res[(q, int(m))] = register_f64(c["q_feat"][q], c["map_feat"][m], c["q_kp"][q], c["map_kp"][m], c["T_planted"][m],
                                                seed=0, pair_id=pair_id(q, m), H=PLANTED_H)
        _SOLVED.update(case=c, res=res)
    return _SOLVED["case"], _SOLVED["res"]


# ------------------------------------------------------------------ tests
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


def test_new_symbols_declared_and_exported(built):
    import egonn_amd
    from egonn_amd import _lib, relocalize
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "egonn_hip.h")).read()
    declared = set(re.findall(r"\b(egonn_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    for name in ("EGONN_RELOC_NO_CANDIDATE = 1", "EGONN_RELOC_BAD_INDEX = 2", "EGONN_RELOC_UNVERIFIED = 4"):
        assert name in header
    assert (relocalize.RELOC_NO_CANDIDATE, relocalize.RELOC_BAD_INDEX, relocalize.RELOC_UNVERIFIED) == (1, 2, 4)
    for name in ("KeypointMap", "verify_candidates", "Relocalizer", "evaluate_relocalization"):
        assert getattr(egonn_amd, name) is getattr(relocalize, name) and name in egonn_amd.__all__
    # 64-row x 32-column tiles: (cdiv(n, 64) + cdiv(n, 32)) * n partial minima per pair, a double and an int32 each
    assert lib.egonn_match_candidates_scratch_bytes(1, 20, 128) == 20 * (2 + 4) * 128 * 12
    assert lib.egonn_match_candidates_scratch_bytes(3, 2, 200) == 6 * (4 + 7) * 200 * 12
    assert lib.egonn_match_candidates_scratch_bytes(1, 1, 257) == -1 and lib.egonn_match_candidates_scratch_bytes(1, 0, 128) == -1


def test_argument_checks_need_no_gpu(built):
    """every up-front refusal returns the library's invalid status before anything is launched"""
    from egonn_amd import _lib
    lib = _lib.load()
    one, big = 16, 1 << 30      # non-null, aligned, never dereferenced: every call below fails its argument check first

    def match(q_feat=one, bank_feat=one, nn=one, k=2, n_max=128, dim=128, corr=one, scratch=one, nbytes=big, M=3):
        return lib.egonn_match_candidates(q_feat, one, bank_feat, one, nn, 1, k, M, n_max, dim, corr, one, None, scratch, nbytes,
                                          None)
    need = lib.egonn_match_candidates_scratch_bytes(1, 2, 128)
    assert need > 0
    for kw, word in ((dict(q_feat=None), b"null"), (dict(bank_feat=None), b"null"), (dict(nn=None), b"null"),
                     (dict(corr=None), b"null"), (dict(scratch=None), b"null"), (dict(k=0), b"k=0"),
                     (dict(n_max=257), b"n_max=257"), (dict(dim=6), b"width 6"), (dict(nbytes=need - 1), b"scratch needs"),
                     (dict(q_feat=one + 4), b"16-byte aligned"), (dict(bank_feat=one + 8), b"16-byte aligned"),
                     (dict(scratch=one + 4), b"8-byte aligned"), (dict(M=0), b"at least one entry")):
        assert match(**kw) == 1, kw
        assert word in lib.egonn_last_error(), (kw, lib.egonn_last_error())
    g = lambda **kw: lib.egonn_gather_candidates(kw.get("q_kp", one), one, one, one, one, None, 1, kw.get("k", 2), 3,      # noqa: E731
                                                 kw.get("n_max", 128), one, one, one, one, kw.get("pair_id", one), None)
    assert g(q_kp=None) == 1 and g(pair_id=None) == 1 and g(k=0) == 1 and g(n_max=257) == 1

    def pick(nn=one, k=2, pose=one, min_inliers=0, M=3):
        return lib.egonn_pick_candidates(nn, 1, k, M, one, one, one, one, one, None, None, None, min_inliers, one, one, one, one,
                                         pose, one, one, one, None, None, None, None)
    assert pick(nn=None) == 1 and pick(pose=None) == 1 and pick(k=0) == 1 and pick(k=1025) == 1 and pick(M=0) == 1
    assert pick(min_inliers=-1) == 1 and b"min_inliers" in lib.egonn_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_relocalization_has_no_cpu_path(built):
    import egonn_amd
    c = planted_case()
    km = egonn_amd.KeypointMap(n_k=64, dim=128, global_dim=8, device="cpu")
    km.add({"global": torch.zeros(7, 8), "keypoints": torch.from_numpy(c["map_kp"]), "descriptors": torch.from_numpy(c["map_feat"])},
           planted_map_poses(7))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        egonn_amd.verify_candidates(torch.from_numpy(c["q_feat"]), torch.from_numpy(c["q_kp"]), None, km, c["nn"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        egonn_amd.KeypointMap()


def test_keypoint_map_round_trip(tmp_path):
    import egonn_amd
    rng = np.random.default_rng(3)
    km = egonn_amd.KeypointMap(n_k=16, dim=8, global_dim=12, device="cpu")
    assert len(km) == 0 and km.descriptors.shape == (0, 16, 8)
    batches, poses = [], []
    for b in (1, 3, 2, 7):                                           # grows several times
        batches.append({"global": torch.from_numpy(rng.standard_normal((b, 12)).astype(np.float32)),
                        "keypoints": torch.from_numpy(rng.standard_normal((b, 16, 3)).astype(np.float32)),
                        "descriptors": torch.from_numpy(rng.standard_normal((b, 16, 8)).astype(np.float32)),
                        "count": torch.from_numpy(rng.integers(0, 17, b).astype(np.int32))})
        poses.append(planted_map_poses(b, utm=True, seed=b))
        km.add(batches[-1], poses[-1])
    assert len(km) == 13
    assert torch.equal(km.globals, torch.cat([x["global"] for x in batches]))
    assert torch.equal(km.descriptors, torch.cat([x["descriptors"] for x in batches]))
    assert torch.equal(km.keypoints, torch.cat([x["keypoints"] for x in batches]))
    assert torch.equal(km.counts, torch.cat([x["count"] for x in batches])) and km.counts.dtype == torch.int32
    assert np.array_equal(km.poses.numpy(), np.concatenate(poses)) and km.poses.dtype == torch.float64      # UTM poses exactly
    no_count = {k: v for k, v in batches[0].items() if k != "count"}
    km.add(no_count, poses[0])
    assert int(km.counts[-1]) == 16
    with pytest.raises(ValueError, match="KeypointMap.add"):
        km.add({**batches[0], "descriptors": torch.zeros(1, 16, 4)}, poses[0])
    with pytest.raises(ValueError):
        egonn_amd.KeypointMap(n_k=257, device="cpu")
    with pytest.raises(ValueError):
        egonn_amd.KeypointMap(dim=6, device="cpu")
    # a CloudBank rides along in the same file
    bank = egonn_amd.CloudBank(crop=(-10.0, 10.0, None, None, -1.0, 5.0), voxel_size=0.2, device="cpu")
    bank.points = torch.from_numpy(rng.standard_normal((30, 3)))
    bank.host_offsets, bank.status = [0, 4, 4, 30], [0, 0, 8]
    km.clouds = bank
    path = str(tmp_path / "map.npz")
    km.save(path)
    back = egonn_amd.KeypointMap.load(path, device="cpu")
    assert (back.n_k, back.dim, back.global_dim, len(back)) == (16, 8, 12, 14)
    for name in ("globals", "keypoints", "descriptors", "counts", "poses"):
        assert torch.equal(getattr(back, name), getattr(km, name)) and getattr(back, name).dtype == getattr(km, name).dtype, name
    assert torch.equal(back.clouds.points, bank.points) and back.clouds.host_offsets == [0, 4, 4, 30]
    assert back.clouds.status == [0, 0, 8] and back.clouds.voxel_size == 0.2
    assert back.clouds.crop == (-10.0, 10.0, None, None, -1.0, 5.0)
    km.clouds = None
    km.save(path)
    assert egonn_amd.KeypointMap.load(path, device="cpu").clouds is None


def test_pair_id_rule():
    assert pair_id(0, 5) == 5 and pair_id(3, 2) == 3000011
    assert pair_id(2000, 7) == (2000 * 1000003 + 7) % (1 << 30) == 2000006007 - (1 << 30)
    assert pair_id(5, -1) == 5 * 1000003 - 1 and pair_id(0, -1) == (1 << 30) - 1 and pair_id(-1, 0) == (1 << 30) - 1000003
    ids = {pair_id(q, m) for q in range(64) for m in range(64)}
    assert len(ids) == 64 * 64                                       # no collisions among a batch's pairs
    assert [match_status(i, 5) for i in (2, -1, 5, -7)] == [0, 1, 3, 3]


def test_pick_rule_and_pose_product_on_hand_made_tables():
    M = 5
    poses = planted_map_poses(M, utm=True)
    rng = np.random.default_rng(0)
    T = np.tile(np.eye(4), (4, 1, 1))
    for c in range(4):
        T[c, :3, :3], T[c, :3, 3] = rot_zyx(*rng.uniform(-1, 1, 3)), rng.uniform(-20, 20, 3)
    none = [0, 0, 0, 0]
    # a tie on inliers broken by rmse
    r = pick_f64([3, 1, 4, 0], M, T, [10, 30, 30, 5], [0.1, 0.3, 0.2, 0.1], none, poses)
    assert r["reranked"].tolist() == [4, 1, 3, 0] and (r["best_rank"], r["best_index"], r["best_inliers"], r["status"]) == (2, 4, 30, 0)
    assert r["safe_pick"] == 4 and np.array_equal(r["T_rel"], T[2])
    # the pose product: last row exact, and the matrix product to rounding (|t| ~ 4e6: one ulp is 1e-9)
    want = poses[4] @ T[2]
    assert np.array_equal(r["pose"][3], [0, 0, 0, 1]) and np.abs(r["pose"] - want).max() < 1e-8
    assert np.array_equal(r["pose"][:3, :3], np.array([[(poses[4][i, 0] * T[2][0, j] + poses[4][i, 1] * T[2][1, j]) +
                                                        poses[4][i, 2] * T[2][2, j] for j in range(3)] for i in range(3)]))
    # a full tie broken by rank
    r = pick_f64([2, 0], M, T, [7, 7], [0.5, 0.5], none, poses)
    assert r["reranked"].tolist() == [2, 0] and r["best_rank"] == 0
    # more inliers beat a lower rmse; a candidate without a model at the head leaves the query unverified
    r = pick_f64([2, 0], M, T, [7, 8], [0.1, 0.5], none, poses)
    assert r["reranked"].tolist() == [0, 2] and r["best_index"] == 0
    r = pick_f64([2, 0], M, T, [0, 0], [0.0, 0.0], [STATUS_NO_MODEL, STATUS_NO_MODEL], poses)
    assert r["best_rank"] == -1 and r["status"] == UNVERIFIED and r["safe_pick"] == 2 and r["reranked"].tolist() == [2, 0]
    # an all-invalid row
    r = pick_f64([-1, -1, 9, -7], M, T, none, [0.0] * 4, [STATUS_NO_MODEL] * 4, poses)
    assert r["reranked"].tolist() == [-1] * 4 and r["best_rank"] == -1 and r["best_index"] == -1 and r["best_inliers"] == 0
    assert r["status"] == NO_CANDIDATE | BAD_INDEX | UNVERIFIED and r["safe_pick"] == 0
    assert np.array_equal(r["pose"], np.eye(4)) and np.array_equal(r["T_rel"], np.eye(4))
    assert pick_f64([9, 1], M, T, [0, 3], [0.0, 0.1], none, poses)["safe_pick"] == 1       # verified: the winner
    assert pick_f64([9, 1], M, T, [0, 3], [0.0, 0.1], none, poses, min_inliers=4)["safe_pick"] == 4    # else rank 0, clamped
    # invalid candidates go last in rank order, whatever their tables hold
    r = pick_f64([-1, 3, 7, 1], M, T, [99, 4, 99, 6], [0.0, 0.2, 0.0, 0.4], none, poses)
    assert r["reranked"].tolist() == [1, 3, -1, -1] and r["best_rank"] == 3 and r["status"] == NO_CANDIDATE | BAD_INDEX
    # min_inliers just above and just at the best count
    args = ([3, 1, 4, 0], M, T, [10, 30, 30, 5], [0.1, 0.3, 0.2, 0.1], none, poses)
    above, at = pick_f64(*args, min_inliers=31), pick_f64(*args, min_inliers=30)
    assert above["best_rank"] == -1 and above["status"] == UNVERIFIED and above["safe_pick"] == 3 and above["best_inliers"] == 0
    assert np.array_equal(above["pose"], np.eye(4)) and above["reranked"].tolist() == [4, 1, 3, 0]
    assert at["best_rank"] == 2 and at["status"] == 0
    # the winner's metrics ride along
    r = pick_f64(*args, rte=[1.0, 2.0, 3.0, 4.0], rre=[0.1, 0.2, 0.3, 0.4], success=[1, 1, 0, 1])
    assert (r["best_rte"], r["best_rre"], r["best_success"]) == (3.0, 0.3, 0)
    r = pick_f64(*args, min_inliers=31, rte=[1.0] * 4, rre=[0.1] * 4, success=[1] * 4)
    assert (r["best_rte"], r["best_rre"], r["best_success"]) == (-1.0, -1.0, 0)


def test_planted_case_is_solved_by_the_restatement():
    """the condition that makes the GPU test meaningful: with the pair-id rule, at H = 1024, the true candidate of every
    query is registered (45 inliers = the 70 % planted matches of 64, success), the weak twin keeps its 13, every unrelated
    entry ends without a model, and the true candidate has at least twice the inliers of any other"""
    c, res = planted_solved()
    assert c["nn"].shape == (PLANTED_M, PLANTED_K) and PLANTED_M in c["nn"][WEAK_OF]
    for q in range(PLANTED_M):
        assert c["nn"][q, q % PLANTED_K] == q and len(set(c["nn"][q].tolist())) == PLANTED_K
        true = res[(q, q)]
        assert true["inliers"] == 45 and true["success"] == 1 and true["status"] == 0, (q, true["inliers"], true["status"])
        for m in c["nn"][q]:
            if m == q:
                continue
            r = res[(q, int(m))]
            if m == PLANTED_M:
                assert q == WEAK_OF and r["inliers"] == 13 and r["success"] == 1 and r["status"] == 0
            else:
                assert r["inliers"] == 0 and r["status"] == STATUS_NO_MODEL and r["best_t"] == -1, (q, m, r["inliers"])
            assert true["inliers"] >= 2 * r["inliers"]
        # the restated pick on the restated tables: the true entry wins from every rank, the weak twin is second
        rows = [res[(q, int(m))] for m in c["nn"][q]]
        p = pick_f64(c["nn"][q], PLANTED_M + 1, [r["T"] for r in rows], [r["inliers"] for r in rows],
                     [r["inlier_rmse"] for r in rows], [r["status"] for r in rows], planted_map_poses(PLANTED_M + 1))
        assert p["best_index"] == q and p["best_rank"] == q % PLANTED_K and p["reranked"][0] == q and p["status"] == 0
        if q == WEAK_OF:
            assert p["reranked"][1] == PLANTED_M

"""CPU tests of the NDT layer (egonn_amd/mapping.py `NDTMap`, csrc/ndt.hip): the two restatements of tests/ndt_ref.py agree bit
for bit on moments, mean and covariance; the properties the GPU tests rely on hold for them (batching, order, the residual
clamp, a hand-made voxel, planar / single-point / few-point voxels, `missed`); scan-to-map NDT moves the planted scans towards
their planted poses; the C entries are declared, exported and refuse bad arguments before any launch, and the Python surface
refuses them before it asks for a device.  Nothing here needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import ndt_ref as ref
from tests import voxel_map_ref as vref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["egonn_ndt_accumulate", "egonn_ndt_accumulate_scratch_bytes", "egonn_ndt_finalize", "egonn_ndt_register",
               "egonn_ndt_register_scratch_bytes"]
VOXEL = 0.5
ORIGIN = (0.5, -1.25, 0.125)
EYE = np.eye(4)[None]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from egonn_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def scene():
    return ref.random_scene()


def _keys(bank, off, pick, poses, origin=ORIGIN, voxel=VOXEL):
    return vref.integrate(bank, off, pick, poses, origin, voxel)["keys"]


def _one_cloud(pts, voxel=1.0, keys=None, **kw):
    """points of one cloud under the identity in a frame at 0 -> (keys, moments, Gaussians)"""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    off = np.array([0, len(pts)])
    keys = _keys(pts, off, [0], EYE, (0, 0, 0), voxel) if keys is None else keys
    acc = ref.accumulate(keys, pts, off, [0], EYE, (0, 0, 0), voxel)
    return keys, acc, ref.finalize(keys, acc["cnt"], acc["s1"], acc["s2"], voxel, **kw)


# ----------------------------------------------------------------------------- the two restatements
def test_the_two_restatements_agree(scene):
    bank, off, poses = scene
    pick = [0, 1, 2, 3, 4, 5, 6, 2]                           # an empty cloud (3) and a cloud picked twice (2)
    ps = poses[pick]
    keys = _keys(bank, off, pick, ps)
    a = ref.accumulate(keys, bank, off, pick, ps, ORIGIN, VOXEL)
    naive = ref.NaiveLayer(keys, VOXEL, ORIGIN).accumulate(bank, off, pick, ps)
    assert ref.same(a, naive.arrays()) and a["status"] == naive.status == 0 and a["missed"] == 0
    assert a["cnt"].sum() == sum(off[p + 1] - off[p] for p in pick) and (a["cnt"] >= 6).sum() > 20, "the scene must fill voxels"
    assert a["s1"].max() < 2 ** 20 * a["cnt"].max() and (a["s2"][:, [0, 3, 5]] >= 0).all()
    mean, cov = ref.mean_cov(keys, a["cnt"], a["s1"], a["s2"], VOXEL)
    rows, nmean, ncov = naive.mean_cov()
    assert len(rows) == (a["cnt"] >= 2).sum() > 50
    assert np.array_equal(mean[rows].view(np.uint64), nmean.view(np.uint64)) and np.array_equal(cov[rows].view(np.uint64), ncov.view(np.uint64))
    # the mean is the voxel map's centroid up to the ten dropped residual bits: within 2^-20 of a voxel
    rec = vref.integrate(bank, off, pick, ps, ORIGIN, VOXEL)
    cen = vref.centroids(rec, ORIGIN, VOXEL) - np.asarray(ORIGIN)
    assert np.array_equal(rec["count"], a["cnt"]) and np.abs(mean - cen).max() <= VOXEL * 2.0 ** -20 * 1.001
    # a bad pick contributes nothing and is reported by both
    c = ref.accumulate(keys, bank, off, [0, 9, 1], poses[[0, 1, 1]], ORIGIN, VOXEL)
    d = ref.NaiveLayer(keys, VOXEL, ORIGIN).accumulate(bank, off, [0, 9, 1], poses[[0, 1, 1]])
    assert ref.same(c, d.arrays()) and c["status"] == d.status == ref.BAD_INDEX
    assert ref.same(c, ref.accumulate(keys, bank, off, [0, 1], poses[[0, 1]], ORIGIN, VOXEL))
    # more points than points_capacity: CAPACITY, nothing added
    e = ref.accumulate(keys, bank, off, [0, 1], poses[[0, 1]], ORIGIN, VOXEL, points_capacity=int(off[2]) - 1)
    assert e["status"] == ref.CAPACITY and e["cnt"].sum() == 0 and e["missed"] == 0


@pytest.mark.parametrize("batches", [1, 2, 5])
def test_incremental_equals_one_shot(scene, batches):
    bank, off, poses = scene
    pick = np.array([0, 1, 2, 3, 4, 5, 6, 2, 0])
    ps = poses[pick]
    keys = _keys(bank, off, pick, ps)
    one = ref.accumulate(keys, bank, off, pick, ps, ORIGIN, VOXEL)
    for order in (np.arange(len(pick)), np.arange(len(pick))[::-1]):
        acc, naive = None, ref.NaiveLayer(keys, VOXEL, ORIGIN)
        for part in np.array_split(order, batches):
            acc = ref.accumulate(keys, bank, off, pick[part], ps[part], ORIGIN, VOXEL, out=acc)
            naive.accumulate(bank, off, pick[part], ps[part])
        assert ref.same(acc, one) and ref.same(naive.arrays(), one)


def test_residual_clamp_gives_the_largest_moment():
    """s = -1e-20 floors to -1 and s - (-1) rounds to 1.0: q is clamped to 2^30 - 1, so m = 2^20 - 1, inside the voxel"""
    pts = np.array([[-1e-20, 0.25, 0.0]])
    keys, acc, _ = _one_cloud(pts)
    assert vref.indices(keys).tolist() == [[-1, 0, 0]] and acc["cnt"].tolist() == [1]
    assert acc["s1"].tolist() == [[2 ** 20 - 1, 2 ** 18, 0]]
    assert acc["s2"].tolist() == [[(2 ** 20 - 1) ** 2, (2 ** 20 - 1) * 2 ** 18, 0, 2 ** 36, 0, 0]]
    n = ref.NaiveLayer(keys, 1.0, (0, 0, 0)).accumulate(pts, np.array([0, 1]), [0], EYE).arrays()
    assert ref.same(acc, n)


def test_a_hand_made_voxel():
    """six points of voxel (2, -1, 0) at quarters of its edge; h = 2^18 is a quarter in moment units.  In units of h the
    points are (1,2,3) (2,2,1) (3,1,2) (1,3,2) (2,1,1) (3,3,3): s1 = (12,12,12) h, s2 = (28,23,24,28,26,28) h^2,
    C = (s2 - s1 s1^T / 6) / 5 / 16 = (0.05, -0.0125, 0, 0.05, 0.025, 0.05), mean = corner + 0.5"""
    q = np.array([(1, 2, 3), (2, 2, 1), (3, 1, 2), (1, 3, 2), (2, 1, 1), (3, 3, 3)], np.float64) * 0.25
    keys, acc, G = _one_cloud(q + np.array([2.0, -1.0, 0.0]))
    h = 2 ** 18
    assert vref.indices(keys).tolist() == [[2, -1, 0]] and acc["cnt"].tolist() == [6]
    assert acc["s1"].tolist() == [[12 * h] * 3] and acc["s2"].tolist() == [[v * h * h for v in (28, 23, 24, 28, 26, 28)]]
    assert G["mean"].tolist() == [[2.5, -0.5, 0.5]]
    assert G["cov"].tolist() == [[0.05, -0.0125, 0.0, 0.05, 0.025, 0.05]]
    assert G["valid"].tolist() == [1] and G["n_valid"] == 1
    lam, vec = np.linalg.eigh(ref.full(G["cov"])[0])
    assert np.abs(G["eigenvalues"][0] - lam).max() <= 1e-12 * lam[2] and lam[0] > 0.01 * lam[2]
    assert np.abs(ref.full(G["info"])[0] @ ref.full(G["cov"])[0] - np.eye(3)).max() < 1e-12, "no eigenvalue was lifted: info = C^-1"
    n = G["normal"][0]
    assert abs(abs(n @ vec[:, 0]) - 1.0) < 1e-12 and n[np.nonzero(n)[0][0]] > 0


def test_a_planar_voxel_is_given_a_thickness():
    g = np.arange(1, 8) / 8.0
    xy = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    flat = np.concatenate([xy, np.full((len(xy), 1), 0.5)], 1)                     # the plane z = 0.5 of voxel (0, 0, 0)
    _, acc, G = _one_cloud(flat)
    l = G["eigenvalues"][0]
    assert G["valid"].tolist() == [1] and l[0] == 0.0 and l[1] > 0 and G["cov"][0, [2, 4, 5]].tolist() == [0.0, 0.0, 0.0]
    assert G["normal"][0].tolist() == [0.0, 0.0, 1.0]
    assert G["info"][0, 5] == 1.0 / (0.01 * l[2]) and G["info"][0, [2, 4]].tolist() == [0.0, 0.0], "l_0 is lifted to 0.01 l_2"
    # a tilted plane x = y: the normal is (1, -1, 0) / sqrt 2 by the sign rule (the first non-zero component is positive)
    t = np.stack([xy[:, 0], xy[:, 0], xy[:, 1]], 1)
    _, _, Gt = _one_cloud(t)
    assert Gt["valid"].tolist() == [1] and np.abs(Gt["normal"][0] - np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)).max() < 1e-9
    lt = Gt["eigenvalues"][0]
    assert abs(lt[0]) <= 1e-12 * lt[2]
    nn = Gt["normal"][0]
    assert nn @ ref.full(Gt["info"])[0] @ nn == pytest.approx(1.0 / (0.01 * lt[2]), rel=1e-9)
    # a line: two eigenvalues are lifted
    line = np.stack([g, g, g], 1)
    _, _, Gl = _one_cloud(np.concatenate([line, line[:3]]))
    ll = Gl["eigenvalues"][0]
    assert Gl["valid"].tolist() == [1] and np.abs(ll[:2]).max() <= 1e-12 * ll[2]
    assert np.linalg.eigvalsh(ref.full(Gl["info"])[0])[1] == pytest.approx(1.0 / (0.01 * ll[2]), rel=1e-9)


def test_invalid_voxels_are_zeros():
    pts = np.concatenate([np.tile([[0.25, 0.5, 0.75]], (8, 1)),                    # voxel (0,0,0): one point eight times
                          np.random.default_rng(0).uniform(0.1, 0.9, (5, 3)) + [1.0, 0.0, 0.0],         # voxel (1,0,0): 5 points
                          np.random.default_rng(1).uniform(0.1, 0.9, (6, 3)) + [2.0, 0.0, 0.0]])        # voxel (2,0,0): 6 points
    keys, acc, G = _one_cloud(pts)
    assert acc["cnt"].tolist() == [8, 5, 6] and G["valid"].tolist() == [0, 0, 1] and G["n_valid"] == 1
    for f in ("mean", "cov", "info", "eigenvalues", "normal"):
        assert not G[f][:2].any() and G[f][2].any(), f
    assert ref.mean_cov(keys, acc["cnt"], acc["s1"], acc["s2"], 1.0)[1][0].tolist() == [0.0] * 6, "a repeated point has no extent"
    G5 = ref.finalize(keys, acc["cnt"], acc["s1"], acc["s2"], 1.0, min_points=5)
    assert G5["valid"].tolist() == [0, 1, 1]
    # the eigh-based variant agrees on validity
    assert ref.finalize(keys, acc["cnt"], acc["s1"], acc["s2"], 1.0, eig="eigh")["valid"].tolist() == [0, 0, 1]


def test_missed_counts_the_points_outside_the_key_set(scene):
    bank, off, poses = scene
    keys = _keys(bank, off, [0, 1], poses[:2])
    a = ref.accumulate(keys, bank, off, [0, 1, 2, 4], poses[[0, 1, 2, 4]], ORIGIN, VOXEL)
    k2, _, ok = vref.point_keys(bank[off[2]: off[3]], poses[2], ORIGIN, VOXEL)
    k4, _, _ = vref.point_keys(bank[off[4]: off[5]], poses[4], ORIGIN, VOXEL)
    want = int((~np.isin(k2, keys)).sum() + (~np.isin(k4, keys)).sum())
    assert ok.all() and 0 < want < len(k2) + len(k4) and a["missed"] == want
    assert a["cnt"].sum() == off[2] + len(k2) + len(k4) - want
    n = ref.NaiveLayer(keys, VOXEL, ORIGIN).accumulate(bank, off, [0, 1, 2, 4], poses[[0, 1, 2, 4]])
    assert ref.same(a, n.arrays())
    # dropped points are RANGE, not missed
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0.1, 0.1, 0.1]])
    b = ref.accumulate(keys, bad, np.array([0, 3]), [0], EYE, ORIGIN, VOXEL)
    assert b["status"] == ref.RANGE and b["missed"] + b["cnt"].sum() == 1


def test_an_evaluation_is_the_sum_of_its_points():
    """the teacher-forced evaluation against a plain per-point loop, and its rules: neighbours 7 >= 1, no hit -> nothing"""
    c = ref.planted_case()
    L, src, T = c["layers"][0], c["clouds"][0][:300], c["T0"][0]
    for nb in (1, 7):
        ev = ref.evaluate(src, T, L["keys"], L["G"], 1.0, nb)
        A, b, score, n_term, n_pts = np.zeros((6, 6)), np.zeros(6), 0.0, 0, 0
        lut = {int(k): r for r, k in enumerate(L["keys"])}
        for p in src:
            vs = T[:3, :3] @ p + T[:3, 3]
            i, hit = np.floor(vs / 1.0).astype(int), False
            for o in ref.OFFSETS[:nb]:
                j = i + o
                r = lut.get(int((j[0] + vref.BIAS) << 42 | (j[1] + vref.BIAS) << 21 | (j[2] + vref.BIAS)))
                if r is None or not L["G"]["valid"][r]:
                    continue
                I, d = ref.full(L["G"]["info"][r]), vs - L["G"]["mean"][r]
                g = I @ d
                w = np.exp(-0.5 * d @ g)
                J = np.concatenate([np.array([[0, vs[2], -vs[1]], [-vs[2], 0, vs[0]], [vs[1], -vs[0], 0]]), np.eye(3)], 1)     # [-[vs]x | I]
                assert np.allclose(J.T @ g, np.concatenate([np.cross(vs, g), g]))
                A += w * J.T @ I @ J
                b += w * J.T @ g
                score, n_term, hit = score + w, n_term + 1, True
            n_pts += hit
        assert (ev["n_term"], ev["n_pts"]) == (n_term, n_pts) and n_pts > 100
        assert np.abs(ev["A"] - A).max() <= 1e-10 * np.abs(A).max() and np.abs(ev["b"] - b).max() <= 1e-10 * np.abs(A).max()
        assert ev["score"] == pytest.approx(score, rel=1e-12)
    far = ref.evaluate(src + 1e4, np.eye(4), L["keys"], L["G"], 1.0, 7)
    assert far["n_term"] == 0 and far["n_pts"] == 0 and not far["A"].any()


def test_scan_to_map_ndt_condition_holds_for_the_restatement():
    """The condition of the GPU seam test, for the restatement alone: every scan of planted_sequence(), cropped and downsampled
    as the bank does, started at its "GPS" pose against the NDT map (voxel 1.0 m, min_points 6, min_eig_ratio 0.01) of the
    other five scans at their planted poses, ends nearer to its planted pose and with a higher score.  Frobenius distances,
    start -> end, as printed here:
      neighbors = 1: 0.1254 -> 0.0047, 0.2839 -> 0.0043, 0.1737 -> 0.0030, 0.1821 -> 0.0170, 0.2313 -> 0.0046, 0.1933 -> 0.0082
      neighbors = 7: 0.1254 -> 0.0040, 0.2839 -> 0.0034, 0.1737 -> 0.0055, 0.1821 -> 0.0113, 0.2313 -> 0.0057, 0.1933 -> 0.0147
    with 202 to 207 valid Gaussians out of 312 to 317 voxels and 12 to 30 rounds (one run ends with MAX_ITER)."""
    c = ref.planted_case()
    for nb in (1, 7):
        for k in range(6):
            r, L = ref.planted_free(k, nb), c["layers"][k]
            d0, d1 = np.linalg.norm(c["T0"][k] - c["T_planted"][k]), np.linalg.norm(r["T"] - c["T_planted"][k])
            s0, s1 = r["evals"][0]["score"], r["evals"][-1]["score"]
            print(f"[ndt] neighbors {nb} scan {k}: {d0:.4f} -> {d1:.4f}, score {s0:.1f} -> {s1:.1f}, {r['iterations']} rounds, "
                  f"status {r['status']}, {L['G']['n_valid']} of {len(L['keys'])} voxels valid, fitness {r['fitness']:.3f}")
            assert d1 < d0 and s1 > s0, (nb, k)
            assert L["acc"]["missed"] == 0 and r["status"] in (0, ref.MAX_ITER)


# ----------------------------------------------------------------------------- the C ABI
def test_symbols_declared_and_exported(lib):
    from egonn_amd import _lib
    header = open(os.path.join(REPO, "include", "egonn_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert "NDT layer" in header and "Gauss-Newton" in header and "More-Thuente" in header
    src = open(os.path.join(REPO, "egonn_amd", "csrc", "ndt.hip")).read()
    assert "#pragma clang fp contract(off)" in src and '#include "voxel_key.h"' in src
    assert not re.search(r"atomicAdd\s*\(\s*\(?\s*(float|double)|unsafeAtomicAdd|atomicAdd_system", src), "integer atomics only"
    # the shared arithmetic is stated once
    csrc = os.path.join(REPO, "egonn_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc))}
    for fn, home in (("nrm_jacobi3", "jacobi3.h"), ("icp_plane_solve", "plane_step.h"), ("vm_point_key", "voxel_key.h")):
        defs = [f for f in text if re.search(r"\b(void|bool)\s+" + fn + r"\s*\(", text[f])]
        assert defs == [home], (fn, defs)
    # the loop around it as well (pair_loop.h): every piece is defined there and nowhere else, and the copies it replaced are gone
    loop = ("pair_apply", "pair_begin", "pair_of", "pair_chunk", "pair_reduce", "pair_gather", "pair_stop", "pair_advance",
            "pair_layout", "pair_clear_traces")
    for fn, home in [(fn, "pair_loop.h") for fn in loop] + [("se3_load", "pose_math.h"), ("se3_store", "pose_math.h")]:
        defs = [f for f in text if re.search(r"\b(void|bool|int|PairLayout)\s+" + fn + r"\s*\([^;{]*\)\s*\{", text[f])]
        assert defs == [home], (fn, defs)
    for fn in loop:
        users = ("ndt.hip",) if fn == "pair_chunk" else ("icp.hip", "ndt.hip")      # icp.hip's hot kernels spell the early-out out
        assert all(re.search(r"\b" + fn + r"(<[^>]*>)?\(", text[f]) for f in users), fn
    for old in ("icp_pair_of", "ndt_pair_of", "ndt_write_T"):
        assert not [f for f in text if re.search(r"\b" + old + r"\b", text[f])], old
    for f in ("icp.hip", "ndt.hip"):
        assert '#include "pair_loop.h"' in text[f] and '"pose_math.h"' not in text[f], f
        assert not re.search(r"__shfl_xor\(v\[|\bm3_\w+\(|\bse3_(mul|inv_mul|mul_inv)\(", text[f]), f
    assert "#pragma clang fp contract(off)" in text["pair_loop.h"]


def _refused(lib, rc, needle):
    assert rc == 1, rc                              # EGONN_STATUS_INVALID: returned before any device work
    assert needle in lib.egonn_last_error().decode(), lib.egonn_last_error()


def _broken(args, at, value):
    out = list(args)
    out[at] = value
    return out


def test_c_entries_refuse_bad_arguments_before_any_launch(lib):
    """one valid-looking argument list per entry point, broken in one place per case: every refusal is decided on the host from
    the scalar arguments, the pointers are never dereferenced, and no GPU is present when this runs"""
    p, s = C.c_void_p(256), C.c_void_p(4096)
    d3 = lambda *v: (C.c_double * 3)(*v)             # noqa: E731
    org, nan, inf = d3(0.0, 0.0, 0.0), float("nan"), float("inf")
    # accumulate: bank n_bank off n_clouds pick poses n_obs origin voxel points_capacity keys n_dev capacity_map cnt s1 s2 missed status scratch bytes stream
    need = lib.egonn_ndt_accumulate_scratch_bytes(1000, 4)
    assert need > 0 and need % 256 == 0
    ok = [p, 1000, p, 4, p, p, 4, org, 1.0, 1000, p, p, 500, p, p, p, p, p, s, need, None]
    f = lib.egonn_ndt_accumulate
    for at, value, needle in ((6, 0, "n_obs"), (6, 4097, "n_obs"), (1, -1, "bad shape"), (3, -1, "bad shape"), (9, -1, "points_capacity"),
                              (9, 1 << 31, "points_capacity"), (12, -1, "capacity_map"), (12, 1 << 31, "capacity_map"),
                              (8, 0.0, "voxel"), (8, -1.0, "voxel"), (8, nan, "voxel"), (8, inf, "voxel"),
                              (7, d3(0.0, nan, 0.0), "origin"), (7, d3(inf, 0.0, 0.0), "origin"), (7, None, "origin"),
                              (0, None, "null"), (2, None, "null"), (4, None, "null"), (5, None, "null"), (10, None, "null"),
                              (11, None, "null"), (13, None, "null"), (14, None, "null"), (15, None, "null"), (16, None, "null"),
                              (17, None, "null"), (18, None, "null"), (18, C.c_void_p(4096 + 8), "256-byte aligned"),
                              (19, need - 1, "scratch needs")):
        _refused(lib, f(*_broken(ok, at, value)), needle)
    g = lib.egonn_ndt_accumulate_scratch_bytes
    assert g(-1, 4) == -1 and g(1 << 31, 4) == -1 and g(10, 0) == -1 and g(10, 4097) == -1 and g(0, 1) > 0
    # finalize: keys n_dev capacity_map cnt s1 s2 voxel min_points min_eig_ratio mean info eigenvalues normal valid n_valid cov stream
    ok = [p, p, 500, p, p, p, 1.0, 6, 0.01, p, p, p, p, p, p, None, None]
    f = lib.egonn_ndt_finalize
    for at, value, needle in ((2, -1, "capacity_map"), (2, 1 << 31, "capacity_map"), (6, 0.0, "voxel"), (6, nan, "voxel"),
                              (6, inf, "voxel"), (6, -2.0, "voxel"), (7, 2, "min_points"), (7, -1, "min_points"),
                              (8, 0.0, "min_eig_ratio"), (8, -0.1, "min_eig_ratio"), (8, nan, "min_eig_ratio"), (8, inf, "min_eig_ratio"),
                              (0, None, "null"), (1, None, "null"), (3, None, "null"), (4, None, "null"), (5, None, "null"),
                              (9, None, "null"), (10, None, "null"), (11, None, "null"), (12, None, "null"), (13, None, "null"),
                              (14, None, "null")):
        _refused(lib, f(*_broken(ok, at, value)), needle)
    # register: src n_src off n_pairs T_init keys n_dev capacity_map mean info valid voxel neighbors max_iteration eps_rot eps_trans
    #           T fitness score iterations status T_trace eval_trace sums_trace scratch bytes stream
    need = lib.egonn_ndt_register_scratch_bytes(1000, 3)
    assert need > 0 and need % 256 == 0
    ok = [p, 1000, p, 3, p, p, p, 500, p, p, p, 1.0, 7, 30, 1e-5, 1e-4, p, p, p, p, p, None, None, None, s, need, None]
    f = lib.egonn_ndt_register
    for at, value, needle in ((1, -1, "n_src"), (1, 1 << 31, "n_src"), (3, 0, "n_pairs"), (3, 4097, "n_pairs"), (7, -1, "capacity_map"),
                              (7, 1 << 31, "capacity_map"), (11, 0.0, "voxel"), (11, nan, "voxel"), (11, inf, "voxel"),
                              (12, 0, "neighbors"), (12, 6, "neighbors"), (12, 27, "neighbors"), (13, -1, "max_iteration"),
                              (14, 0.0, "eps_rot"), (14, nan, "eps_rot"), (14, inf, "eps_rot"), (15, -1e-4, "eps_trans"),
                              (15, nan, "eps_trans"), (0, None, "null"), (2, None, "null"), (5, None, "null"), (6, None, "null"),
                              (8, None, "null"), (9, None, "null"), (10, None, "null"), (16, None, "null"), (17, None, "null"),
                              (18, None, "null"), (19, None, "null"), (20, None, "null"), (24, None, "null"),
                              (24, C.c_void_p(4096 + 128), "256-byte aligned"), (25, need - 1, "scratch needs")):
        _refused(lib, f(*_broken(ok, at, value)), needle)
    g = lib.egonn_ndt_register_scratch_bytes
    assert g(-1, 3) == -1 and g(1 << 31, 3) == -1 and g(10, 0) == -1 and g(10, 4097) == -1 and g(0, 1) > 0


# ----------------------------------------------------------------------------- the Python surface
class _Bank:
    def __init__(self, sizes):
        self._sizes = np.asarray(sizes, np.int64)

    def __len__(self):
        return len(self._sizes)

    def sizes(self):
        return self._sizes


def test_python_refuses_bad_arguments_before_asking_for_a_device(lib):
    import egonn_amd
    from egonn_amd import mapping as M
    from egonn_amd.relocalize import Relocalizer
    assert egonn_amd.NDTMap is M.NDTMap and egonn_amd.build_ndt_map is M.build_ndt_map
    assert (M.NDT_MIN_POINTS, M.NDT_MIN_EIG_RATIO, M.NDT_MAX_ITERATION, M.NDT_EPS_ROT, M.NDT_EPS_TRANS) == (6, 0.01, 30, 1e-5, 1e-4)
    vm = M.VoxelMap()
    for bad in (2, 0, -1):
        with pytest.raises(ValueError, match="min_points"):
            M.NDTMap(vm, min_points=bad)
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="min_eig_ratio"):
            M.NDTMap(vm, min_eig_ratio=bad)
    with pytest.raises(ValueError, match="chunk_points"):
        M.NDTMap(vm, chunk_points=0)
    with pytest.raises(ValueError, match="empty"):
        M.NDTMap(vm)
    with pytest.raises(ValueError, match="empty"):
        M.NDTMap(None)
    with pytest.raises(ValueError, match="min_points"):
        M.build_ndt_map(_Bank([3]), np.eye(4)[None], min_points=1)
    bank, eye = _Bank([5, 0, 7]), np.tile(np.eye(4), (3, 1, 1))
    with pytest.raises(ValueError, match="method"):
        M.refine_against_map(vm, bank, [0, 1], eye[:2], method="gicp")
    with pytest.raises(ValueError, match="needs ndt"):
        M.refine_against_map(vm, bank, [0, 1], eye[:2], method="ndt")
    with pytest.raises(ValueError, match=r"\(2, 4, 4\)"):
        M.refine_against_map(vm, bank, [0, 1], eye, method="ndt", ndt=None)
    with pytest.raises(ValueError, match="ndt_neighbors"):
        Relocalizer(None, None, ndt_neighbors=3)
    with pytest.raises(ValueError, match="finalized NDTMap"):
        Relocalizer(None, None, ndt_map=object())
    assert vm.n_voxels == 0 and vm.status == 0 and vm.origin is None, "nothing above asked for a device or changed the map"


def test_load_refuses_other_files(tmp_path):
    from egonn_amd import NDTMap
    path = str(tmp_path / "junk.npz")
    np.savez(path, keys=np.zeros(3, np.int64), cnt=np.zeros(3, np.int32))
    with pytest.raises(ValueError, match="not an NDT map"):
        NDTMap.load(path)

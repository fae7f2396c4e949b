"""CPU tests: the oracle (oracle/me_ops.py + oracle/egonn_ref.py) against
  (1) hand-derivable known-answer cases for the sparse primitives (the reference has no tests
      and MinkowskiEngine is absent, so these are the only pins for the primitive semantics),
  (2) torch CPU for the quantiser arithmetic (torch is the reference's own arithmetic backend),
  (3) the golden vectors produced by the reference's own graph code (tests/golden/)."""
import numpy as np
import pytest
import torch

from oracle import egonn_ref as ref
from oracle import me_ops as ops
from tests import helpers as H


# ------------------------------------------------------------------ (1) known-answer primitives
def test_kernel_offsets_order_and_even_kernel():
    o3 = ops.kernel_offsets(3, 1)
    assert o3.shape == (27, 3)
    assert tuple(o3[0]) == (-1, -1, -1) and tuple(o3[1]) == (0, -1, -1) and tuple(o3[3]) == (-1, 0, -1)
    assert tuple(o3[13]) == (0, 0, 0) and tuple(o3[26]) == (1, 1, 1)
    o2 = ops.kernel_offsets(2, 4)          # even kernel: non-centred, multiples of the input stride
    assert o2.min() == 0 and o2.max() == 4
    assert tuple(o2[1]) == (4, 0, 0) and tuple(o2[2]) == (0, 4, 0) and tuple(o2[4]) == (0, 0, 4)


def test_conv3_three_voxel_line_known_answer():
    # voxels at x=0,1,2 ; feature = [1],[10],[100] ; kernel[i] = i (1x1 channel)
    c = np.array([[0, 0, 0, 0], [0, 1, 0, 0], [0, 2, 0, 0]], dtype=np.int32)
    f = np.array([[1.0], [10.0], [100.0]], dtype=np.float32)
    k = np.arange(27, dtype=np.float32).reshape(27, 1, 1)
    out = ops.conv_forward(f, k, ops.kernel_map(c, c, 3, 1), 3)
    # offsets along x only: index 12 = (-1,0,0), 13 = centre, 14 = (+1,0,0)
    assert np.allclose(out[:, 0], [1 * 13 + 10 * 14, 1 * 12 + 10 * 13 + 100 * 14, 10 * 12 + 100 * 13])


def test_strided_conv_and_transpose_known_answer():
    # negative coordinates use true floor: -1 -> parent -2 (slot 1), 0 and 1 -> parent 0
    c = np.array([[0, -1, 0, 0], [0, 0, 0, 0], [0, 1, 0, 0], [0, 1, 1, 1]], dtype=np.int32)
    parents = ops.stride_coords(c, 2)
    assert H.sort_rows(parents).tolist() == [[0, -2, 0, 0], [0, 0, 0, 0]]
    f = np.array([[1.0], [2.0], [4.0], [8.0]], dtype=np.float32)
    k = (10.0 ** np.arange(8)).astype(np.float32).reshape(8, 1, 1) / 1000.0   # slot i -> 10^(i-3)
    maps = ops.kernel_map(c, parents, 2, 1)
    out = ops.conv_forward(f, k, maps, len(parents))
    by = {tuple(p): o for p, o in zip(parents.tolist(), out[:, 0].tolist())}
    assert np.isclose(by[(0, -2, 0, 0)], 1.0 * k[1, 0, 0])                      # (-1,0,0) = parent+(1,0,0)
    assert np.isclose(by[(0, 0, 0, 0)], 2.0 * k[0, 0, 0] + 4.0 * k[1, 0, 0] + 8.0 * k[7, 0, 0])
    # transposed conv: every fine voxel receives parent feature * kernel[slot]
    g = np.array([[3.0], [5.0]], dtype=np.float32)          # features on `parents` rows
    up = ops.conv_transpose_forward(g, k, maps, len(c))
    pf = {tuple(p): v for p, v in zip(parents.tolist(), g[:, 0].tolist())}
    assert np.isclose(up[0, 0], pf[(0, -2, 0, 0)] * k[1, 0, 0])
    assert np.isclose(up[1, 0], pf[(0, 0, 0, 0)] * k[0, 0, 0])
    assert np.isclose(up[3, 0], pf[(0, 0, 0, 0)] * k[7, 0, 0])


def _dense_case(seed, box=10, n=260, cin=3, b=2, lo=-5):
    """random sparse set in a box (negative coordinates included), its features, and the same data as a dense volume
    [b, cin, X, Y, Z] whose index 0 is coordinate `lo`"""
    rng = np.random.default_rng(seed)
    c = np.unique(np.c_[rng.integers(0, b, n), rng.integers(lo, lo + box, (n, 3))], axis=0).astype(np.int32)
    f = rng.standard_normal((len(c), cin)).astype(np.float32)
    vol = np.zeros((b, cin, box, box, box), np.float32)
    vol[c[:, 0], :, c[:, 1] - lo, c[:, 2] - lo, c[:, 3] - lo] = f
    return c, f, vol, lo


@pytest.mark.parametrize("k", [3, 5])
def test_conv_matches_dense_conv3d(k):
    """Independent cross-check of oracle/me_ops.conv_forward + kernel_map: the same convolution computed
    by torch.nn.functional.conv3d on the densified volume.  conv3d is a cross-correlation, out[x] = sum_d in[x + d] w[d],
    which is the form A.5 states for ME; with the volume laid out [X, Y, Z] the dense weight is w[co][ci][kx][ky][kz] =
    kernel[kx + k*ky + k*k*kz][ci][co] (first spatial axis fastest).  A transposed / flipped / y-fastest restatement fails
    this test; it does not pin MinkowskiEngine itself (absent), only that the restatement is the convolution it claims."""
    import torch.nn.functional as F
    c, f, vol, lo = _dense_case(100 + k)
    cin, cout = f.shape[1], 4
    rng = np.random.default_rng(7)
    kern = rng.standard_normal((k ** 3, cin, cout)).astype(np.float32)
    out = ops.conv_forward(f, kern, ops.kernel_map(c, c, k, 1), len(c))
    w = torch.from_numpy(kern).reshape(k, k, k, cin, cout).permute(4, 3, 2, 1, 0).contiguous()    # [kz][ky][kx] -> [co][ci][kx][ky][kz]
    dense = F.conv3d(torch.from_numpy(vol).double(), w.double(), padding=k // 2).numpy()
    want = dense[c[:, 0], :, c[:, 1] - lo, c[:, 2] - lo, c[:, 3] - lo]
    np.testing.assert_allclose(out, want, rtol=1e-4, atol=1e-4)
    # an asymmetric kernel makes the check sensitive to the axis order: the y-fastest reading must NOT match
    w_bad = torch.from_numpy(kern).reshape(k, k, k, cin, cout).permute(4, 3, 1, 2, 0).contiguous()
    bad = F.conv3d(torch.from_numpy(vol).double(), w_bad.double(), padding=k // 2).numpy()
    assert np.abs(bad[c[:, 0], :, c[:, 1] - lo, c[:, 2] - lo, c[:, 3] - lo] - out).max() > 0.1


def test_strided_and_transposed_conv_match_dense():
    """k=2,s=2 (non-centred even kernel, floor parents — also for negative coordinates) against conv3d(stride=2) on the volume
    aligned to even coordinates, and the transposed convolution onto the cached fine map against conv_transpose3d(stride=2)
    read back at the fine voxels (A.5 / A.6)."""
    import torch.nn.functional as F
    c, f, vol, lo = _dense_case(31, box=10, lo=-6)         # lo even: dense index 2X' <-> coordinate lo + 2X'
    cin, cout = f.shape[1], 5
    rng = np.random.default_rng(9)
    kern = rng.standard_normal((8, cin, cout)).astype(np.float32)
    parents = ops.stride_coords(c, 2)
    maps = ops.kernel_map(c, parents, 2, 1)
    out = ops.conv_forward(f, kern, maps, len(parents))
    w = torch.from_numpy(kern).reshape(2, 2, 2, cin, cout).permute(4, 3, 2, 1, 0).contiguous()
    dense = F.conv3d(torch.from_numpy(vol).double(), w.double(), stride=2).numpy()
    pi = (parents[:, 1:] - lo) // 2
    np.testing.assert_allclose(out, dense[parents[:, 0], :, pi[:, 0], pi[:, 1], pi[:, 2]], rtol=1e-4, atol=1e-4)
    # transposed: features on the parents, kernel (8, cout, cin2)
    g = rng.standard_normal((len(parents), cout)).astype(np.float32)
    kt = rng.standard_normal((8, cout, 2)).astype(np.float32)
    up = ops.conv_transpose_forward(g, kt, maps, len(c))
    pv = np.zeros((vol.shape[0], cout, 5, 5, 5), np.float32)
    pv[parents[:, 0], :, pi[:, 0], pi[:, 1], pi[:, 2]] = g
    wt = torch.from_numpy(kt).reshape(2, 2, 2, cout, 2).permute(3, 4, 2, 1, 0).contiguous()       # conv_transpose3d: [in][out][kx][ky][kz]
    dense_up = F.conv_transpose3d(torch.from_numpy(pv).double(), wt.double(), stride=2).numpy()
    np.testing.assert_allclose(up, dense_up[c[:, 0], :, c[:, 1] - lo, c[:, 2] - lo, c[:, 3] - lo], rtol=1e-4, atol=1e-4)


def test_sparse_quantize_first_occurrence_and_negative_floor():
    pc = np.array([[0.05, 0.0, 0.0], [-0.05, 0.0, 0.0], [0.06, 0.01, 0.0], [0.31, 0.0, -0.11]], np.float32)
    d, idx = ops.sparse_quantize(pc, 0.1)
    assert d.tolist() == [[0, 0, 0], [-1, 0, 0], [3, 0, -2]]
    assert idx.tolist() == [0, 1, 3]


# ------------------------------------------------------------------ (2) quantiser arithmetic vs torch
def test_cartesian_division_is_true_fp32_division():
    rng = np.random.default_rng(0)
    pc = (rng.uniform(-80, 80, size=(200000, 3))).astype(np.float32)
    for q in (0.1, 0.3, 0.01):
        want = torch.floor(torch.from_numpy(pc) / q).int().numpy()
        got = np.floor(pc / np.float32(q)).astype(np.int32)
        assert np.array_equal(want, got)


def test_polar_conversion_matches_torch():
    rng = np.random.default_rng(1)
    pc = rng.uniform(-80, 80, size=(100000, 3)).astype(np.float32)
    t = torch.from_numpy(pc)
    theta = 180. + torch.atan2(t[:, 1], t[:, 0]) * 180. / np.pi      # reference quantization.py:35
    dist = torch.sqrt(t[:, 0] ** 2 + t[:, 1] ** 2)
    want = (torch.stack([theta, dist, t[:, 2]], dim=1) / torch.tensor([1., 0.3, 0.2])).numpy()
    got = ref.PolarQuantizer([1., 0.3, 0.2]).to_polar(pc)
    # libm differences between torch and numpy are allowed only as <= 1 ulp noise, and must not
    # move any point across a bin edge in this sample
    assert np.allclose(want, got, rtol=3e-7, atol=3.1e-5)   # 2 ulp at theta ~ 256
    frac_moved = (np.floor(want) != np.floor(got)).any(axis=1).mean()
    assert frac_moved < 1e-4


# ------------------------------------------------------------------ (3) golden vectors
@pytest.mark.parametrize("name", H.CASES)
def test_quantizer_matches_reference(name):
    case = H.load_case(name)
    q = H.make_quantizer(case, ref)
    for b in range(int(case["n_scans"])):
        coords, idx = q(case[f"points_{b}"])
        if str(case["coordinates"]) == "cartesian":
            assert np.array_equal(coords, case[f"quant_coords_{b}"])
            assert np.array_equal(idx, case[f"quant_index_{b}"])
        else:   # transcendental: sets may differ by bin-edge points only
            a = set(map(tuple, coords.tolist()))
            g = set(map(tuple, case[f"quant_coords_{b}"].tolist()))
            assert len(a ^ g) <= max(2, len(g) // 1000)


@pytest.mark.parametrize("name", H.CASES)
def test_forward_matches_reference_graph(name):
    case = H.load_case(name)
    oracle = ref.EgoNNOracle(H.seeded_weights(case["weight_seed"]), H.make_quantizer(case, ref))
    c4 = case["coords"]
    y = oracle.forward(c4, np.ones((len(c4), 1), np.float32), return_internals=True)
    lv = y["_levels"]
    for lvl in range(3, 8):
        assert np.array_equal(H.sort_rows(lv.coords[lvl]), case[f"level{lvl}_coords"])
    for lvl in (3, 7):
        perm = H.join_perm(lv.coords[lvl], case[f"level{lvl}_coords"])
        np.testing.assert_allclose(y["_trunk"][lvl][perm], case[f"level{lvl}_feats"], rtol=2e-4, atol=2e-5)
    assert H.cosine_err(y["global"], case["global"]).max() < 1e-6
    np.testing.assert_allclose(y["global"], case["global"], rtol=1e-4, atol=1e-5)
    for b in range(int(case["n_scans"])):
        perm = H.join_perm(y["keypoint_coords"][b], case[f"kp_coords_{b}"])
        np.testing.assert_allclose(y["keypoints"][b][perm], case[f"keypoints_{b}"], rtol=1e-5, atol=2e-4)
        np.testing.assert_allclose(y["sigma"][b][perm], case[f"sigma_{b}"], rtol=1e-4, atol=1e-5)
        assert H.cosine_err(y["descriptors"][b][perm], case[f"descriptors_{b}"]).max() < 1e-6
        # selection: same ordered list of super-voxel coordinates as torch.topk on the reference sigma
        idx = ref.select_keypoints(case[f"sigma_{b}"], case[f"kp_coords_{b}"], 128)
        sel_sigma = case[f"sigma_{b}"].reshape(-1)[idx]
        assert np.array_equal(sel_sigma, case[f"topk_sigma_{b}"])
        if len(np.unique(sel_sigma)) == len(sel_sigma):      # no ties -> order is fully determined
            assert np.array_equal(case[f"kp_coords_{b}"][idx], case[f"topk_coords_{b}"])


@pytest.mark.parametrize("name", H.MINKLOC_CASES)
def test_minkloc_oracle_matches_reference_graph(name):
    """MinkFPN + GeM (models/minkfpn.py, models/minkloc.py, third_party/minkloc3d/minkloc.py)."""
    case = H.load_case(name)
    oracle = ref.MinkLocOracle(H.seeded_weights(case["weight_seed"], name))
    c4 = case["coords"]
    y = oracle.forward(c4, np.ones((len(c4), 1), np.float32))
    assert H.cosine_err(y["global"], case["global"]).max() < 1e-6
    np.testing.assert_allclose(y["global"], case["global"], rtol=1e-4, atol=1e-5)
    perm = H.join_perm(y["_coords"], case["backbone_coords"])
    np.testing.assert_allclose(y["_feats"][perm], case["backbone_feats"].astype(np.float32), rtol=2e-3, atol=2e-3)


def test_triplet_miner_matches_reference_formulas():
    """The in-tree miner of models/loss.py:114-143 is plain torch (its file cannot be imported because of the
    pytorch_metric_learning import at the top), so its formulas are evaluated with torch here and compared with
    the oracle's index choice."""
    rng = np.random.default_rng(0)
    n = 40
    e = rng.standard_normal((n, 16)).astype(np.float32)
    lab = rng.integers(0, 6, n)
    pm = (lab[:, None] == lab[None, :]) & ~np.eye(n, dtype=bool)
    nm = (np.abs(lab[:, None] - lab[None, :]) >= 2)
    pm[3] = False                                              # anchor without positives is dropped
    D = torch.cdist(torch.from_numpy(e), torch.from_numpy(e), p=2)
    tp, tn = torch.from_numpy(pm), torch.from_numpy(nm)
    mm = D.clone(); mm[~tp] = 0
    (hpd, hpi) = torch.max(mm, dim=1)
    mm = D.clone(); mm[~tn] = float('inf')
    (hnd, hni) = torch.min(mm, dim=1)
    keep = torch.any(tp, dim=1) & torch.any(tn, dim=1)
    loss, stats, (a, p, q) = ref.batch_hard_triplet_loss(e, pm, nm, 0.2)
    assert np.array_equal(a, torch.where(keep)[0].numpy())
    assert np.array_equal(p, hpi[keep].numpy()) and np.array_equal(q, hni[keep].numpy())
    assert abs(stats["max_pos_pair_dist"] - hpd.max().item()) < 1e-5
    assert abs(stats["mean_neg_pair_dist"] - hnd.mean().item()) < 1e-5
    # swap + AvgNonZero (Appendix A.9), evaluated with torch
    d_ap, d_an, d_pn = D[a, p], D[a, q], D[p, q]
    li = torch.relu(d_ap - torch.minimum(d_an, d_pn) + 0.2)
    want = li[li > 0].mean().item() if (li > 0).any() else 0.0
    assert abs(loss - want) < 1e-5


def test_retrieval_oracle_known_answer():
    from oracle import retrieval_ref as R
    m = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 2.0], [1.0, 0.0]], dtype=np.float32)      # rows 1 and 3 tie
    q = np.array([[0.9, 0.0], [0.0, 1.9]], dtype=np.float32)
    idx, dist = R.knn(q, m, 3)
    assert idx.tolist() == [[1, 3, 0], [2, 0, 1]]
    assert np.allclose(dist[0], [0.1, 0.1, 0.9], atol=1e-6)
    mpos = np.array([[0, 0], [10, 0], [0, 10], [50, 50]], dtype=np.float32)
    qpos = np.array([[48, 50], [0, 9]], dtype=np.float32)
    rec = R.recall(idx, qpos, mpos, [5, 20], 3)
    assert rec[5] == [0.5, 1.0, 1.0] and rec[20] == [0.5, 1.0, 1.0]
    idx2, _ = R.knn(q, m[:2], 3)                                   # k larger than the database
    assert idx2.tolist() == [[1, 0, -1], [0, 1, -1]]


def test_ingest_oracle_known_answer():
    from oracle import ingest_ref as I
    raw = np.array([[0, 0, 0, 5], [1, 2, -0.9, 1], [1, 2, -0.8999, 1], [0, 0, 1e-9, 0], [3, 4, np.nan, 0], [5, 6, 7, 8]],
                   dtype=np.float32)
    pc = I.preprocess(I.read_pc(raw), "mulran")
    assert pc.tolist() == [[1.0, 2.0, np.float32(-0.8999)], [5.0, 6.0, 7.0]]


def test_c_openmp_oracle_matches_numpy_oracle_and_fixture():
    """oracle/egonn_cpu.c (the CPU baseline bench.py times) vs the numpy oracle and the reference-graph fixture."""
    from oracle import egonn_cpu, egonn_ref as ref
    case = H.load_case("egonn_cart01_b1")
    w = H.seeded_weights(int(case["weight_seed"]))
    pc = case["points_0"]
    co = egonn_cpu.CpuOracle(w, 0.1)
    g, kp, desc, coords, sigma, counts = co.compute_embedding(pc, 128)
    # fixture produced by the reference's own graph code
    assert H.cosine_err(g, case["global"]).max() <= 1e-4
    assert counts[0] == len(case["quant_coords_0"]) and counts[3] == len(case["kp_coords_0"])
    assert np.array_equal(coords, case["topk_coords_0"][:, 1:])                 # the 128 selected super-voxels, in order
    assert np.allclose(sigma, case["topk_sigma_0"], rtol=1e-3, atol=1e-6)
    # numpy oracle: same selection, same keypoints / descriptors
    orc = ref.EgoNNOracle(w, ref.CartesianQuantizer(0.1))
    g2, kp2, desc2, c2 = ref.compute_embedding(orc, pc, 128)
    assert np.array_equal(coords, c2[:, 1:])
    assert np.allclose(kp, kp2, atol=2e-4) and H.cosine_err(desc, desc2).max() <= 1e-5
    assert H.cosine_err(g, g2).max() <= 1e-6


def test_c_oracle_polar_matches_reference_fixture():
    """oracle/egonn_cpu.c with the polar quantiser (the reference's shipped configuration, models/egonn.txt:3-5) against the
    fixture produced by the reference's own graph code, and against the numpy restatement."""
    from oracle import egonn_cpu, egonn_ref as ref
    case = H.load_case("egonn_polar_b1")
    w = H.seeded_weights(int(case["weight_seed"]))
    pc = case["points_0"]
    step = [float(v) for v in case["quantization_step"]]
    g, kp, de, sc, sg, cnt = egonn_cpu.CpuOracle(w, step).compute_embedding(pc, 128)
    assert H.cosine_err(g, case["global"]).max() < 1e-6
    assert cnt[0] == len(case["quant_coords_0"])
    want = {tuple(c): i for i, c in enumerate(case["topk_coords_0"][:, 1:].tolist())}
    gap = np.r_[True, np.diff(case["topk_sigma_0"]) > 1e-5] & np.r_[np.diff(case["topk_sigma_0"]) > 1e-5, True]
    same = np.array([want.get(tuple(c), -1) == i for i, c in enumerate(sc.tolist())])
    assert (same | ~gap).all()
    g2, kp2, de2, kc2, sg2 = ref.compute_embedding_with_sigma(ref.EgoNNOracle(w, ref.PolarQuantizer(step)), pc, 128)
    assert np.array_equal(sc, kc2[:, 1:]) and np.allclose(kp, kp2, atol=1e-4) and np.allclose(sg, sg2, rtol=1e-4, atol=1e-6)
    assert H.cosine_err(de, de2).max() < 1e-6


def test_c_oracle_under_sanitizers(tmp_path):
    """SURVEY.md §5 / VERDICT r2 6-iv: oracle/egonn_cpu.c built with -fsanitize=address,undefined (plain gcc on its one source
    file + the stand-alone driver oracle/egonn_cpu_san_main.c) and run over ragged / tiny / empty / polar inputs: no
    sanitizer report, and the level counts / output sums equal the regular build's."""
    import os, shutil, struct, subprocess
    from oracle import egonn_cpu
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    here = os.path.dirname(egonn_cpu.SRC)
    exe = str(tmp_path / "egonn_cpu_san")
    cmd = ["gcc", "-O1", "-g", "-fopenmp", "-std=c11", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-mavx2", "-mfma",
           "-o", exe, egonn_cpu.SRC, os.path.join(here, "egonn_cpu_san_main.c"), "-lm"]
    subprocess.run(cmd, check=True)
    w = H.seeded_weights(5)
    keys = egonn_cpu.weight_order()
    from egonn_amd.synth import lidar_scan
    rng = np.random.default_rng(3)
    cases = [("lidar4k", lidar_scan(11, 4000), [0.1]), ("lidar_polar", lidar_scan(12, 3000), [1.0, 0.3, 0.2]),
             ("one_point", np.array([[1.0, 2.0, 0.5]], np.float32), [0.1]),
             ("two_far", np.array([[0.0, 0.0, 0.0], [70.0, -60.0, 3.0]], np.float32), [0.1]),
             ("dup_points", np.repeat(rng.standard_normal((5, 3)).astype(np.float32), 40, axis=0), [0.1]),
             ("negatives", (rng.standard_normal((800, 3)) * 3 - 5).astype(np.float32), [0.3])]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               OMP_NUM_THREADS="2")
    for name, pc, step in cases:
        f = tmp_path / (name + ".bin")
        st = (step * 3)[:3]
        with open(f, "wb") as fh:
            fh.write(struct.pack("<qi3fii", len(pc), 1 if len(step) == 3 else 0, *st, 64, len(keys)))
            for k in keys:
                a = np.ascontiguousarray(w[k], dtype=np.float32).reshape(-1)
                fh.write(struct.pack("<q", a.size)); fh.write(a.tobytes())
            fh.write(np.ascontiguousarray(pc, np.float32).tobytes())
        r = subprocess.run([exe, str(f)], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (name, r.stderr[-2000:])
        g, kp, de, sc, sg, cnt = egonn_cpu.CpuOracle(w, step if len(step) == 3 else step[0]).compute_embedding(pc, 64, 2)
        tok = r.stdout.split()
        assert int(tok[1]) == len(kp) and [int(t) for t in tok[3:11]] == cnt.tolist(), (name, r.stdout)
        assert np.isclose(float(tok[12]), float(g.astype(np.float64).sum()), rtol=1e-4, atol=1e-4), (name, r.stdout)


# ------------------------------------------------------------------ (4) the reference map on the edge geometries
# tests/test_gpu_maps.py holds the HIP plan against oracle.me_ops.kernel_map on the geometries of tests/helpers.py; the counts
# below are derivable by hand and pin the oracle itself there.  A solid block of m cells per axis has (3m - 2)^3 k=3 entries:
# per axis, m centre pairs + (m - 1) pairs each way.
def _levels(scan_list):
    c4, _ = H.batch_of(scan_list)
    return ref.SparseLevels(c4)


def _n_pairs(lv, level):
    return sum(len(j) for j, _ in lv.kmap(level, level, 3))


def test_oracle_key_range_covers_coord_bits_16_and_one_step_beyond():
    lo, hi = -(1 << 15), (1 << 15) - 1
    c = np.array([[0, lo, lo, lo], [0, hi, hi, hi], [511, lo, hi, 0]], dtype=np.int64)
    k = ops.encode_rows(c)
    assert (np.diff(k) > 0).all() and k.dtype == np.int64
    # one k=5 step of level 7 beyond either end still encodes, without meeting another voxel's key
    far = np.array([[0, lo - 256, lo - 256, lo - 256], [0, hi + 256, hi + 256, hi + 256]], dtype=np.int64)
    assert len(np.unique(np.concatenate([k, ops.encode_rows(far)]))) == 5
    for c4 in (np.array([[0, 1 << 17, 0, 0]]), np.array([[0, 0, -(1 << 17) - 1, 0]]), np.array([[512, 0, 0, 0]])):
        with pytest.raises(AssertionError):
            ops.encode_rows(c4)


@pytest.mark.parametrize("n", [1, 2, 5, 20])
def test_solid_cube_pair_count(n):
    lv = _levels([H.solid_cube(n)])
    assert lv.n(0) == n ** 3
    assert _n_pairs(lv, 0) == (3 * n - 2) ** 3
    if n == 20:
        assert _n_pairs(lv, 0) == 195112
        # interior rows carry all 27 offsets
        per_row = np.zeros(lv.n(0), dtype=np.int64)
        for _, o in lv.kmap(0, 0, 3):
            per_row[o] += 1
        assert (per_row == 27).sum() == 18 ** 3
    # an origin on the block boundaries gives the same count: the map does not see alignment
    assert _n_pairs(_levels([H.solid_cube(n, origin=(-64, 0, 60))]), 0) == (3 * n - 2) ** 3


def test_checkerboard_pair_counts():
    lv = _levels([H.checkerboard(16)])
    assert lv.n(0) == 4096 and lv.n(1) == 4096
    assert _n_pairs(lv, 0) == 4096                      # the centre offset only
    assert all(len(j) == (4096 if k == 13 else 0) for k, (j, _) in enumerate(lv.kmap(0, 0, 3)))
    assert _n_pairs(lv, 1) == 46 ** 3 == 97336          # a solid 16-cube of level-1 cells
    assert _n_pairs(lv, 2) == (3 * 8 - 2) ** 3          # ... of 8 level-2 cells per axis (origin -16 is a multiple of 4)


@pytest.mark.parametrize("cb", [10, 11, 12, 13, 14, 15, 16])
def test_corner_clusters_pair_counts_and_no_wrap(cb):
    """The eight corner clusters: 8 x 343 = 2 744 entries at level 0, 8 x 64 = 512 at level 1 (two cells per axis), 8 from level 2
    on (one cell per corner); each of the six isolated face voxels of corners(cb) adds its centre entry and nothing else; no entry
    at any level links a cell on a low face with a cell on the high face of the same axis."""
    lo, hi = -(1 << (cb - 1)), (1 << (cb - 1)) - 1
    cl = _levels([H.corner_clusters(cb)])
    lv = _levels([H.corners(cb)])
    assert lv.n(0) == 222 and lv.coords[0][:, 1:].min() == lo and lv.coords[0][:, 1:].max() == hi
    for level in range(8):
        want = 2744 if level == 0 else (512 if level == 1 else 8)
        assert _n_pairs(cl, level) == want, (cb, level)
        assert _n_pairs(lv, level) == want + 6, (cb, level)
        c = lv.coords[level].astype(np.int64)
        far = 0
        for j, o in lv.kmap(level, level, 3):
            far = max(far, int(np.abs(c[j, 1:] - c[o, 1:]).max(initial=0)))
        assert far <= (1 << level), (cb, level, far)            # an entry never spans more than one step: nothing wraps
        for kind in (1, 2):
            if level + (kind == 2) > 7 or level - (kind == 1) < 0:
                continue
            lin, _ = H.map_levels(kind, level)
            p = H.oracle_pairs(lv, kind, level)
            d = np.abs(lv.coords[lin].astype(np.int64)[p[:, 2], 1:] - c[p[:, 0], 1:])
            assert d.max() < (1 << max(lin, level)), (cb, level, kind)
    # the face voxels of one axis are never each other's neighbour
    fp = H.face_pairs(cb)
    assert all(np.abs(fp[2 * a] - fp[2 * a + 1]).max() == hi - lo for a in range(3))


def test_axis_lines_and_pow2_pairs_known_answers():
    lines = H.axis_lines(9)
    lv = _levels(lines)
    assert lv.batch_size == 7 and lv.n(0) == 63
    assert _n_pairs(lv, 0) == 7 * (9 + 2 * 8)           # per line: 9 centres + 8 pairs each way; scans never pair up
    offs = ops.kernel_offsets(3, 1)
    dirs = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1)]
    for k, (j, o) in enumerate(lv.kmap(0, 0, 3)):
        b = lv.coords[0][o, 0]
        assert np.array_equal(b, lv.coords[0][j, 0])
        for bb in np.unique(b):
            assert tuple(offs[k]) in ((0, 0, 0), dirs[bb], tuple(-np.array(dirs[bb])))
    for cb in (10, 12, 16):
        pairs = H.pow2_pairs(cb)
        lv = _levels(pairs)
        assert lv.batch_size == cb - 1 and lv.n(0) == 2 * (cb - 1)
        for level in range(8):
            c = lv.coords[level]
            for k in range(cb - 1):
                n_cells = int((c[:, 0] == k).sum())
                linked = sum(int(((c[o, 0] == k) & (j != o)).sum()) for j, o in lv.kmap(level, level, 3))
                assert n_cells == (1 if level > k else 2), (cb, level, k)
                assert linked == (2 if level == k else 0), (cb, level, k)      # neighbours at level k only


@pytest.mark.parametrize("level,n_rows", [(0, 1), (1, 17), (1, 513), (4, 1025), (7, 16)])
def test_row_count_scan_has_the_rows_it_promises(level, n_rows):
    v = H.row_count_scan(level, n_rows)
    c4, B = H.batch_of([None, v, None, 1])
    assert B == 4 and sorted(np.unique(c4[:, 0]).tolist()) == [1, 3]
    lv = ref.SparseLevels(c4)
    assert lv.n(level) == 2 * n_rows
    assert np.array_equal(lv.coords[0][c4[:, 0] == 1][:, 1:], lv.coords[0][c4[:, 0] == 3][:, 1:])
    for j, o in lv.kmap(level, level, 3):                # duplicates of a scan under another batch index never pair up
        assert np.array_equal(lv.coords[level][j, 0], lv.coords[level][o, 0])


# ------------------------------------------------------------------ (5) the comparisons of tests/test_gpu_maps.py can fail
def _synthetic_tables(kind=0, level=1):
    """a correct row-group table set, built on the host from the oracle's own map of a two-scan geometry with opposite faces"""
    cb = 10
    c4, B = H.batch_of([H.corners(cb), None, H.solid_cube(5)])
    lv = ref.SparseLevels(c4)
    lin, lout = H.map_levels(kind, level)
    c_out, c_in = lv.coords[lout], lv.coords[lin]
    boff = [int((c_out[:, 0] < b).sum()) for b in range(B + 1)]
    assert (np.diff(c_out[:, 0]) >= 0).all()                    # rows are batch-contiguous, as the row-group form needs
    pairs = H.oracle_pairs(lv, kind, level)
    perm, snbr, gmask, first = H.encode_rowgroups(pairs, H.MAP_K[kind], boff)
    return lv, c_out, c_in, boff, pairs, perm, snbr, gmask, first


def _compare(lv, c_out, c_in, boff, pairs, perm, snbr, gmask, first):
    H.check_rowgroup_form(perm, snbr, gmask, len(c_out), first, boff)
    H.assert_same_map(H.triples_by_coord(H.decode_rowgroups(perm, snbr), c_out, c_in), H.triples_by_coord(pairs, c_out, c_in), "synthetic")


@pytest.mark.parametrize("kind,level", [(0, 0), (0, 1), (1, 1), (2, 0), (0, 3)])
def test_table_comparison_accepts_a_correct_table_set(kind, level):
    t = _synthetic_tables(kind, level)
    assert t[7].shape[0] > 0 and (t[5] == -1).any() and t[8][1] == t[8][2]      # padding slots exist; the empty scan owns no group
    _compare(*t)


def test_table_comparison_rejects_a_neighbour_moved_to_the_opposite_face():
    lv, c_out, c_in, boff, pairs, perm, snbr, gmask, first = _synthetic_tables(0, 0)
    lo, hi = -512, 511
    row = {tuple(c): i for i, c in enumerate(c_out.tolist())}
    a, b, wrapped = row[(0, hi, hi, hi)], row[(0, hi - 1, hi, hi)], row[(0, lo, hi, hi)]
    g, s = np.argwhere(perm == b)[0]
    assert snbr[g, 14, s] == a                                   # slot 14 = (+1, 0, 0)
    g2, s2 = np.argwhere(perm == a)[0]
    assert snbr[g2, 14, s2] == -1                                # the corner voxel has no +x neighbour ...
    bad = snbr.copy()
    bad[g2, 14, s2] = wrapped                                    # ... a wrapped key would find the opposite face
    gm = gmask.copy()
    gm[g2] |= 1 << 14
    with pytest.raises(AssertionError, match="map entries"):
        _compare(lv, c_out, c_in, boff, pairs, perm, bad, gm, first)
    bad = snbr.copy()
    bad[g, 14, s] = wrapped                                      # an existing entry moved to the opposite-face row
    with pytest.raises(AssertionError, match="map entries differ"):
        _compare(lv, c_out, c_in, boff, pairs, perm, bad, gmask, first)


def test_table_comparison_rejects_a_cleared_gmask_bit_and_a_missing_row():
    lv, c_out, c_in, boff, pairs, perm, snbr, gmask, first = _synthetic_tables(0, 1)
    g = int(np.argmax(gmask & (1 << 13) != 0))
    for bit in (13, 31):
        gm = gmask.copy()
        gm[g] &= ~(1 << bit)
        with pytest.raises(AssertionError, match="gmask"):
            _compare(lv, c_out, c_in, boff, pairs, perm, snbr, gm, first)
    gm = gmask.copy()
    g_abs, k_abs = [(gi, k) for gi in range(len(gmask)) for k in range(27) if gmask[gi] >> 31 and not (gmask[gi] >> k) & 1][0]
    gm[g_abs] |= 1 << k_abs                                     # a bit set for an offset that no slot of the group has
    with pytest.raises(AssertionError, match="gmask"):
        _compare(lv, c_out, c_in, boff, pairs, perm, snbr, gm, first)
    # one output row missing from perm (its slot turned into padding), with and without its snbr column
    gg, ss = np.argwhere(perm >= 0)[3]
    pm = perm.copy()
    pm[gg, ss] = -1
    with pytest.raises(AssertionError, match="exactly once"):
        _compare(lv, c_out, c_in, boff, pairs, pm, snbr, gmask, first)
    sn = snbr.copy()
    sn[gg, :, ss] = -1
    with pytest.raises(AssertionError, match="exactly once"):
        _compare(lv, c_out, c_in, boff, pairs, pm, sn, gmask, first)
    # a row listed twice, a padding slot with an entry, a group of the wrong scan
    pm = perm.copy()
    pm[gg, ss] = perm[np.argwhere(perm >= 0)[4][0], np.argwhere(perm >= 0)[4][1]]
    with pytest.raises(AssertionError, match="exactly once"):
        _compare(lv, c_out, c_in, boff, pairs, pm, snbr, gmask, first)
    gp, sp = np.argwhere(perm < 0)[0]
    sn = snbr.copy()
    sn[gp, 13, sp] = 0
    with pytest.raises(AssertionError, match="padding slot"):
        _compare(lv, c_out, c_in, boff, pairs, perm, sn, gmask, first)
    f = list(first)
    f[1] = f[2] = int(np.nonzero((perm[:first[1]] >= 0).any(axis=1))[0][-1])      # scan 0's last real group handed to scan 2
    with pytest.raises(AssertionError, match="scan"):
        _compare(lv, c_out, c_in, boff, pairs, perm, snbr, gmask, f)


def test_k5_decode_rejects_a_flipped_presence_bit():
    c4, _ = H.batch_of([H.corners(10), H.solid_cube(6)])
    lv = ref.SparseLevels(c4)
    want = H.oracle_k5_presence(lv.kmap(0, 0, 5), lv.n(0))
    assert want[:, 62].all() and want.sum() == sum(len(j) for j, _ in lv.kmap(0, 0, 5))
    w = H.k5_probe_kernel()
    out = ops.conv_forward(np.ones((lv.n(0), 1), dtype=np.float32), w, lv.kmap(0, 0, 5), lv.n(0))
    assert np.array_equal(H.decode_k5_presence(out), want)
    for k in (0, 62, 124):
        bad = out.copy()
        bit = np.float32(2.0 ** (k % 4))
        bad[5, k // 4] += -bit if want[5, k] else bit
        assert not np.array_equal(H.decode_k5_presence(bad), want)
    bad = out.copy()
    bad[0, 0] += 0.5
    with pytest.raises(AssertionError, match="presence code"):
        H.decode_k5_presence(bad)


def test_integer_conv_reference_matches_the_oracle_convolution():
    c4, _ = H.batch_of([H.solid_cube(4), H.checkerboard(3)])
    lv = ref.SparseLevels(c4)
    rng = np.random.default_rng(3)
    for kind, level in [(0, 0), (0, 1), (1, 1), (2, 0)]:
        lin, lout = H.map_levels(kind, level)
        K = H.MAP_K[kind]
        x = rng.integers(-8, 9, size=(lv.n(lin), 5))
        w = rng.integers(-8, 9, size=(K, 5, 3))
        got = H.int_conv_reference(H.oracle_pairs(lv, kind, level), x, w, lv.n(lout))
        want = H.sparse_conv_f64(lv, kind, level, x, w)
        assert np.array_equal(got, want.astype(np.int64)) and np.array_equal(want, np.rint(want))

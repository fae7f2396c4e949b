"""The float64 restatement of the eval graph (oracle/egonn_f64.py), on the host:

  * chained over all stages it reproduces the committed reference fixtures within the tolerances tests/test_oracle.py uses for the
    fp32 oracle — this pins it to the reference graph;
  * chained, it agrees with oracle/egonn_ref.EgoNNOracle on the edge batches of tests/helpers.py (EDGE_BATCHES), and the per-stage
    deviation of the fp32 oracle from it under teacher forcing (the oracle's stage fed the float64 input rounded to fp32),
    e_ref(stage, batch), is computed and printed: the noise floor tests/test_gpu_forward_stages.py measures the kernels against;
  * liveness of every edge batch, from the float64 restatement alone: >= 25 % of every stage's output entries are non-zero, every
    ECA gate lies in (0.05, 0.95) on at least half of its channels, the keypoint offsets are not saturated (|pre-tanh| < 4 on 90 %
    of the rows), the softplus inputs stay below its threshold 20 — so that a stage cannot pass because it computes nothing.

DEAD lists the (batch, scan, stage) whose float64 output is all zero (none with the seeded weights used here): the GPU test holds
those to exact zeros."""
import numpy as np
import pytest

from oracle import egonn_f64 as F
from oracle import egonn_ref as ref
from tests import helpers as H

DEAD = set()                       # (batch, scan, stage): float64 output all zero — kept, and held to exact zeros on the GPU
TRUNK_CH = [32] + ref.PLANES


def _chain(name):
    b = H.edge_batch(name)
    if not hasattr(b, "chain"):
        b.chain = F.Stages(H.edge_weights(), b.mode, b.step).forward(b.lv, np.ones((b.lv.n(0), 1)), b.B)
    return b, b.chain


@pytest.mark.parametrize("name", H.CASES)
def test_chained_stages_match_reference_fixtures(name):
    case = H.load_case(name)
    polar = str(case["coordinates"]) == "polar"
    step = [float(s) for s in case["quantization_step"]]
    c4 = case["coords"]
    lv = ref.SparseLevels(c4)
    y = F.Stages(H.seeded_weights(case["weight_seed"]), 1 if polar else 0, step).forward(lv, np.ones((len(c4), 1)))
    for lvl in (3, 7):
        perm = H.join_perm(lv.coords[lvl], case[f"level{lvl}_coords"])
        np.testing.assert_allclose(y["levels"][lvl][perm], case[f"level{lvl}_feats"], rtol=2e-4, atol=2e-5)
    assert H.cosine_err(y["global"], case["global"]).max() < 1e-6
    np.testing.assert_allclose(y["global"], case["global"], rtol=1e-4, atol=1e-5)
    c3 = lv.coords[3]
    for b in range(int(case["n_scans"])):
        rows = np.nonzero(c3[:, 0] == b)[0]
        perm = rows[H.join_perm(c3[rows], case[f"kp_coords_{b}"])]
        np.testing.assert_allclose(y["local"]["keypoints"][perm], case[f"keypoints_{b}"], rtol=1e-5, atol=2e-4)
        np.testing.assert_allclose(y["local"]["sigma"][perm], case[f"sigma_{b}"], rtol=1e-4, atol=1e-5)
        assert H.cosine_err(y["local"]["descriptors"][perm], case[f"descriptors_{b}"]).max() < 1e-6


def test_bf16_rounding_is_round_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.0e38, 0.0, 2.0 ** -130])
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.0e38, 0.0, 2.0 ** -130])
    got = F.round_bf16(x)
    assert np.array_equal(got[:4], want[:4]) and got[5] == 0 and got[6] == 2.0 ** -130
    assert abs(got[4] / -3.0e38 - 1) < 2.0 ** -8
    import torch
    r = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    assert np.array_equal(F.round_bf16(r), torch.from_numpy(r).to(torch.bfloat16).double().numpy())


def test_keypoint_position_fp32_order_equals_the_oracle_quantizers():
    rng = np.random.default_rng(3)
    c3 = rng.integers(-4096, 4096, size=(500, 3)) * 8
    off = np.tanh(rng.standard_normal((500, 3))).astype(np.float32)
    for mode, step, q in ((0, [0.1], ref.CartesianQuantizer(0.1)), (1, H.POLAR_STEP, ref.PolarQuantizer(H.POLAR_STEP))):
        got, theta, _ = F.keypoint_position_f32(mode, step, c3, 3, off)
        assert np.array_equal(got, q.keypoint_position(c3, [8, 8, 8], off))
        if mode == 1:                      # physical polar cells: azimuth bins 0 .. 359 (theta beyond them loses fp32 digits)
            c3 = np.stack([rng.integers(0, 45, size=500) * 8, np.abs(c3[:, 1]) % 800, c3[:, 2] % 800], axis=1)
            got, theta, _ = F.keypoint_position_f32(mode, step, c3, 3, off)
        assert np.abs(got - F.keypoint_position_f64(mode, step, c3, 3, off)).max() <= 2e-3


@pytest.mark.parametrize("name", list(H.EDGE_BATCHES))
def test_edge_batch_agrees_with_fp32_oracle_and_e_ref(name):
    b, y = _chain(name)
    w = H.edge_weights()
    q = ref.CartesianQuantizer(0.1) if b.mode == 0 else ref.PolarQuantizer(b.step)
    o = ref.EgoNNOracle(w, q)
    lv = b.lv
    ones = np.ones((lv.n(0), 1), np.float32)
    x = o.trunk(ones, lv)
    for l in range(1, 8):
        np.testing.assert_allclose(x[l], y["levels"][l], rtol=2e-4, atol=2e-5)
    rs = F.RefStages(w, b.mode, b.step)
    g = rs.global_head(lv, x[5], x[6], x[7], "GeM", b.B)
    np.testing.assert_allclose(g, y["global"], rtol=1e-4, atol=1e-5)
    lo = rs.local_head(lv, x[3], x[4])
    # (polar corners: an azimuth of +-32 768 degrees is legal arithmetic but leaves fp32 few digits of theta — those rows are held
    #  to the fp32-order restatement of keypoint_position on the GPU, and here only the physical bins 0 .. 359 to the tolerance)
    phys = np.ones(lv.n(3), dtype=bool) if b.mode == 0 else (lv.coords[3][:, 1] >= 0) & (lv.coords[3][:, 1] < 360)
    np.testing.assert_allclose(lo["keypoints"][phys], y["local"]["keypoints"][phys], rtol=1e-5, atol=2e-4)
    np.testing.assert_allclose(lo["sigma"], y["local"]["sigma"], rtol=1e-4, atol=1e-5)
    assert H.cosine_err(lo["descriptors"], y["local"]["descriptors"]).max() < 1e-6
    # e_ref: teacher forcing, stage by stage
    table = []
    X = y["levels"]
    H.check_stage(table, name, "exact", "conv0", None, X[0], rs.conv0(lv, ones), b.scan[0], b.B)
    for i in range(1, 8):
        H.check_stage(table, name, "exact", f"block{i}", None, X[i], rs.block(lv, i, X[i - 1]), b.scan[i], b.B)
    lo = rs.local_head(lv, X[3], X[4])
    for k, s in (("descriptors", "local.desc"), ("keypoints", "local.kp"), ("sigma", "local.sigma")):
        H.check_stage(table, name, "exact", s, None, y["local"][k], lo[k], b.scan[3], b.B)
    for pool in ("GeM", "MAC", "SPoC"):
        want = y["global"] if pool == "GeM" else F.Stages(w, b.mode, b.step).global_head(lv, X[5], X[6], X[7], pool, b.B)
        H.check_stage(table, name, "exact", f"global.{pool}", None, want, rs.global_head(lv, X[5], X[6], X[7], pool, b.B),
                      np.arange(b.B), b.B)
    print("\n" + H.format_table(table))
    for _, _, stage, e_ref, _, _ in table:
        if not (stage == "local.kp" and not phys.all()):
            assert e_ref < 1e-5, (stage, e_ref)          # an fp32 stage is far inside the end-to-end bars (1e-4 .. 2e-3)


@pytest.mark.parametrize("name", list(H.EDGE_BATCHES))
def test_edge_batch_liveness(name):
    b, y = _chain(name)
    dead = set()
    for l in range(8):
        x = y["levels"][l]
        assert x.shape == (b.lv.n(l), TRUNK_CH[l])
        assert (x != 0).mean() >= 0.25, (name, l, float((x != 0).mean()))
        dead |= {(name, s, "conv0" if l == 0 else f"block{l}") for s in range(b.B)
                 if (b.scan[l] == s).any() and not x[b.scan[l] == s].any()}
        if l:
            has = np.bincount(b.scan[l], minlength=b.B)[:b.B] > 0
            g = y["gates"][l]
            assert g.shape == (b.B, TRUNK_CH[l])
            share = ((g > 0.05) & (g < 0.95)).mean(axis=1)
            assert (share[has] >= 0.5).all(), (name, l, share)
    lo = y["local"]
    assert (np.abs(lo["pre_tanh"]).max(axis=1) < 4.0).mean() >= 0.9
    assert lo["pre_softplus"].max() < 20.0
    assert (lo["descriptors"] != 0).mean() >= 0.25 and (lo["offsets"] != 0).mean() >= 0.25
    has5 = np.bincount(b.scan[5], minlength=b.B)[:b.B] > 0
    g = y["global"]
    assert (g[has5] != 0).mean() >= 0.25 and not g[~has5].any()
    dead |= {(name, int(s), "global") for s in np.nonzero(has5)[0] if not g[s].any()}
    assert dead == {d for d in DEAD if d[0] == name}, dead


def test_edge_batches_are_the_edges_they_claim():
    hb = H.edge_batch("head_tiles")
    assert np.bincount(hb.scan[3]).tolist() == H.head_tile_counts() and 16 * H.kernel_constant("LH_WAVES") in H.head_tile_counts()
    pb = H.edge_batch("pool_chunks")
    assert np.bincount(pb.scan[5]).tolist() == H.pool_chunk_counts() and H.kernel_constant("SEG_CHUNKS") in H.pool_chunk_counts()
    rb = H.edge_batch("ragged")
    assert np.bincount(rb.scan[0], minlength=6).tolist()[:4] == [1, 2, len(H.lidar_voxels(9, 40)), 0] and rb.B == 6
    assert np.bincount(rb.scan[0], minlength=6)[5] == 0
    mb = H.edge_batch("many_scans")
    n0 = np.bincount(mb.scan[0], minlength=64)
    assert mb.B == 64 and n0.max() <= 5 and (n0 == 0).sum() == 5 and n0[63] == 0
    for name in H.RANGE_CORNER_BATCHES:
        b = H.edge_batch(name)
        lo, hi = -(1 << (b.cb - 1)), (1 << (b.cb - 1)) - 1
        c3 = b.lv.coords[3][:, 1:]
        assert c3.min() == lo and c3.max() == (hi // 8) * 8          # the most negative and the most positive level-3 coordinate
        if b.mode == 1:
            t = b.lv.coords[3][b.scan[3] == 1][:, 1]
            assert t.min() == 0 and t.max() == 352                   # the first and the last azimuth cell of 8 one-degree bins

"""The fp16-split range guard at every consumer (include/egonn_hip.h, egonn_ctx_set_exact_fp32), against float64 host evaluations.

An fp16 operand part holds |x| < 65520 (65504 .. 65519.99 round to 65504 with an exact low part); beyond that, or for a non-finite
input, the plan's status must report EGONN_STATUS_FP16_RANGE (6) — for every split sparse-convolution consumer (kinds 0 / 1 / 2, the
offset parts, the tail split of levels 6-7) and for the local heads, whose ReLU would otherwise hide the NaN of an out-of-range
input.  Every forward clears the flag (a status after it covers that forward), DescriptorExtractor.extract falls back to exact fp32
by itself, the small-operand accuracy of the split is measured, and reserved plans of many scans in few rows equal eager ones."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers as H  # noqa: E402

FP16_EDGE = 65520.0
# log2 of the largest |x| of an fp32 map down to which the default split arithmetic keeps the 3e-6 bound relative to the largest
# output (test_scale_sweep_small_operands measures 2^-4.6 .. 2^-5.0 on its four layers; include/egonn_hip.h states 2^-4.5)
SMALL_OPERAND_LOG2 = -4.5


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as entry
    entry.build()
    import egonn_amd
    from egonn_amd import _lib
    egonn_amd._lib = _lib
    return egonn_amd


# ----------------------------------------------------------------------------------------------------------- operator level
class _Plan:
    """A 2-scan plan on the GPU and the same pyramid on the host (oracle.egonn_ref.SparseLevels), rows joined by coordinate."""

    def __init__(self, gpu, seeds=(61, 62), n_points=20000):
        from egonn_amd.synth import lidar_scan
        from oracle import egonn_ref as ref
        scans = [lidar_scan(s, n_points) for s in seeds]
        self.off = [0]
        for s in scans:
            self.off.append(self.off[-1] + len(s))
        self.pts = torch.from_numpy(np.concatenate(scans)).cuda()
        self.ctx = gpu._lib.Context(coord_bits=12)
        self.revoxelize()
        self.lv = ref.SparseLevels(self.ctx.level_coords(0).cpu().numpy())
        self._perm = {}

    def revoxelize(self):                 # a fresh plan: clears the flag word
        self.ctx.voxelize(self.pts, self.off, 0, [0.1])

    def perm(self, level):
        """perm with gpu_rows[perm] == host_rows"""
        if level not in self._perm:
            self._perm[level] = H.join_perm(self.ctx.level_coords(level).cpu().numpy(), self.lv.coords[level])
        return self._perm[level]

    def ref(self, kind, lvl, x, w):
        """float64 reference in GPU row order: x (GPU rows of the input level), w (K, cin, cout)"""
        lin = lvl if kind == 0 else (lvl - 1 if kind == 1 else lvl + 1)
        xh = np.asarray(x, dtype=np.float64)[self.perm(lin)]
        out = H.sparse_conv_f64(self.lv, kind, lvl, xh, np.asarray(w, dtype=np.float64))
        back = np.empty_like(out)
        back[self.perm(lvl)] = out
        return back

    def status_raised(self, gpu):
        try:
            self.ctx.plan_status()
            return False
        except gpu._lib.Fp16RangeError as e:
            assert e.code == 6
            return True


def _lin(kind, lvl):
    return lvl if kind == 0 else (lvl - 1 if kind == 1 else lvl + 1)


@pytest.fixture(scope="module")
def plan(gpu):
    return _Plan(gpu)


def _rel(got, want):
    """max |got - want| / max |want| in float64 (got a torch tensor, want a float64 numpy array)"""
    g = got.double().cpu().numpy()
    return float(np.abs(g - want).max() / np.abs(want).max())


# kind, output level, cin = cout, offset-part setting (None: the product rule; (mc, kparts, kw) via set_ksplit)
CONSUMERS = [(0, l, c, None) for l, c in zip(range(1, 8), (32, 64, 64, 128, 128, 128, 128))] + \
            [(1, l, c, None) for l, c in zip(range(1, 6), (32, 32, 64, 64, 128))] + \
            [(2, 3, 64, None), (2, 5, 128, None), (2, 6, 128, None)] + \
            [(0, l, c, (0, 1, 2)) for l, c in ((3, 64), (4, 128), (5, 128))] + \
            [(0, l, c, (0, 3, 0)) for l, c in ((3, 64), (4, 128), (5, 128))] + \
            [(1, l, c, (1, 2, 0)) for l, c in ((3, 64), (4, 64), (5, 128))]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,lvl,c,ks", CONSUMERS, ids=[f"k{k}-L{l}-{'rule' if s is None else f'kp{s[1]}kw{s[2]}'}"
                                                         for k, l, c, s in CONSUMERS])
def test_range_guard_per_split_consumer(gpu, plan, kind, lvl, c, ks):
    """Values at the first row, the last row (the tail row group) and a row of the last scan, in the last 32-channel block:
    65504 and 65519.99 (fp16 rounds both to 65504) pass within 3e-6 of the float64 reference; 65520, 7e4, 3e38, +Inf and NaN raise
    the range status (NaN comes out as NaN) — and the finite ones come within 2e-6 of float64 on the exact kernels."""
    ctx = plan.ctx
    lin = _lin(kind, lvl)
    K = 27 if kind == 0 else 8
    n_in = ctx.level_count(lin)
    boff = ctx.level_batch_offsets(lin)
    g = torch.Generator(device="cuda").manual_seed(100 * kind + lvl)
    w = (torch.randn(K, c, c, device="cuda", generator=g) / np.sqrt(c * K / 3)).contiguous()
    base = torch.randn(n_in, c, device="cuda", generator=g)
    rows = [0, n_in - 1, (boff[-2] + boff[-1]) // 2]
    signs = [1.0, -1.0, -1.0]
    ch = c - 3                                                       # in the last 32-channel block
    # linearity: ref(x) = ref(base) + v * ref(E) - ref(base at the injected entries), every term in float64
    E = np.zeros((n_in, c))
    Bm = np.zeros((n_in, c))
    bh = base.cpu().numpy().astype(np.float64)
    for r, s in zip(rows, signs):
        E[r, ch] = s
        Bm[r, ch] = bh[r, ch]
    wh = w.cpu().numpy()
    R0, RE, RB = plan.ref(kind, lvl, bh, wh), plan.ref(kind, lvl, E, wh), plan.ref(kind, lvl, Bm, wh)

    def inject(v):
        x = base.clone()
        for r, s in zip(rows, signs):
            x[r, ch] = s * v
        return x

    if ks is not None:
        ctx.set_ksplit(ks[0], lvl, kparts=ks[1], kw=ks[2], col_parts=0)
    try:
        for v in (65504.0, 65519.99):
            plan.revoxelize()
            got = ctx.sparse_conv(kind, lvl, inject(v), w)
            assert not plan.status_raised(gpu), (v, "in range: no report")
            err = _rel(got, R0 + np.float64(np.float32(v)) * RE - RB)
            assert err < 3e-6, (v, err)
        for v in (FP16_EDGE, 7e4, 3e38, float("inf"), float("nan")):
            x = inject(v)
            plan.revoxelize()
            got = ctx.sparse_conv(kind, lvl, x, w)
            assert plan.status_raised(gpu), (v, "out of range: must raise")
            if v != v:
                assert bool(torch.isnan(got).any()), "NaN propagates"
                continue
            if not np.isfinite(v):
                continue
            plan.revoxelize()
            ctx.set_exact_fp32(True)
            try:
                exact = ctx.sparse_conv(kind, lvl, x, w)
                assert not plan.status_raised(gpu)
            finally:
                ctx.set_exact_fp32(False)
            err = _rel(exact, R0 + np.float64(np.float32(v)) * RE - RB)
            assert err < 2e-6, (v, err)
    finally:
        if ks is not None:
            ctx.set_ksplit(ks[0], lvl, kparts=1, kw=2 if 3 <= lvl <= 5 else 0, col_parts=0)     # the product rule again


SWEEP = [(0, 2, 64), (1, 3, 64), (0, 5, 128), (0, 6, 128)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,lvl,c", SWEEP, ids=[f"k{k}-L{l}" for k, l, c in SWEEP])
def test_scale_sweep_small_operands(gpu, plan, kind, lvl, c):
    """x * 2^s for s = -24 .. 14 against float64 (the convolution is linear: ref(x 2^s) = 2^s ref(x)).  Exact mode: 2e-6 of the
    largest output at every s.  Operand autoscale: 3e-6 down to s = -24.  Default split: the 3e-6 bound from the measured threshold
    upward (printed; include/egonn_hip.h states it), below it the header's absolute bound per output — the low part of an activation
    carries <= 2^-25, so |err| <= 2^-25 sum_k sum_c |W| plus fp32 rounding; past 65520 the range status."""
    ctx = plan.ctx
    lin = _lin(kind, lvl)
    K = 27 if kind == 0 else 8
    g = torch.Generator(device="cuda").manual_seed(7 + lvl)
    w = (torch.randn(K, c, c, device="cuda", generator=g) / np.sqrt(c * K / 3)).contiguous()
    x = torch.randn(ctx.level_count(lin), c, device="cuda", generator=g)
    wh = w.cpu().numpy().astype(np.float64)
    xh = x.cpu().numpy().astype(np.float64)
    R = torch.from_numpy(plan.ref(kind, lvl, xh, wh)).cuda()
    A = torch.from_numpy(plan.ref(kind, lvl, np.ones_like(xh), np.abs(wh))).cuda()     # sum_k sum_c |W| per output
    Bx = torch.from_numpy(plan.ref(kind, lvl, np.abs(xh), np.abs(wh))).cuda()          # sum |x| |W| per output
    xmax = float(x.abs().max())
    table = {}
    for mode in ("exact", "autoscale", "split"):
        plan.revoxelize()
        ctx.set_exact_fp32(mode == "exact")
        ctx.set_operand_autoscale(mode == "autoscale")
        try:
            for s in range(-24, 15):
                f = 2.0 ** s
                got = ctx.sparse_conv(kind, lvl, (x * f).contiguous(), w).double()
                past = xmax * f >= FP16_EDGE
                if mode == "split" and past:
                    assert plan.status_raised(gpu), (s, "past 65520: must raise")
                    plan.revoxelize()
                    continue
                assert not plan.status_raised(gpu), (mode, s)
                d = (got - R * f).abs()
                rel = float(d.max()) / float((R * f).abs().max())
                absr = float((d / (2.0 ** -25 * A + 1e-6 * Bx * f + 1e-300)).max())
                table[(mode, s)] = (rel, absr)
                if mode == "exact":
                    assert rel < 2e-6, (mode, s, rel)
                elif mode == "autoscale":
                    assert rel < 3e-6, (mode, s, rel)
        finally:
            ctx.set_exact_fp32(False)
            ctx.set_operand_autoscale(False)
    s_min = 14
    while ("split", s_min - 1) in table and table[("split", s_min - 1)][0] < 3e-6:
        s_min -= 1
    lg = np.log2(xmax) + s_min
    print(f"\n[range sweep] kind {kind} L{lvl} {c}->{c}: split keeps 3e-6 of max|out| from s = {s_min} "
          f"(max|x| = 2^{lg:.2f}); rel / abs-bound ratio per s: " +
          " ".join(f"{s}:{table[('split', s)][0]:.1e}/{table[('split', s)][1]:.2f}" for s in range(-24, 14)))
    assert lg <= SMALL_OPERAND_LOG2, (s_min, lg)
    for s in range(-24, s_min):
        assert table[("split", s)][1] <= 1.0, (s, table[("split", s)])


# ----------------------------------------------------------------------------------------------------------- local heads
HEADS_SEED = 5


def _weights(alpha, hidden_scale=0.25):
    """seeded weights; the level-3 lateral of the local head scaled by alpha, the heads' first layers by hidden_scale (so that
    their hidden activations stay inside the fp16 range: the heads' input is the only thing that leaves it)"""
    w = {k: v.copy() for k, v in H.seeded_weights(HEADS_SEED).items()}
    w["local_head.conv1x1.3.kernel"] = (w["local_head.conv1x1.3.kernel"] * np.float32(alpha)).astype(np.float32)
    for p in ("local_descriptor_decoder", "local_keypoint_regressor", "local_sigma_regressor"):
        w[p + ".net.0.linear.weight"] = (w[p + ".net.0.linear.weight"] * np.float32(hidden_scale)).astype(np.float32)
    return w


def _model(gpu, w, n_k=128):
    mp = gpu.ModelParams(model="egonn", coordinates="cartesian", quantization_step=0.1)
    m = gpu.model_factory(mp)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    m = m.to("cuda").eval()
    return m, gpu.DescriptorExtractor(m, n_k=n_k)


def _heads_terms(gpu, m, ex, pc):
    """(lateral(x3), u3) of the local head in float64, host row order — from an exact-mode forward's level-3 / level-4 maps;
    the heads' input is alpha * lateral + u3."""
    from oracle import egonn_ref as ref
    ctx = m.context()
    ctx.set_exact_fp32(True)
    try:
        ex.extract_packed(torch.from_numpy(pc).cuda(), [0, len(pc)])
        ctx.plan_status()
        x3 = ctx.forward_level_features(3, 64).double().cpu().numpy()
        x4 = ctx.forward_level_features(4, 128).double().cpu().numpy()
    finally:
        ctx.set_exact_fp32(False)
    assert np.abs(x3).max() < 100.0, "premise: the level-3 features are O(1)"
    lv = ref.SparseLevels(ctx.level_coords(0).cpu().numpy())
    p3 = H.join_perm(ctx.level_coords(3).cpu().numpy(), lv.coords[3])
    p4 = H.join_perm(ctx.level_coords(4).cpu().numpy(), lv.coords[4])
    sd = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.state_dict().items() if k.startswith("local_head")}
    lat = x3[p3] @ sd["local_head.conv1x1.3.kernel"]
    u3 = H.sparse_conv_f64(lv, 2, 3, x4[p4] @ sd["local_head.conv1x1.4.kernel"], sd["local_head.tconv.4.kernel"])
    return lat, u3


def _peak(lat, u3, alpha):
    return float(np.abs(alpha * lat + u3).max())


def _alpha_for(lat, u3, target):
    lo, hi = 0.0, 1.0
    while _peak(lat, u3, hi) < target:
        hi *= 2.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if _peak(lat, u3, mid) < target else (lo, mid)
    return 0.5 * (lo + hi)


def _hidden_peak(w, x):
    return max(float(np.maximum(x @ w[p + ".net.0.linear.weight"].astype(np.float64).T + w[p + ".net.0.linear.bias"], 0).max())
               for p in ("local_descriptor_decoder", "local_keypoint_regressor", "local_sigma_regressor"))


@pytest.fixture(scope="module")
def heads_case(gpu):
    """one 10 k-point scan; alpha such that the heads' input peaks at 8e4 (raise) and at 6e4 (pass)"""
    from egonn_amd.synth import lidar_scan
    pc = lidar_scan(77, 10000)
    m, ex = _model(gpu, _weights(1.0))
    lat, u3 = _heads_terms(gpu, m, ex, pc)
    a_hi, a_in = _alpha_for(lat, u3, 8e4), _alpha_for(lat, u3, 6e4)
    w0 = _weights(1.0)
    assert _hidden_peak(w0, a_hi * lat + u3) < 6e4 and _hidden_peak(w0, a_in * lat + u3) < 6e4, "premise: hidden layers in range"
    return {"pc": pc, "a_hi": a_hi, "a_in": a_in}


def _oracle_local(w, pc):
    from oracle import egonn_ref as ref
    from oracle import me_ops as ops
    o = ref.EgoNNOracle(w, ref.CartesianQuantizer(0.1))
    coords, _ = o.quantizer(pc)
    bc = ops.batched_coordinates([coords])
    return o.forward(bc, np.ones((len(bc), 1), dtype=np.float32))


def _check_vs_oracle(m, y, glob, tol, min_share=1.0):
    """all level-3 rows of the last forward (model._last_local) and the global descriptor against the oracle, joined on coordinates;
    min_share < 1: keypoints and sigma within tolerance on that share of the rows, and every keypoint inside its super-voxel"""
    d, k, s = (t.cpu().numpy() for t in m._last_local)
    perm = H.join_perm(m.keypoint_coords()[0].cpu().numpy(), y["keypoint_coords"][0])
    assert H.cosine_err(glob, y["global"]).max() <= 1e-4
    assert H.cosine_err(d[perm], y["descriptors"][0]).max() <= tol["desc"]
    kp_ok = (np.abs(k[perm] - y["keypoints"][0]) <= tol["kp"]).all(axis=1)
    sg_ok = np.isclose(s[perm], y["sigma"][0], rtol=tol["sigma"], atol=1e-5).all(axis=1)
    print(f"\n[heads vs oracle] keypoints {kp_ok.mean():.4f}, sigma {sg_ok.mean():.4f} of {len(kp_ok)} rows within tolerance")
    assert kp_ok.mean() >= min_share and sg_ok.mean() >= min_share
    assert np.abs(k[perm] - y["keypoints"][0]).max() <= 2 ** 3 * 0.1 + 1e-3        # the offset's range: one level-3 voxel


FP32_TOL = {"desc": 1e-4, "kp": 2e-3, "sigma": 2e-3}           # test_fuzz_single_scan_vs_c_oracle
BF16_TOL = {"desc": 2e-4, "kp": 5e-2, "sigma": 2e-2}           # test_bf16_feature_maps_config2


@pytest.mark.gpu
def test_local_heads_input_beyond_fp16_range_is_reported(gpu, heads_case):
    """The heads' input (lateral + transposed convolution, exact fp32) beyond 65520 while every sparse convolution's input is O(1):
    the split heads must raise the range status (their first layers' ReLU turned the NaN accumulators into 0 before the guard saw
    them), exact mode must match the oracle, compute_embedding / extract must return the exact result on their own — and an input
    that peaks at 6e4 must pass on the split heads within 3e-6 of exact."""
    pc = heads_case["pc"]
    w = _weights(heads_case["a_hi"])
    m, ex = _model(gpu, w)
    ctx = m.context()
    pts = torch.from_numpy(pc).cuda()
    ex.extract_packed(pts, [0, len(pc)])
    assert float(ctx.forward_level_features(3, 64).abs().max()) < 100.0
    with pytest.raises(gpu._lib.Fp16RangeError):
        ctx.plan_status()
    # exact mode against the oracle (fp32's full range)
    ctx.set_exact_fp32(True)
    try:
        ref_out = ex.extract_packed(pts, [0, len(pc)])
        ctx.plan_status()
    finally:
        ctx.set_exact_fp32(False)
    y = _oracle_local(w, pc)
    _check_vs_oracle(m, y, ref_out["global"].cpu().numpy(), FP32_TOL)
    # the Python entry points: the exact result without being asked
    got = ex.extract([torch.from_numpy(pc)])
    ctx.plan_status()
    for key in ("global", "keypoints", "descriptors", "count", "rows"):
        assert torch.equal(got[key], ref_out[key]), key
    g, kp, desc = ex.compute_embedding(torch.from_numpy(pc))
    n = int(ref_out["count"][0])
    assert np.array_equal(g, ref_out["global"].cpu().numpy())
    assert torch.equal(kp, ref_out["keypoints"][0, :n].cpu()) and torch.equal(desc, ref_out["descriptors"][0, :n].cpu())

    # in range (peak 6e4): no report, split within 3e-6 of exact per output
    m2, ex2 = _model(gpu, _weights(heads_case["a_in"]))
    ctx2 = m2.context()
    ex2.extract_packed(pts, [0, len(pc)])
    ctx2.plan_status()
    split = [t.clone() for t in m2._last_local]
    ctx2.set_exact_fp32(True)
    try:
        ex2.extract_packed(pts, [0, len(pc)])
        ctx2.plan_status()
    finally:
        ctx2.set_exact_fp32(False)
    for a, b, name in zip(split, m2._last_local, ("descriptors", "keypoints", "sigma")):
        assert float((a - b).abs().max()) <= 3e-6 * float(b.abs().max()), name


@pytest.mark.gpu
def test_local_heads_range_bf16_maps(gpu, heads_case):
    """The same out-of-range heads' input with bf16 feature maps (the heads widen them on load): the status is raised, and the exact
    rerun matches the oracle at the bf16 tolerances of test_bf16_feature_maps_config2 — the descriptors on every row; keypoints and
    sigma on 99 % of the rows: the bf16 rounding of the level-3 map (2^-9 relative) is scaled up with the heads' input to absolute
    errors of ~1e2 in the regressors' last layers, which flips tanh / softplus on the rows whose value lies that close to 0."""
    pc = heads_case["pc"]
    w = _weights(heads_case["a_hi"])
    m, ex = _model(gpu, w)
    m.precision = "bf16"
    ctx = m.context()
    pts = torch.from_numpy(pc).cuda()
    ex.extract_packed(pts, [0, len(pc)])
    with pytest.raises(gpu._lib.Fp16RangeError):
        ctx.plan_status()
    ctx.set_exact_fp32(True)
    try:
        out = ex.extract_packed(pts, [0, len(pc)])
        ctx.plan_status()
    finally:
        ctx.set_exact_fp32(False)
    y = _oracle_local(w, pc)
    _check_vs_oracle(m, y, out["global"].cpu().numpy(), BF16_TOL, min_share=0.99)


# ----------------------------------------------------------------------------------------------------------- flag lifecycle
@pytest.mark.gpu
def test_flag_cleared_by_the_next_forward_on_the_same_plan(gpu, heads_case):
    """A flagged forward, then exact mode and a forward on the SAME plan (no new voxelisation): the status covers the second
    forward only — clean — and its outputs match the oracle.  Also the throughput path: extract_packed does not read the flag, the
    caller's plan_status() reports the batch."""
    pc = heads_case["pc"]
    w = _weights(heads_case["a_hi"])
    m, ex = _model(gpu, w)
    ctx = m.context()
    out = ex.extract_packed(torch.from_numpy(pc).cuda(), [0, len(pc)])
    assert out["global"].shape == (1, 256)
    with pytest.raises(gpu._lib.Fp16RangeError):
        ctx.plan_status()
    ctx.set_exact_fp32(True)
    try:
        y_gpu = m._forward_on_plan(ctx, None)
        ctx.plan_status()
    finally:
        ctx.set_exact_fp32(False)
    _check_vs_oracle(m, _oracle_local(w, pc), y_gpu["global"].cpu().numpy(), FP32_TOL)


@pytest.mark.gpu
def test_flag_follows_the_batch_under_graph_replay(gpu):
    """GraphExtractor (one captured voxelise -> forward -> select): same weights, a 2 k-point scan whose heads' input stays in range
    and a 50 k-point scan whose peak crosses 65520 — status() raises after the second and is clean after the first again."""
    from egonn_amd.synth import lidar_scan
    small, big = lidar_scan(91, 2000), lidar_scan(91, 50000)
    m, ex = _model(gpu, _weights(1.0))
    ls, us = _heads_terms(gpu, m, ex, small)
    lb, ub = _heads_terms(gpu, m, ex, big)
    # alpha between the two peaks: the geometric mean of the two peaks at 65520
    lo, hi = 0.0, 1.0
    gm = lambda a: np.sqrt(_peak(ls, us, a) * _peak(lb, ub, a))
    while gm(hi) < FP16_EDGE:
        hi *= 2.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if gm(mid) < FP16_EDGE else (lo, mid)
    alpha = 0.5 * (lo + hi)
    ps, pb = _peak(ls, us, alpha), _peak(lb, ub, alpha)
    assert pb / ps >= 1.5, f"precondition: peak ratio {pb / ps:.3f} (synthetic scans changed?)"
    w0 = _weights(1.0)
    assert _hidden_peak(w0, alpha * lb + ub) < 6e4 and _hidden_peak(w0, alpha * ls + us) < 6e4
    m, ex = _model(gpu, _weights(alpha))
    caps = ex.calibrate(torch.from_numpy(big).cuda(), [0, len(big)])
    ge = ex.graph(1, len(big), caps, slot=1)
    ps_dev, pb_dev = torch.from_numpy(small).cuda(), torch.from_numpy(big).cuda()
    ge.run(ps_dev, [0, len(small)])
    ge.status()
    ge.run(pb_dev, [0, len(big)])
    with pytest.raises(gpu._lib.Fp16RangeError):
        ge.status()
    ge.run(ps_dev, [0, len(small)])
    ge.status()


@pytest.mark.gpu
def test_flag_raised_in_train_mode(gpu):
    """Train mode (SparseConvFn on the split kernels): a level-1 BatchNorm bias of 1e6 puts the rows that the level-2 strided
    convolution gathers out of range — the flag is raised and readable through plan_status()."""
    case = H.load_case("egonn_cart01_b1")
    w = {k: v.copy() for k, v in H.seeded_weights(int(case["weight_seed"])).items()}
    w["trunk.blocks.1.0.norm2.bn.bias"] = np.full_like(w["trunk.blocks.1.0.norm2.bn.bias"], 1e6)
    mp = gpu.ModelParams(model="egonn", coordinates="cartesian", quantization_step=0.1)
    m = gpu.model_factory(mp)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    m = m.to("cuda").train()
    coords = torch.from_numpy(case["coords"]).cuda()
    m({"coords": coords, "features": torch.ones((len(coords), 1), device="cuda")})
    with pytest.raises(gpu._lib.Fp16RangeError):
        m.context().plan_status()


# ----------------------------------------------------------------------------------------------------------- reserved plans
def _sparse_batch(n_scans=600, seed=3):
    """most scans empty, a few with 1-3 points, the last one among them"""
    rng = np.random.default_rng(seed)
    counts = np.zeros(n_scans, dtype=np.int64)
    for b in (0, 17, 255, 256, 300, 511, 599):
        counts[b] = 1 + (b % 3)
    off = np.concatenate([[0], np.cumsum(counts)])
    pts = (rng.standard_normal((int(off[-1]), 3)) * 5.0).astype(np.float32)
    return pts, off


@pytest.mark.gpu
@pytest.mark.parametrize("extra_rows", [0, 150])
def test_reserved_plan_of_many_scans_in_few_rows(gpu, extra_rows):
    """reserve(200 points, 600 scans), voxelize_device with fewer than 256 rows (the key kernel's grid is one workgroup, smaller than
    the 601 scan offsets): per-level counts, level_batch_offsets and level coordinates equal the eager plan of the same input; rows
    beyond scan_offsets[B] (extra_rows of them) are ignored."""
    pts, off = _sparse_batch()
    rng = np.random.default_rng(11)
    rows = np.concatenate([pts, (rng.standard_normal((extra_rows, 3)) * 5.0).astype(np.float32)]) if extra_rows else pts
    assert len(rows) < 256
    dev_pts = torch.from_numpy(rows).cuda().contiguous()
    eager = gpu._lib.Context(coord_bits=12)
    eager.voxelize(torch.from_numpy(pts).cuda().contiguous(), off.tolist(), 0, [0.1])
    res = gpu._lib.Context(coord_bits=12)
    res.reserve(200, 600)
    res.voxelize_device(dev_pts, torch.from_numpy(off).cuda(), 600, 0, [0.1])
    res.plan_status()
    for l in range(8):
        assert res.level_count(l) == eager.level_count(l), l
        assert res.level_batch_offsets(l) == eager.level_batch_offsets(l), l
        assert torch.equal(res.level_coords(l), eager.level_coords(l)), l


@pytest.mark.gpu
def test_operand_autoscale_refused_on_reserved_plans(gpu):
    """The autoscale reads the map's row count on the host: a reserved context refuses it (EGONN_ERR_STATE), with the reason."""
    ctx = gpu._lib.Context(coord_bits=12)
    ctx.reserve(1000, 2)
    with pytest.raises(gpu._lib.EgonnError) as ei:
        ctx.set_operand_autoscale(True)
    assert ei.value.code == 4 and "eager plans only" in str(ei.value)
    ctx.set_operand_autoscale(False)
    other = gpu._lib.Context(coord_bits=12)
    other.set_operand_autoscale(True)
    with pytest.raises(gpu._lib.EgonnError) as ei:
        other.reserve(1000, 2)
    assert ei.value.code == 4

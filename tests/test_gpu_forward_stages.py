"""The eval forward, stage by stage against float64, on the edge batches of tests/helpers.py (EDGE_BATCHES).

Method.  Every forward runs with keep_level_features(True); the eight level maps (forward_level_features), the local outputs of
every level-3 row (model._last_local) and the global descriptor are read back and joined on coordinates with the oracle's pyramid.
Each stage of oracle/egonn_f64.py (conv0, block 1..7, local head, global head) is fed the GPU's OWN input maps, widened to
float64, and its output is compared with what the GPU produced for that stage: errors do not accumulate across stages, so every
stage is held to its own rounding.  e = max |got - want64| / max |want64| over the stage's output and, again, per scan of the batch
(a one-voxel scan next to a 3 000-point scan is held to its own scale).

Bounds (tests/helpers.py:stage_bound) — none of them comes from the kernels' output:
  exact fp32   8 x e_ref, e_ref = the deviation of the fp32 numpy oracle's stage (oracle/egonn_ref.py) from float64 on the same
               input, computed here at run time; floor 16 x 2^-24.  8: another summation order, not another algorithm.
  product      that plus 3e-6 per split sparse convolution of the stage (README, test_split_conv_matches_exact_fp32) and 3e-6 for
               the split heads (test_local_heads_input_beyond_fp16_range_is_reported).
  bf16 maps    (bf16 stores between the observed input and output) x 2^-8 of the stage's largest value: a derived count.
  1 - cos      for unit vectors 1 - cos = |a - b|^2 / 2 <= 128 x (descriptor bound)^2 / 2: implied by the descriptor bound.
  sigma, per row, relative: d log softplus(x) / dx <= 1, so the fp32 bound is 8 x (the oracle's same figure) and the product
               allowance is 6e-6 x max |pre-activation|.
  polar cos / sin (regressor ignored): 4 x the largest deviation of numpy's fp32 cos / sin from float64 on the same fp32 thetas,
               times the row's radius, plus one rounding of the product.

Configurations per batch: (1) product dispatch, with unit features (the product's occupancy-only first layer) and with non-constant
features (first layer only), and a second forward without keep_level_features — there the gated level-1 tail runs inside level 2's
strided convolution and level 1 is not observable: its level maps >= 2 and outputs must be torch.equal those of the first forward,
every stage of which was checked (stronger than a two-stage float64 chain); (2) set_exact_fp32; (3) bf16 maps against the bf16
variant of the stages; (4) two reserved plans (all capacities large: fused downsample epilogue, five-launch global head; levels
5-7 small: fused global head) whose buffers hold a larger batch — a superset of every scan — from the forward before: bitwise
configuration 1 on the rows in use, and the local output rows beyond the live count untouched (n_dev / boff[B] clipping); (5) local
head only / global head only, MAC and SPoC pooling (pool_chunks, ragged), EGONN_FLAG_IGNORE_KP_REGRESSOR on the range corners, where
Cartesian keypoints equal the fp32-order restatement of keypoint_position exactly.  Every forward runs twice: bitwise equal.

Coverage guard.  The profile tags (egonn_profile_fetch) name the sparse-convolution kernels only: configuration 1 must show
sconv_split_kernel launches and configuration 2 none.  The gated strided convolution carries the same tag as the plain one; it is
identified by what it leaves behind instead — without keep_level_features, forward_level_features(1) has no map to return (and has
one in exact mode).  The split heads kernel and the grouped lateral launch carry no profile tag, so no assertion names them."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_forward_f64_host import DEAD

CH = [32, 32, 64, 64, 128, 128, 128, 128]
TABLE = []


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as entry
    entry.build()
    import egonn_amd
    from egonn_amd import _lib
    egonn_amd._lib = _lib
    yield egonn_amd
    print("\n[forward stages] stage x configuration x batch\n" + H.format_table(TABLE))


def _np(t):
    return t.detach().cpu().numpy()


class _Run:
    """one edge batch on the GPU: model, eager context, the batch as points at voxel centres (step 1), joins to the oracle's rows"""

    def __init__(self, gpu, name):
        self.gpu, self.b = gpu, H.edge_batch(name)
        b = self.b
        self.w = H.edge_weights()
        mp = gpu.ModelParams(model="egonn", coordinates=b.coordinates, quantization_step=0.1 if b.mode == 0 else b.step)
        m = gpu.model_factory(mp)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in self.w.items()})
        self.m = m.to("cuda").eval()
        self.m.coord_bits = b.cb
        self.ctx = self.m.context()
        self.pts = torch.from_numpy(b.c4[:, 1:].astype(np.float32) + np.float32(0.5)).cuda().contiguous()
        self.off = [int((b.c4[:, 0] < s).sum()) for s in range(b.B + 1)]
        self.perm = None

    def forward(self, keep=True, exact=False, bf16=False, feats=None, pool="GeM", no_global=False, no_local=False, ignore_kp=False,
                profile=False):
        m, ctx, b = self.m, self.ctx, self.b
        ctx.keep_level_features(keep)
        ctx.set_exact_fp32(exact)
        m.precision = "bf16" if bf16 else "fp32"
        m.global_pool_method, m.ignore_keypoint_regressor = pool, ignore_kp
        try:
            ctx.voxelize(self.pts, self.off, 0, [1.0])
            if self.perm is None:      # gpu_rows[perm[l]] == oracle rows
                self.perm = [H.join_perm(_np(ctx.level_coords(l)), b.lv.coords[l]) for l in range(8)]
            f = None
            if feats is not None:      # voxelize plans take features in level-0 row order
                inv = np.empty_like(self.perm[0])
                inv[self.perm[0]] = np.arange(len(inv))
                f = torch.from_numpy(np.ascontiguousarray(feats[inv])).cuda()
            if profile:
                ctx.profile_enable(1)
                ctx.profile_fetch()
            y = m._forward_on_plan(ctx, f, no_global, no_local)
            ctx.plan_status()
            out = {"names": [r[0] for r in ctx.profile_fetch()] if profile else None}
            out["global"] = None if no_global else y["global"].clone()
            out["local"] = None if no_local else tuple(t.clone() for t in m._last_local)
            out["levels"] = {}
            for l in range(8):
                if keep or l != 1 or exact or bf16:
                    out["levels"][l] = ctx.forward_level_features(l, CH[l])
            return out
        finally:
            ctx.profile_enable(0)
            ctx.set_exact_fp32(False)
            ctx.keep_level_features(False)
            m.precision, m.global_pool_method, m.ignore_keypoint_regressor = "fp32", "GeM", False

    def host(self, out):
        """levels / local / global of a forward in the oracle's row order, float64"""
        X = {l: _np(t).astype(np.float64)[self.perm[l]] for l, t in out["levels"].items()}
        loc = None if out["local"] is None else [_np(t).astype(np.float64)[self.perm[3]] for t in out["local"]]
        return X, loc, None if out["global"] is None else _np(out["global"]).astype(np.float64)


def _same(a, b, what, fails, levels=True):
    """bitwise equality of two forwards' outputs (and level maps)"""
    if a["global"] is not None and b["global"] is not None and not torch.equal(a["global"], b["global"]):
        fails.append(f"{what}: global descriptors differ")
    if a["local"] is not None and b["local"] is not None:
        for t, u, n in zip(a["local"], b["local"], ("descriptors", "keypoints", "sigma")):
            if not torch.equal(t, u):
                fails.append(f"{what}: {n} differ")
    if levels:
        for l in set(a["levels"]) & set(b["levels"]):
            if not torch.equal(a["levels"][l], b["levels"][l]):
                fails.append(f"{what}: level-{l} maps differ")


def _dead(name, stage):
    return tuple(s for (n, s, st) in DEAD if n == name and st == stage)


def _check_local(r, config, st, rs, X, loc, fails, ignore_kp=False):
    from oracle import egonn_f64 as F
    b, name = r.b, r.b.name
    lv, scan = b.lv, b.scan[3]
    want = st.local_head(lv, X[3], X[4], ignore_kp)
    ref32 = rs.local_head(lv, X[3], X[4], ignore_kp) if rs is not None else None
    share = 0.99 if config == "bf16" else 1.0
    tag = ".nokp" if ignore_kp else ""
    for i, (k, s) in enumerate((("descriptors", "local.desc"), ("keypoints", "local.kp"), ("sigma", "local.sigma"))):
        fails += H.check_stage(TABLE, name, config, s + tag, loc[i], want[k], None if ref32 is None else ref32[k], scan, b.B,
                               min_share=1.0 if k == "descriptors" else share)
    d_bound = TABLE[-3][5]
    nrm = np.sqrt((loc[0] ** 2).sum(axis=1))
    if np.abs(nrm - 1.0).max(initial=0.0) > 1e-6:
        fails.append(f"{name}/{config}: descriptor norm off by {np.abs(nrm - 1.0).max():.2e} at row {int(np.argmax(np.abs(nrm - 1)))}")
    cos = H.cosine_err(loc[0], want["descriptors"])
    cos_bound = 64.0 * (d_bound * np.abs(want["descriptors"]).max()) ** 2 + 2e-6           # (+ the norm allowance, twice)
    if cos.max(initial=0.0) > cos_bound:
        fails.append(f"{name}/{config}: 1 - cos {cos.max():.3e} > {cos_bound:.3e} at row {int(np.argmax(cos))} (scan {scan[int(np.argmax(cos))]})")
    # every keypoint inside its level-3 super-voxel (polar: the z axis, the one the transform leaves alone)
    s3 = np.asarray([np.float32(v) for v in (b.step * 3)[:3]], dtype=np.float64)
    centre = (lv.coords[3][:, 1:].astype(np.float64) + 0.5) * s3
    axes = [0, 1, 2] if b.mode == 0 else [2]
    dev = np.abs(loc[1] - centre)[:, axes] - 4.0 * s3[axes] * (1 + 1e-6) - 2.0 ** -23 * np.abs(centre[:, axes])
    if (dev > 0).any():
        fails.append(f"{name}/{config}: a keypoint lies outside its super-voxel (row {int(np.argmax(dev.max(axis=1)))})")
    if config != "bf16":
        rel = np.abs(loc[2] - want["sigma"]) / want["sigma"]
        rel_ref = np.abs(ref32["sigma"].astype(np.float64) - want["sigma"]) / want["sigma"]
        bound = max(8.0 * rel_ref.max(initial=0.0), H.FP32_FLOOR)
        if config == "product":
            bound += (H.SPLIT_CONV + H.SPLIT_HEADS) * max(1.0, np.abs(want["pre_softplus"]).max())
        print(f"[sigma per row] {name}/{config}: relative error {rel.max():.3e}, oracle {rel_ref.max():.3e}, bound {bound:.3e}; "
              f"keypoints: {np.abs(loc[1] - want['keypoints']).max():.3e} m")
        if rel.max(initial=0.0) > bound:
            fails.append(f"{name}/{config}: sigma relative error {rel.max():.3e} > {bound:.3e} at row {int(np.argmax(rel))}")
    if ignore_kp:
        kp32, theta, radius = F.keypoint_position_f32(b.mode, b.step, lv.coords[3][:, 1:], 3, np.zeros((lv.n(3), 3), np.float32))
        got32 = _np(r._last_kp)[r.perm[3]]
        if b.mode == 0:
            if not np.array_equal(got32, kp32):
                fails.append(f"{name}/{config}: Cartesian keypoints differ from the fp32-order restatement of keypoint_position")
        else:
            t64 = theta.astype(np.float64)
            dv = max(np.abs(np.cos(theta).astype(np.float64) - np.cos(t64)).max(), np.abs(np.sin(theta).astype(np.float64) - np.sin(t64)).max())
            tol = 4.0 * dv * np.abs(radius.astype(np.float64))[:, None] + 2.0 ** -23 * np.abs(kp32.astype(np.float64))
            bad = np.abs(got32.astype(np.float64) - kp32.astype(np.float64)) > tol
            bad[:, 2] = got32[:, 2] != kp32[:, 2]
            print(f"[polar cos/sin] {name}: numpy fp32 deviation {dv:.2e}, GPU - numpy fp32 max "
                  f"{np.abs(got32.astype(np.float64) - kp32)[:, :2].max():.3e}")
            if bad.any():
                fails.append(f"{name}/{config}: polar keypoints beyond the cos/sin bound at row {int(np.argmax(bad.any(axis=1)))}")


def _check_global(r, config, st, rs, X, glob, pool, fails):
    b = r.b
    want = st.global_head(b.lv, X[5], X[6], X[7], pool, b.B)
    ref32 = rs.global_head(b.lv, X[5], X[6], X[7], pool, b.B) if rs is not None else None
    fails += H.check_stage(TABLE, b.name, config, f"global.{pool}", glob, want, ref32, np.arange(b.B), b.B,
                           exact_zero=_dead(b.name, "global"))
    empty = np.bincount(b.scan[5], minlength=b.B)[:b.B] == 0
    if glob[empty].any() or not np.isfinite(glob).all():
        fails.append(f"{b.name}/{config}/{pool}: the global descriptor of an empty scan is not exactly 0 (or NaN / Inf)")


def _check_forward(r, config, out, fails, feats=None, conv0_only=False):
    """every stage of one forward against float64 on the GPU's own inputs"""
    from oracle import egonn_f64 as F
    b, name = r.b, r.b.name
    st = F.Stages(r.w, b.mode, b.step, bf16=config == "bf16")
    rs = F.RefStages(r.w, b.mode, b.step) if config != "bf16" else None
    X, loc, glob = r.host(out)
    for l, x in X.items():
        if not np.isfinite(x).all():
            fails.append(f"{name}/{config}: NaN or Inf in the level-{l} map")
    f = np.ones((b.lv.n(0), 1), np.float32) if feats is None else feats
    fails += H.check_stage(TABLE, name, config, "conv0" if feats is None else "conv0.feat", X[0], st.conv0(b.lv, f),
                           rs.conv0(b.lv, f) if rs else None, b.scan[0], b.B, exact_zero=_dead(name, "conv0"))
    if conv0_only:
        return
    for i in range(1, 8):
        w = st.block(b.lv, i, X[i - 1], b.B)
        fails += H.check_stage(TABLE, name, config, f"block{i}", X[i], w["out"], rs.block(b.lv, i, X[i - 1]) if rs else None,
                               b.scan[i], b.B, gate=w["gate"], exact_zero=_dead(name, f"block{i}"))
    _check_local(r, config, st, rs, X, loc, fails)
    _check_global(r, config, st, rs, X, glob, "GeM", fails)


def _stale_scans(b):
    """a larger batch with the same number of scans: scan s = the live scan, the live scan moved by one voxel, and a slab of a
    30 k-point lidar scan — a superset of every live scan, so every buffer of the plan holds more rows than the live batch needs"""
    lo, hi = -(1 << (b.cb - 1)), (1 << (b.cb - 1)) - 1
    v = H.lidar_voxels(78, 30000)
    v = v[((v >= lo) & (v <= hi)).all(axis=1)]
    cut = np.linspace(0, len(v), b.B + 1).astype(int)
    scans = []
    for s in range(b.B):
        live = b.c4[b.c4[:, 0] == s][:, 1:].astype(np.int64)
        moved = live + np.array([1, 0, 0])
        moved = moved[(moved <= hi).all(axis=1)]
        scans.append(np.unique(np.concatenate([live, moved, v[cut[s]:cut[s + 1]]]), axis=0))
    return scans


def _reserved(r, base, caps, what, fails):
    """configuration 4: the live batch on a reserved plan whose buffers hold the stale batch of the forward before"""
    gpu, m, b = r.gpu, r.m, r.b
    scans = _stale_scans(b)
    stale = np.concatenate(scans).astype(np.float32) + np.float32(0.5)
    soff = np.concatenate([[0], np.cumsum([len(s) for s in scans])])
    max_points = 65536
    assert len(stale) <= max_points and len(stale) > len(b.c4)
    ctx = gpu._lib.Context(m._device(), coord_bits=b.cb)
    ctx.reserve(max_points, b.B, caps)
    ctx.keep_level_features(True)
    buf = torch.zeros((max_points, 3), dtype=torch.float32, device="cuda")
    buf[:len(stale)] = torch.from_numpy(stale).cuda()
    ctx.voxelize_device(buf, torch.from_numpy(soff.astype(np.int64)).cuda(), b.B, 0, [1.0])
    ctx.plan_status()
    cap3 = ctx.level_capacity(3)
    outs = (torch.zeros((b.B, 256), device="cuda"), torch.zeros((cap3, 128), device="cuda"), torch.zeros((cap3, 3), device="cuda"),
            torch.zeros((cap3, 1), device="cuda"))
    m._forward_on_plan(ctx, None, outputs=outs)
    ctx.plan_status()
    n_stale = [ctx.level_count(l) for l in range(8)]
    snap = [t.clone() for t in outs]
    buf[:len(r.pts)] = r.pts
    ctx.voxelize_device(buf, torch.tensor(r.off, dtype=torch.int64).cuda(), b.B, 0, [1.0])
    m._forward_on_plan(ctx, None, outputs=outs)
    ctx.plan_status()
    n3 = ctx.level_count(3)
    for l in range(8):
        assert n_stale[l] > ctx.level_count(l) == b.lv.n(l), (what, l, n_stale[l], ctx.level_count(l))
        if not torch.equal(ctx.forward_level_features(l, CH[l]), base["levels"][l]):
            fails.append(f"{b.name}/{what}: level-{l} map differs from configuration 1 on an eager plan")
    if not torch.equal(outs[0], base["global"]):
        fails.append(f"{b.name}/{what}: global descriptor differs from configuration 1")
    for t, u, s, n in zip(outs[1:], base["local"], snap[1:], ("descriptors", "keypoints", "sigma")):
        if not torch.equal(t[:n3], u):
            fails.append(f"{b.name}/{what}: {n} of the rows in use differ from configuration 1")
        if not torch.equal(t[n3:], s[n3:]):
            fails.append(f"{b.name}/{what}: {n} rows beyond the live count were written (n_dev clipping)")
    assert bool((snap[1][n3:n_stale[3]] != 0).any()), "premise: the rows beyond the live count hold the stale batch's outputs"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(H.EDGE_BATCHES))
def test_forward_stages_vs_float64(gpu, name):
    r = _Run(gpu, name)
    b = r.b
    fails = []
    first = len(TABLE)
    # ---- configuration 1: product dispatch
    base = r.forward(profile=True)
    _same(base, r.forward(), f"{name}/product: second run", fails)
    assert any("sconv_split_kernel" in n for n in base["names"]), base["names"]
    _check_forward(r, "product", base, fails)
    feats = b.features()
    _check_forward(r, "product", r.forward(feats=feats), fails, feats=feats, conv0_only=True)
    gated = r.forward(keep=False)
    with pytest.raises(gpu._lib.EgonnError):                   # the gated strided convolution ran: level 1 was never written
        r.ctx.forward_level_features(1, CH[1])
    _same(base, gated, f"{name}/product: forward with the gated level-1 tail", fails)
    _same(gated, r.forward(keep=False), f"{name}/product, gated: second run", fails)
    # ---- configuration 2: exact fp32
    ex = r.forward(exact=True, profile=True)
    assert ex["names"] and not any("sconv_split_kernel" in n for n in ex["names"]), ex["names"]
    _same(ex, r.forward(exact=True), f"{name}/exact: second run", fails)
    _check_forward(r, "exact", ex, fails)
    _check_forward(r, "exact", r.forward(exact=True, feats=feats), fails, feats=feats, conv0_only=True)
    assert 1 in r.forward(exact=True, keep=False)["levels"]      # no gated tail off the split pipe: level 1 exists
    # ---- configuration 3: bf16 maps
    bf = r.forward(bf16=True)
    _same(bf, r.forward(bf16=True), f"{name}/bf16: second run", fails)
    _check_forward(r, "bf16", bf, fails)
    # ---- configuration 4: reserved plans with stale contents
    _reserved(r, base, None, "reserved", fails)
    _reserved(r, base, [65536] * 5 + [4096] * 3, "reserved, small top levels", fails)
    # ---- configuration 5: one head only; other poolings; the keypoint regressor ignored
    lo = r.forward(no_global=True)
    go = r.forward(no_local=True)
    _same(base, lo, f"{name}: local head only", fails)
    _same(base, go, f"{name}: global head only", fails)
    if name in ("pool_chunks", "ragged"):
        from oracle import egonn_f64 as F
        for pool in ("MAC", "SPoC"):
            for config, kw in (("product", {}), ("exact", {"exact": True})):
                o = r.forward(pool=pool, **kw)
                _same({**(base if config == "product" else ex), "global": None}, o, f"{name}/{config}/{pool}: trunk and local head", fails)
                _same(o, r.forward(pool=pool, **kw), f"{name}/{config}/{pool}: second run", fails)
                X, _, glob = r.host(o)
                _check_global(r, config, F.Stages(r.w, b.mode, b.step), F.RefStages(r.w, b.mode, b.step), X, glob, pool, fails)
    if name in H.RANGE_CORNER_BATCHES:
        from oracle import egonn_f64 as F
        for config, kw in (("product", {}), ("exact", {"exact": True})):
            o = r.forward(ignore_kp=True, **kw)
            _same(o, r.forward(ignore_kp=True, **kw), f"{name}/{config}: regressor ignored, second run", fails)
            r._last_kp = o["local"][1]
            X, loc, _ = r.host(o)
            _check_local(r, config, F.Stages(r.w, b.mode, b.step), F.RefStages(r.w, b.mode, b.step), X, loc, fails, ignore_kp=True)
    print("\n" + H.format_table(TABLE[first:]))
    assert not fails, "\n".join(fails)

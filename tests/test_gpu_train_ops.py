"""Every train-mode operator (egonn_amd/train.py, csrc/train.hip) against a plain float64 reference of the same operation, at
the shapes, value ranges and batch layouts where reductions and per-sample kernels go wrong.

References are torch float64 autograd of the reference formulas (nn.BatchNorm1d, layers/pooling.py GeM, layers/eca_block.py,
F.normalize, the activations) and a host float64 loop over the kernel maps (oracle SparseLevels) for the convolutions.  Very
large column reductions (up to 600 000 x 256) are summed by torch in float64 on the device: the reference is the fp64 sum, not
the kernel under test.

Tolerances are derived, not fitted; u = 2^-24 is the fp32 unit roundoff.  A serial fp32 sum of L terms is off by at most
L u sum|terms|; fp64 sums (the column statistics) by a negligible 2^-53 n sum|terms|.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import helpers as H

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from egonn_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(lib):
    """a plan-less context is enough for the row-wise operators (col_stats, act, l2, dense weight gradient)"""
    return lib.Context(lib.require_gpu(), coord_bits=12)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _plan_from_counts(lib, counts, seed=0):
    """a context whose level 0 holds exactly `counts[b]` rows for sample b (0 = an empty sample), via egonn_coords_set"""
    dev = lib.require_gpu()
    c = lib.Context(dev, coord_bits=12)
    rng = np.random.default_rng(seed)
    parts = []
    for b, n in enumerate(counts):
        if n == 0:
            continue
        flat = rng.choice(64 ** 3, size=n, replace=False)
        xyz = np.stack([flat % 64, (flat // 64) % 64, flat // 4096], 1) - 32
        parts.append(np.concatenate([np.full((n, 1), b), xyz], 1))
    coords = np.concatenate(parts).astype(np.int32)
    c.coords_set(torch.from_numpy(coords).to(dev).contiguous(), len(counts))
    off = c.level_batch_offsets(0)
    assert [off[b + 1] - off[b] for b in range(len(counts))] == list(counts)
    return c


# ============================================================================================================ 1. BatchNorm
def _stats(ctx, x, shift, n_total=None):
    """exactly what BatchNormFn.forward computes before it normalises: col_stats mode 3 around `shift` + the finalize kernel
    (no running-statistics update) -> mean, invstd (fp32 tensors on the device)"""
    n, c = x.shape
    s = ctx.col_stats(3, x, mean=shift)
    assert s.dtype == torch.float64
    out4 = torch.empty((4, c), dtype=torch.float32, device=x.device)
    w = torch.ones(c, device=x.device)
    b = torch.zeros(c, device=x.device)
    ctx._call(ctx.lib.egonn_bn_train_finalize, s.data_ptr(), shift.data_ptr(), float(n if n_total is None else n_total), c,
              w.data_ptr(), b.data_ptr(), 1e-5, 0.0, None, None, out4.data_ptr())
    return out4[0], out4[1]


def _bn_input(n, c, R, seed, dev):
    """rows with per-channel std in [0.5, 2] and |mean| = R * std (alternating sign); channel 1 constant (var = 0)"""
    g = _gen(seed)
    std = 0.5 + 1.5 * torch.rand(c, generator=g, dtype=torch.float64)
    sign = torch.where(torch.arange(c) % 2 == 0, 1.0, -1.0).double()
    x = torch.randn((n, c), generator=g, dtype=torch.float64) * std + sign * R * std
    if c > 1:
        x[:, 1] = 0.75
    return x.float().to(dev)


def _rel(got, want, floor):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float(((got - want).abs() / torch.maximum(want.abs(), floor)).max())


COL_LAYOUTS = [(32, "vec"), (64, "vec"), (128, "vec"), (256, "vec"), (1, "scalar"), (3, "scalar"), (96, "scalar"),
               (64, "misaligned")]
COL_ROWS = [2, 31, 33, 1023, 1025, 8160, 8161, 8192, 8193, 600_000]


@pytest.mark.parametrize("c,layout", COL_LAYOUTS, ids=[f"{c}-{l}" for c, l in COL_LAYOUTS])
def test_col_stats_every_kernel_path_matches_fp64(ctx, c, layout):
    """egonn_col_stats on col_stats4_kernel (C = 32..256, 16-byte aligned), the scalar col_stats_kernel (C = 1, 3, 96, and C = 64
    read through a view one float off 16-byte alignment), at row counts on both sides of the reducer switch
    (sum_partials_wave below 256 partial blocks, sum_partials_block from 256) and of every rows-per-block step, up to 600 000
    rows.  All four modes against fp64 sums: the kernels form differences, products and sums in fp64, so |err| <= 1e-12 sum|terms|
    (2^-53 times the ~10^4-deep chains, with margin) — then mean and invstd to 1e-5 relative with mean/std = 30."""
    dev = ctx.device
    for n in COL_ROWS:
        if n > 100_000 and c in (1, 3):
            continue
        x = _bn_input(n, c, 30.0, 100 + n % 997 + c, dev)
        if layout == "misaligned":
            buf = torch.empty(n * c + 1, device=dev)
            buf[1:] = x.reshape(-1)
            x = buf[1:].view(n, c)
            assert x.data_ptr() % 16 != 0
        g = torch.randn((n, c), generator=_gen(n + c), dtype=torch.float32).to(dev)
        mask = (torch.rand((n, c), generator=_gen(n + 2 * c)) > 0.3).float().to(dev)
        shift = (x[: min(n, 5)].mean(0) * 0.5).contiguous()
        xd, gd, md, sd = x.double(), g.double(), mask.double(), shift.double()
        d = xd - sd
        gm = gd * md
        cases = {0: (xd.sum(0), xd.abs().sum(0), (xd * xd).sum(0), (xd * xd).sum(0)),
                 1: ((d * d).sum(0), (d * d).sum(0), torch.zeros_like(sd), torch.zeros_like(sd)),
                 2: (gm.sum(0), gm.abs().sum(0), (gm * (xd - sd)).sum(0), (gm * (xd - sd)).abs().sum(0)),
                 3: (d.sum(0), d.abs().sum(0), (d * d).sum(0), (d * d).sum(0))}
        for mode, (w0, a0, w1, a1) in cases.items():
            if mode == 2:
                s = ctx.col_stats(2, g, b=x, mask=mask, mean=shift)
            else:
                s = ctx.col_stats(mode, x, mean=shift if mode else None)
            e0 = float(((s[0] - w0).abs() - 1e-12 * a0).max())
            e1 = float(((s[1] - w1).abs() - 1e-12 * a1).max())
            assert e0 <= 0 and e1 <= 0, (n, c, layout, mode, e0, e1)
        mean, inv = _stats(ctx, x, shift)
        var = xd.var(0, unbiased=False)
        assert _rel(mean, xd.mean(0), 1e-3 * var.sqrt().cpu() + 1e-30) <= 1e-5, (n, c, layout)
        assert _rel(inv, 1.0 / (var + 1e-5).sqrt(), torch.tensor(0.0)) <= 1e-5, (n, c, layout)
        del x, g, mask


def test_col_stats_coarser_blocks_when_scratch_is_short(ctx):
    """a caller passing less scratch than the wrapper's 4*c*max(1024, ceil(n/512)) floats gets coarser row blocks (another fixed
    summation order, here also the other partial reducer) and the same fp64 sums: direct egonn_col_stats calls with room for
    200 and 98 blocks (the default is 782); 40 is below the minimum of ceil(n/1024) blocks, and the call fails cleanly."""
    dev = ctx.device
    n, c = 100_000, 64
    x = _bn_input(n, c, 100.0, 7, dev)
    shift = torch.zeros(c, device=dev)
    xd = x.double()
    want0, want1 = xd.sum(0), (xd * xd).sum(0)
    for blocks in (200, 98, 40):
        sc = torch.empty(blocks * 2 * c * 2, device=dev)
        out = torch.empty((2, c), dtype=torch.float64, device=dev)
        rc = ctx.lib.egonn_col_stats(3, x.data_ptr(), None, None, shift.data_ptr(), n, c, out.data_ptr(), sc.data_ptr(),
                                     sc.numel(), torch.cuda.current_stream().cuda_stream)
        if blocks < (n + 1023) // 1024:
            assert rc != 0
            continue
        assert rc == 0
        assert float(((out[0] - want0).abs() - 1e-12 * xd.abs().sum(0)).max()) <= 0, blocks
        assert float(((out[1] - want1).abs() - 1e-12 * want1).max()) <= 0, blocks


BN_R = [0.0, 1.0, 10.0, 100.0, 1000.0]


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("lagged", [False, True], ids=["first-step", "lagged-shift"])
@pytest.mark.parametrize("R", BN_R)
def test_batch_norm_conditioning_matches_fp64(ctx, R, lagged, relu):
    """BatchNormFn (train mode) vs nn.BatchNorm1d in float64, with |mean|/std = R per channel plus one constant channel (var = 0:
    invstd = 1/sqrt(eps)).  The shift of the one-pass sums is the running mean: 0 on a first step, or (1 - 0.9^3) of the batch
    mean after three momentum steps.

    Forward: batch mean, invstd, running_mean, running_var within 1e-5 relative (fp64 statistics; fp32 rounding of the stored
    results is ~1e-7).  The normalised output is the folded fp32 form y = x*scale + shift with scale = gamma*invstd,
    shift = beta - mean*scale: rounding scale (2u) times |x*scale| ~ |gamma|(R + |xhat|), rounding mean*scale and beta - ... (2u R
    |gamma|), the fma (u|y|) give |(y - beta)/gamma - xhat| <= 8 (R + 1) u + 1e-6 (|xhat| <= 6 here, |beta| <= 0.3 |gamma|).

    Backward: dx = A g' + B x + C with A = gamma invstd, B = -A invstd mean(g' xhat), C = -B mean - A mean(g'), g' the ReLU-
    masked gradient.  Rounding A, B, C (u each) against |B x| ~ |A| (R + |xhat|) |mean(g' xhat)|, the two fmas, and the fp32
    mean (u R std) inside the mode-2 sum (it moves sum g'(x - mean) by u R std |sum g'|): |err| <= 8 u |A| (|g'| + |dx/A| +
    (R + 1)(1 + |xhat|)(|mean g'| + |mean g' xhat|)).  dgamma = invstd sum g'(x - mean), dbeta = sum g': fp64 sums, the fp32 mean
    and invstd: |err| <= 8 u (R + 1) sum |g'| (1 + |xhat|).  The ReLU mask is the kernel's own (y > 0): where |y| is within the
    forward bound of 0 the fp64 mask is a coin flip, and the mask decision is the forward test's business.  R is |mean| invstd
    per channel (= mean/std, except on the constant channel where the fold multiplies 0.75 by 1/sqrt(eps))."""
    from egonn_amd.train import BatchNormFn
    dev = ctx.device
    n, c = 20_000, 64
    x = _bn_input(n, c, R, 11 + int(R), dev)
    xd = x.double().cpu()
    bmean = xd.mean(0)
    bn = torch.nn.BatchNorm1d(c).to(dev)
    g = _gen(3)
    with torch.no_grad():
        bn.weight.copy_(0.8 + 0.4 * torch.rand(c, generator=g))
        bn.bias.copy_(0.3 * (torch.rand(c, generator=g) - 0.5))
        if lagged:
            bn.running_mean.copy_((1 - 0.9 ** 3) * bmean.float())
            bn.running_var.copy_(1.0 + torch.rand(c, generator=g))
            bn.num_batches_tracked.fill_(3)
    ref = torch.nn.BatchNorm1d(c).double()
    with torch.no_grad():
        ref.load_state_dict({k: v.detach().cpu() for k, v in bn.state_dict().items()})
    shift0 = bn.running_mean.clone()
    mean, inv = _stats(ctx, x, shift0)
    var = xd.var(0, unbiased=False)
    std = var.sqrt()
    e_mean, e_inv = _rel(mean, bmean, 1e-3 * std + 1e-30), _rel(inv, 1.0 / (var + 1e-5).sqrt(), torch.tensor(0.0))
    assert e_mean <= 1e-5 and e_inv <= 1e-5, ("mean / invstd relative error", e_mean, e_inv)

    xg = x.clone().requires_grad_(True)
    y = BatchNormFn.apply(xg, bn.weight, bn.bias, ctx, bn, relu, None, None)
    G = torch.randn((n, c), generator=_gen(5)).to(dev)
    (y * G).sum().backward()
    xr = xd.clone().requires_grad_(True)
    ypre = ref(xr)
    gam, bet = ref.weight.detach(), ref.bias.detach()
    Rc = bmean.abs() / (var + 1e-5).sqrt()        # R = |mean| invstd: mean/std, and 0.75/sqrt(eps) on the constant channel
    xhat = ((xd - bmean) / (var + 1e-5).sqrt())
    yc = y.detach().cpu().double()
    mask = (yc > 0).double() if relu else torch.ones_like(yc)
    fwd_bound = 8 * (Rc + 1) * U + 1e-6
    if relu:
        err = (yc - torch.relu(ypre.detach())).abs() / gam
    else:
        err = ((yc - bet) / gam - (ypre.detach() - bet) / gam).abs()
    assert float((err - fwd_bound).max()) <= 0, ("y", float(err.max()))
    # running statistics (momentum 0.1, unbiased variance) and the step counter
    assert _rel(bn.running_mean, ref.running_mean, 1e-3 * std + 1e-30) <= 1e-5, "running_mean"
    assert _rel(bn.running_var, ref.running_var, torch.tensor(0.0)) <= 1e-5, "running_var"
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == (4 if lagged else 1)

    Gd = G.double().cpu() * mask
    (ypre * Gd).sum().backward()
    A = gam / (var + 1e-5).sqrt()
    mg, mgx = Gd.mean(0), (Gd * xhat).mean(0)
    dx_bound = 8 * U * A.abs() * (Gd.abs() + (xr.grad / A).abs() + (Rc + 1) * (1 + xhat.abs()) * (mg.abs() + mgx.abs()))
    err = (xg.grad.cpu().double() - xr.grad).abs()
    assert float((err - dx_bound - 1e-30).max()) <= 0, ("dx", float(err.max()), float((err / dx_bound).max()))
    p_bound = 8 * U * (Rc + 1) * (Gd.abs() * (1 + xhat.abs())).sum(0)
    for mine, want, name in ((bn.weight.grad, ref.weight.grad, "dgamma"), (bn.bias.grad, ref.bias.grad, "dbeta")):
        err = (mine.cpu().double() - want).abs()
        assert float((err - p_bound).max()) <= 0, (name, float(err.max()), float((err / p_bound).max()))


# ====================================================================================== 2. per-sample operators (GeM / ECA)
BATCHES = {
    "single": [700],
    "one-row": [300, 1, 517],
    "empty-middle": [400, 0, 250],
    "ragged64": [int(v) for v in np.random.default_rng(64).integers(1, 160, size=64)],
}


def _ragged(counts):
    off = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    return off


def _gem_input(n, c, seed, dev):
    """a mix below, at and above the fp32 clamp 1e-6 (zeros, 3e-7, exactly fp32(1e-6), 2e-6, O(1)); channel 0 constant"""
    g = _gen(seed)
    x = torch.rand((n, c), generator=g, dtype=torch.float64) * 2.0
    pick = torch.rand((n, c), generator=g)
    x = torch.where(pick < 0.05, torch.zeros_like(x), x)
    x = torch.where((pick >= 0.05) & (pick < 0.08), torch.full_like(x, 3e-7), x)
    x = torch.where((pick >= 0.08) & (pick < 0.11), torch.full_like(x, float(np.float32(1e-6))), x)
    x = torch.where((pick >= 0.11) & (pick < 0.13), torch.full_like(x, 2e-6), x)
    x[:, 0] = 0.7
    return x.float().to(dev)


GEM_CASES = [(b, c, p) for b in BATCHES for c in (32, 64, 128, 256) for p in (1.0, 3.0, 6.5)
             if not (b == "ragged64" and c in (32, 128))]


@pytest.mark.parametrize("batch,c,p", GEM_CASES, ids=[f"{b}-{c}-p{p}" for b, c, p in GEM_CASES])
def test_gem_forward_backward_match_fp64(lib, batch, c, p):
    """GeMFn (layers/pooling.py:82-86: (mean_b clamp(x, 1e-6)^p)^(1/p)) and its gradients in x and p vs float64 autograd per
    sample.  The clamp is the fp32 constant the reference module applies to fp32 rows (torch passes the gradient at x == min).
    An empty sample pools to 0 and adds nothing to dx or dp; channel 0 is constant, where dout/dp = out (-ln(out^p)/p^2 +
    T/(p S)) is the difference of two nearly equal terms.

    Bounds: the per-sample sums are fp32 over <= L = n_max/32 + 256/C + 32 serial terms (segment kernel + 32 chunks), powf/logf
    add a few ulp per term, so mean t^p carries eps = (L + 8) u relative, out = mean^(1/p) eps/p + 2u.  dx = g out^(1-p) t^(p-1)
    / n_b: |err| <= (p + 2)(eps + 4u) |dx|.  dp = sum_b,c g dout/dp with term1 = -ln(out)/p (absolute error eps/p: the log of a
    value with relative error eps) and term2 = T/(p S) (relative eps): |err| <= 4 eps sum |g| (out (|term1| + |term2| + 1/p) +
    |dout/dp|) — absolute, scaled by the two terms, because they cancel."""
    from egonn_amd.train import GeMFn
    counts = BATCHES[batch]
    ctx = _plan_from_counts(lib, counts, seed=len(counts) + c)
    dev = ctx.device
    off = _ragged(counts)
    n = int(off[-1])
    x = _gem_input(n, c, c + int(p * 10), dev).requires_grad_(True)
    pp = torch.nn.Parameter(torch.tensor([p], device=dev))
    G = torch.randn((len(counts), c), generator=_gen(c)).to(dev)
    out = GeMFn.apply(x, pp, ctx, 0)
    (out * G).sum().backward()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(x.grad).all()), "non-finite output / dx"
    assert bool(torch.isfinite(pp.grad).all()), ("non-finite dp", float(pp.grad))

    xr = x.detach().cpu().double().requires_grad_(True)
    pr = torch.tensor([p], dtype=torch.float64, requires_grad=True)
    clampv = float(np.float32(1e-6))
    Gd = G.cpu().double()
    rows, t1s, t2s = [], [], []
    for b in range(len(counts)):
        if counts[b] == 0:
            rows.append(torch.zeros(c, dtype=torch.float64))
            t1s.append(torch.zeros(c, dtype=torch.float64))
            t2s.append(torch.zeros(c, dtype=torch.float64))
            continue
        t = xr[off[b]:off[b + 1]].clamp(min=clampv)
        o = t.pow(pr).mean(0).pow(1.0 / pr)
        rows.append(o)
        with torch.no_grad():
            td = t.detach()
            S, T = td.pow(p).sum(0), (td.pow(p) * td.log()).sum(0)
            t1s.append(-(o.detach().pow(p)).log() / p ** 2)
            t2s.append(T / (p * S))
    ref = torch.stack(rows)
    (ref * Gd).sum().backward()
    L = max(counts) / 32 + 256 / c + 32
    eps = (L + 8) * U
    outc = out.detach().cpu().double()
    err = (outc - ref.detach()).abs()
    assert float((err - (eps / p + 2 * U) * ref.detach().abs() - 1e-30).max()) <= 0, ("out", float(err.max()))
    for b in range(len(counts)):
        if counts[b] == 0:
            assert float(outc[b].abs().max()) == 0.0
    dxe = (x.grad.cpu().double() - xr.grad).abs()
    assert float((dxe - (p + 2) * (eps + 4 * U) * xr.grad.abs() - 1e-30).max()) <= 0, ("dx", float(dxe.max()))
    od = ref.detach()
    t1, t2 = torch.stack(t1s), torch.stack(t2s)
    dodp = od * (t1 + t2)
    dp_bound = float((Gd.abs() * (od * (t1.abs() + t2.abs() + 1.0 / p) + dodp.abs())).sum()) * 4 * eps
    assert abs(float(pp.grad) - float(pr.grad)) <= dp_bound + 1e-30, (float(pp.grad), float(pr.grad), dp_bound)


ECA_CASES = [(b, c) for b in BATCHES for c in (32, 64, 128, 256)] + [("b32", 256), ("b33", 256)]


@pytest.mark.parametrize("batch,c", ECA_CASES, ids=[f"{b}-{c}" for b, c in ECA_CASES])
def test_eca_tail_matches_fp64(lib, batch, c):
    """eca_tail = SegmentMeanFn -> EcaGateFn -> GateResidualFn (layers/eca_block.py:21-36,66-73: relu(x * sigmoid(Conv1d_k(mean_b
    x)) + residual)) and all its gradients (x, residual, Conv1d weight) vs float64 autograd per sample, kernel size from
    ECALayer(C).  B*C on both sides of ECA_BWD_LDS = 8192 (C = 256, B = 32 staged / B = 33 unstaged).  An empty sample has no
    rows and adds nothing to the weight gradient.

    The reference backward is taken through the kernel's own ReLU mask M = [h > 0] (where the fp64 pre-activation is within the
    forward bound of 0 the fp64 mask is a coin flip; the mask decision is the forward check's business), so g' = G M exactly.

    Bounds, per sample b and channel c (fp64 quantities of the reference; u = 2^-24).  Every per-sample, (B, C) and weight sum
    is an fp32 chain of <= L = n_max/32 + 256/C + 32 + B*C/256 + 8 terms: eps = (L + 8) u.
      mean:  |dm_b| <= eps mean_r |x|                                 (segment sums over the sample's n_b rows, / n_b)
      z = sum_j w_j m_b[c+j-pad]:  |dz| <= sum_j |w_j| |dm_b[q]| + (k+1) u sum_j |w_j m_b[q]|
      gate = sigmoid(z):  |dgate| <= |dz|/4 + 4u
      out = relu(x gate + res):  |err| <= |x| |dgate| + 2u (|x gate| + |x gate + res|)
      dgate_b = sum_r g' x over the sample's rows:  error eps A_b, A_b = sum_r |g' x|
      dz_b = dgate_b gate (1 - gate):  |e_dz| <= eps A_b / 4 + |dgate_b| (|dgate| + 3u)      (|d(g(1-g))/dg| <= 1)
      dmean_b[c] = sum_j w_j dz_b[c-j+pad]:  |e_dm| <= sum_j |w_j| |e_dz| + (k+1) u sum_j |w_j dz_b|
      dx = g' gate_b + dmean_b / n_b:  |err| <= |g'| (|dgate| + u gate) + (|e_dm| + u |dmean_b|) / n_b + u |dx|
      dres = g':  exact
      dw_j = sum_(b,c) dz_b[c] m_b[c+j-pad]:  |err| <= sum (|e_dz| |m| + |dz| |dm|) + eps sum |dz m|
    The error of dz_b carries the sample's n_b row terms and is divided by the same n_b: no count ratio enters dx."""
    from egonn_amd import train as T
    from egonn_amd.model import ECALayer
    if batch in ("b32", "b33"):
        counts = [int(v) for v in np.random.default_rng(int(batch[1:])).integers(5, 60, size=int(batch[1:]))]
        counts[7] = 0
    else:
        counts = BATCHES[batch]
    ctx = _plan_from_counts(lib, counts, seed=3 * len(counts) + c)
    dev = ctx.device
    off = _ragged(counts)
    n, B = int(off[-1]), len(counts)
    g = _gen(c + B)
    x = (torch.randn((n, c), generator=g) * 0.8 + 0.2).to(dev).requires_grad_(True)
    res = torch.randn((n, c), generator=g).to(dev).requires_grad_(True)
    eca = ECALayer(c).to(dev)
    with torch.no_grad():
        eca.conv.weight.copy_(torch.randn(eca.conv.weight.shape, generator=g) * 0.7)
    G = torch.randn((n, c), generator=g).to(dev)
    h = T.eca_tail(ctx, 0, x, res, eca)
    (h * G).sum().backward()

    idx = torch.from_numpy(np.repeat(np.arange(B), counts))
    cnt = torch.tensor(counts, dtype=torch.float64).unsqueeze(1).clamp(min=1)
    xr, rr = x.detach().cpu().double().requires_grad_(True), res.detach().cpu().double().requires_grad_(True)
    wr = eca.conv.weight.detach().cpu().double().requires_grad_(True)
    k = wr.shape[-1]
    pad = (k - 1) // 2
    m = torch.zeros((B, c), dtype=torch.float64).index_add(0, idx, xr) / cnt          # an empty sample: mean 0, no rows
    gate = torch.sigmoid(F.conv1d(m.unsqueeze(1), wr, padding=pad).squeeze(1))
    pre = xr * gate[idx] + rr
    hc = h.detach().cpu().double()
    Gm = G.cpu().double() * (hc > 0).double()                                           # g' = G M
    (pre * Gm).sum().backward()

    def shifted(a, s):                                                                  # a[:, c + s], 0 outside [0, C)
        out = torch.zeros_like(a)
        if s >= 0:
            out[:, :c - s] = a[:, s:]
        else:
            out[:, -s:] = a[:, :c + s]
        return out

    with torch.no_grad():
        w = wr.detach().reshape(-1)
        wa = w.abs()
        L = max(counts) / 32 + 256 / c + 32 + B * c / 256 + 8
        eps = (L + 8) * U
        xd, md, gt = xr.detach(), m.detach(), gate.detach()
        dm = eps * torch.zeros((B, c), dtype=torch.float64).index_add(0, idx, xd.abs()) / cnt
        dz = sum(wa[j] * shifted(dm, j - pad) + (k + 1) * U * (w[j] * shifted(md, j - pad)).abs() for j in range(k))
        dgt = dz / 4 + 4 * U
        # forward
        err = (hc - torch.relu(pre.detach())).abs()
        bound = xd.abs() * dgt[idx] + 2 * U * ((xd * gt[idx]).abs() + pre.detach().abs())
        assert float((err - bound).max()) <= 0, ("out", float(err.max()), float((err / bound).max()))
        # backward
        dgate = torch.zeros((B, c), dtype=torch.float64).index_add(0, idx, Gm * xd)
        A = torch.zeros((B, c), dtype=torch.float64).index_add(0, idx, (Gm * xd).abs())
        dzb = dgate * gt * (1 - gt)
        e_dz = eps * A / 4 + dgate.abs() * (dgt + 3 * U)
        dmean = sum(w[j] * shifted(dzb, pad - j) for j in range(k))
        e_dm = sum(wa[j] * shifted(e_dz, pad - j) + (k + 1) * U * (w[j] * shifted(dzb, pad - j)).abs() for j in range(k))
        dx_bound = Gm.abs() * (dgt[idx] + U * gt[idx]) + ((e_dm + U * dmean.abs()) / cnt)[idx] + U * xr.grad.abs()
        err = (x.grad.cpu().double() - xr.grad).abs()
        assert float((err - dx_bound).max()) <= 0, ("dx", float(err.max()), float((err / dx_bound).max()))
        assert torch.equal(res.grad.cpu().double(), rr.grad), "dres = g' exactly"
        dw_bound = torch.stack([(e_dz * shifted(md, j - pad).abs() + dzb.abs() * shifted(dm, j - pad)).sum()
                                + eps * (dzb * shifted(md, j - pad)).abs().sum() for j in range(k)])
        err = (eca.conv.weight.grad.cpu().double().reshape(-1) - wr.grad.reshape(-1)).abs()
        assert bool((err <= dw_bound).all()), ("dw", err.tolist(), dw_bound.tolist())


def test_train_step_with_empty_scan_matches_step_without_it(lib):
    """a whole EgoNN train-mode step (global and local branch) on scans [a, empty, b] gives finite gradients for all 104
    parameters, equal to the step on [a, b] within fp32 noise: BatchNorm sees the same rows, the empty sample pools to 0 and the
    loss does not read it.  Tolerance 2e-4 of each tensor's largest entry: the two plans hold the same rows in the same order,
    only per-sample launch shapes differ."""
    import egonn_amd
    from egonn_amd.synth import lidar_scan
    dev = lib.require_gpu()
    mp = egonn_amd.ModelParams(model="egonn", coordinates="cartesian", quantization_step=0.3)
    a, b = lidar_scan(71, 6000), lidar_scan(72, 7000)
    wts = H.seeded_weights(5)

    def step(scans):
        model = egonn_amd.model_factory(mp)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in wts.items()})
        model = model.to(dev).train()
        ctx = model.context()
        off = [0]
        for s in scans:
            off.append(off[-1] + len(s))
        ctx.voxelize(torch.from_numpy(np.concatenate(scans)).to(dev), off, 0, [0.3])
        coords = ctx.level_coords(0)
        y = model({"coords": coords, "features": torch.ones((len(coords), 1), device=dev), "batch_size": len(scans)})
        live = [i for i, s in enumerate(scans) if len(s)]
        gl = y["global"]
        assert torch.isfinite(gl).all()
        R = torch.from_numpy(np.random.default_rng(9).standard_normal((2, gl.shape[1])).astype(np.float32)).to(dev)
        loss = (gl[live] * R).sum()
        for i in live:
            loss = loss + y["descriptors"][i].sum() * 0.01 + y["keypoints"][i].sum() * 0.01 + y["sigma"][i].sum() * 0.01
        loss.backward()
        return {k: p.grad.detach().cpu() for k, p in model.named_parameters()}

    with_empty, without = step([a, np.zeros((0, 3), np.float32), b]), step([a, b])
    assert len(with_empty) == 104
    for k, gw in with_empty.items():
        assert gw is not None and bool(torch.isfinite(gw).all()), k
        scale = float(without[k].abs().max())
        assert float((gw - without[k]).abs().max()) <= 2e-4 * scale + 1e-12, k


# ================================================================================= 3. activations, normalize, dense weights
@pytest.mark.parametrize("act,name", [(1, "relu"), (2, "tanh"), (3, "softplus"), (4, "sigmoid")])
def test_act_backward_matches_fp64(ctx, act, name):
    """egonn_act_backward: grad_in = g * act'(x) computed from the fp32 OUTPUT y (relu [y > 0], tanh 1 - y^2, softplus 1 - exp(-y),
    sigmoid y (1 - y)), pre-activations over [-30, 30] (saturation) plus exactly 0, against the fp64 derivative of the forward
    (torch's softplus, threshold 20).  y carries u relative error, the formula one or two more roundings of values <= 1:
    |err| <= 4u |g| + 2u |ref|.  softplus' 1 - exp(-y) loses RELATIVE accuracy for very negative x (exp(-y) -> 1): the bound
    is absolute, ~2.4e-7 |g|, on purpose.  ReLU is exact, with zero gradient at x = 0."""
    dev = ctx.device
    xs = torch.cat([torch.linspace(-30, 30, 60001, dtype=torch.float64), torch.zeros(7, dtype=torch.float64),
                    torch.tensor([-1e-30, 1e-30, -1e-7, 1e-7], dtype=torch.float64)])
    n = xs.numel() // 7 * 7
    xs = xs[:n].reshape(-1, 7)
    x = xs.clone().requires_grad_(True)
    fwd = {1: torch.relu, 2: torch.tanh, 3: F.softplus, 4: torch.sigmoid}[act]
    y = fwd(x)
    G = torch.randn(xs.shape, generator=_gen(act), dtype=torch.float64)
    (y * G).sum().backward()
    got = ctx.act_backward(act, G.float().to(dev), y.detach().float().to(dev).contiguous()).cpu().double()
    Gf = G.float().double()
    ref = (x.grad / G) * Gf                       # act'(x) (exactly 0 / 1 for ReLU) times the fp32 gradient
    err = (got - ref).abs()
    if act == 1:
        assert torch.equal(got, ref), name
        assert float(got[xs == 0].abs().max()) == 0.0
    else:
        assert float((err - 4 * U * Gf.abs() - 2 * U * ref.abs()).max()) <= 0, (name, float(err.max()))


@pytest.mark.parametrize("c", [3, 64, 128, 256])
def test_l2_normalize_matches_fp64(ctx, c):
    """egonn_l2_normalize forward / backward = F.normalize(x, dim=1, eps=1e-12): y = x / max(|x|, eps); rows of norm ~1, 3e-12,
    1.5e-12, 0.7e-12 and 1e-14 (below eps: y = x/eps, dx = g/eps) and an all-zero row.  The squared norm is an fp32 chain of
    c/64 + 6 terms (lane sums + shuffle tree), so |x| carries k = (c/64 + 8) u: |dy| <= 2k |y|; the backward's g - y (g.y)
    cancels: |err| <= 4k (|g| + |y| sum|g y|) / max(|x|, eps)."""
    dev = ctx.device
    g = _gen(c)
    base = torch.randn((64, c), generator=g, dtype=torch.float64)
    base = base / base.norm(dim=1, keepdim=True)
    scales = torch.tensor([1.0, 3.7, 0.2, 3e-12, 1.5e-12, 0.7e-12, 1e-14, 0.0] * 8, dtype=torch.float64).unsqueeze(1)
    x = (base * scales).float().double()
    xr = x.clone().requires_grad_(True)
    yr = F.normalize(xr, dim=1, eps=1e-12)
    G = torch.randn((64, c), generator=g, dtype=torch.float64).float().double()
    (yr * G).sum().backward()
    xg = x.float().to(dev)
    y = ctx.l2_normalize(xg).cpu().double()
    dx = ctx.l2_normalize(xg, G.float().to(dev)).cpu().double()
    k = (c / 64 + 8) * U
    ya = yr.detach().abs()
    assert float(((y - yr.detach()).abs() - 2 * k * ya - 1e-30).max()) <= 0
    nrm = x.norm(dim=1, keepdim=True).clamp_min(1e-12)
    bound = 4 * k * (G.abs() + ya * (G * yr.detach()).abs().sum(1, keepdim=True)) / nrm
    err = (dx - xr.grad).abs()
    assert float((err - bound - 1e-30).max()) <= 0, float((err / bound).max())
    assert torch.isfinite(dx).all()


DW_CASES = [(1, 128), (3, 128), (32, 64), (64, 128), (128, 128), (256, 256), (128, 32)]


@pytest.mark.parametrize("ca,cb", DW_CASES, ids=[f"{a}x{b}" for a, b in DW_CASES])
def test_dense_weight_and_bias_gradient_match_fp64(ctx, ca, cb):
    """egonn_dense_backward_weight (dW = g^T x of a MinkowskiLinear) and the bias gradient col_stats(0, g)[0] (C = 1 and 3: the
    sigma and keypoint heads) for n in {1, 37, 8191, 8193, 33000}, against fp64.  The bound shape of
    test_dense_every_kernel_path_matches_fp64: |err| <= 2e-5 sum |terms| + 1e-6 (fp32 sums: the bias sums are fp64 now, well
    inside it)."""
    dev = ctx.device
    for n in (1, 37, 8191, 8193, 33000):
        g = torch.randn((n, ca), generator=_gen(n + ca)).to(dev)
        x = torch.randn((n, cb), generator=_gen(n + cb + 1)).to(dev)
        dw = ctx.dense_backward_weight(g, x).cpu().double()
        gd, xd = g.cpu().double(), x.cpu().double()
        want = gd.t() @ xd
        bound = 2e-5 * (gd.abs().t() @ xd.abs()) + 1e-6
        assert float(((dw - want).abs() - bound).max()) <= 0, (n, ca, cb)
        db = ctx.col_stats(0, g)[0].float().cpu().double()
        assert float(((db - gd.sum(0)).abs() - 2e-5 * gd.abs().sum(0) - 1e-6).max()) <= 0, (n, ca)


# ========================================================================================= 4. sparse-conv backward, element-wise
class _HostPlan:
    def __init__(self, lib, scans, step):
        from oracle import egonn_ref as ref
        dev = lib.require_gpu()
        self.ctx = lib.Context(dev, coord_bits=12)
        off = [0]
        for s in scans:
            off.append(off[-1] + len(s))
        self.ctx.voxelize(torch.from_numpy(np.concatenate(scans)).to(dev), off, 0, [step])
        self.lv = ref.SparseLevels(self.ctx.level_coords(0).cpu().numpy())
        self._perm = {}

    def perm(self, level):
        """gpu_rows[perm] == host_rows"""
        if level not in self._perm:
            self._perm[level] = H.join_perm(self.ctx.level_coords(level).cpu().numpy(), self.lv.coords[level])
        return self._perm[level]

    def pairs(self, ks, tr, lin, lout):
        """[(j_in, o_out)] per kernel offset, in GPU row numbers, of the forward convolution"""
        if ks == 1:
            r = np.arange(self.ctx.level_count(lin))
            return [(r, r)]
        if ks == 3:
            maps = self.lv.kmap(lin, lin, 3)
        elif not tr:
            maps = self.lv.kmap(lin, lout, 2)
        else:
            maps = [(o, j) for j, o in self.lv.kmap(lout, lin, 2)]
        pi, po = self.perm(lin), self.perm(lout)
        return [(pi[j], po[o]) for j, o in maps]


def _conv_plans(lib):
    from egonn_amd.synth import lidar_scan
    return {"two-scans+empty": _HostPlan(lib, [lidar_scan(81, 2500), np.zeros((0, 3), np.float32), lidar_scan(82, 2000)], 0.2),
            "tiny": _HostPlan(lib, [lidar_scan(83, 400)[:90]], 0.2)}


@pytest.fixture(scope="module")
def conv_plans(lib):
    return _conv_plans(lib)


from tests.test_gpu_train import CONV_CASES  # noqa: E402  (every case of the adjoint tests, here element by element)


@pytest.mark.parametrize("plan_name", ["two-scans+empty", "tiny"])
@pytest.mark.parametrize("ks,tr,lin,lout,cin,cout", CONV_CASES)
def test_conv_backward_elementwise_matches_fp64(conv_plans, plan_name, ks, tr, lin, lout, cin, cout):
    """SparseConvFn backward element by element against a host fp64 loop over the kernel maps of the forward:
    dW[k] = sum over pairs (j, o) of x[j]^T G[o],  dX[j] += G[o] W[k]^T.  dW is exact fp32 (fp32 products, fp32 + fp64 sums):
    |err| <= 2e-5 sum |x[j]| |G[o]|.  dX runs on the fp16-split pipe with operand autoscale (k = 2, 3) or the dense kernel
    (k = 1): the bound of the split forward tests, max |err| <= 3e-6 max |dX| (tests/test_gpu_range_edges.py)."""
    from egonn_amd.train import SparseConvFn
    P = conv_plans[plan_name]
    ctx, dev = P.ctx, P.ctx.device
    n_in, n_out = ctx.level_count(lin), ctx.level_count(lout)
    if n_in == 0 or n_out == 0:
        pytest.skip("level empty on this plan")     # never for the plans above (asserted below)
    kshape = (cin, cout) if ks == 1 else (ks ** 3, cin, cout)
    g = _gen(ks * 100 + lin * 10 + lout + cin)
    x = torch.randn((n_in, cin), generator=g).to(dev).requires_grad_(True)
    W = (torch.randn(kshape, generator=g) * 0.1).to(dev).requires_grad_(True)
    G = torch.randn((n_out, cout), generator=g).to(dev)
    y = SparseConvFn.apply(x, W, ctx, lin, lout, ks, tr)
    (y * G).sum().backward()
    xd, Wd, Gd = x.detach().cpu().double().numpy(), W.detach().cpu().double().numpy(), G.cpu().double().numpy()
    Wk = Wd.reshape(1, cin, cout) if ks == 1 else Wd
    dW = np.zeros_like(Wk)
    dWa = np.zeros_like(Wk)
    dX = np.zeros_like(xd)
    for k, (j, o) in enumerate(P.pairs(ks, tr, lin, lout)):
        if len(j):
            dW[k] = xd[j].T @ Gd[o]
            dWa[k] = np.abs(xd[j]).T @ np.abs(Gd[o])
            np.add.at(dX, j, Gd[o] @ Wk[k].T)
    gotW = W.grad.cpu().double().numpy().reshape(dW.shape)
    assert float((np.abs(gotW - dW) - 2e-5 * dWa).max()) <= 0, ("dW", float(np.abs(gotW - dW).max()))
    gotX = x.grad.cpu().double().numpy()
    assert float(np.abs(gotX - dX).max()) <= 3e-6 * float(np.abs(dX).max()), ("dX", float(np.abs(gotX - dX).max()))


def test_conv_plans_cover_the_edges(conv_plans):
    """the element-wise conv tests run where they are meant to: an empty scan inside the batch, a plan below one 128-row tile,
    and no level of CONV_CASES empty"""
    a, t = conv_plans["two-scans+empty"].ctx, conv_plans["tiny"].ctx
    off = a.level_batch_offsets(0)
    assert off[2] - off[1] == 0 and off[1] > 0 and off[3] > off[2]
    assert 0 < t.level_count(0) < 128
    for c in (a, t):
        assert all(c.level_count(l) > 0 for l in range(6))

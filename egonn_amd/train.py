"""Training-mode EgoNN graph on the MI355X operators (BASELINE configs[3]: the sharded training step).

The reference trains through MinkowskiEngine's autograd (training/trainer.py:160-175: `model.train()`,
`y = model(batch)`, `loss.backward()`, `optimizer.step()`).  Here `MinkGL.forward` in train mode builds the same
graph (models/minkgl.py:136-153 trunk, layers/eca_block.py:56-73 block, models/minkgl.py:46-60 head,
:207-225 decoder, layers/pooling.py:82-86 GeM) out of `torch.autograd.Function`s whose forward AND backward are
libegonn_hip kernels; PyTorch only owns the tensors, the tape and the optimiser.  Vectors of C or (B, C) values
(batch-norm statistics, the ECA gate's Conv1d over channels, GeM's exponent) are combined with tiny tensor ops.

BatchNorm uses the statistics of ALL rows of the batch (`nn.BatchNorm1d` on SparseTensor.F); with a process group
the per-channel sums are all-reduced (SyncBN) so that a sharded batch reproduces the single-GPU
statistics.  There is no CPU path: every Function needs the HIP library.

Both branches are differentiable: the global one (trunk + global head + decoder + GeM) for the batch-hard triplet
loss of models/loss.py, the local one (local head, descriptor decoder + L2 norm, keypoint regressor + tanh + the
quantiser's keypoint_position, sigma regressor + softplus) so that the reference's own local losses
(models/loss_utils.py, plain torch code on the output lists) can back-propagate into it.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch
from torch.autograd import Function

from . import _lib, graph

ACT_NONE, ACT_RELU, ACT_TANH, ACT_SOFTPLUS = 0, 1, 2, 3


def _c(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous() else t.contiguous()


# ----------------------------------------------------------------------------- sparse convolution
class SparseConvFn(Function):
    """ME.MinkowskiConvolution / MinkowskiConvolutionTranspose on the cached maps of the current plan."""

    @staticmethod
    def forward(fctx, x, kernel, ctx: _lib.Context, level_in: int, level_out: int, ks: int, transposed: bool):
        k = _c(kernel.detach())
        if transposed:
            out = ctx.conv_transpose(level_in, x, k)
        else:
            out = ctx.conv(level_in, level_out, ks, x, k)
        fctx.save_for_backward(x, kernel)
        fctx.meta = (ctx, level_in, level_out, ks, transposed)
        return out

    @staticmethod
    def backward(fctx, g):
        x, kernel = fctx.saved_tensors
        ctx, lin, lout, ks, transposed = fctx.meta
        g = _c(g)
        k = kernel.detach()
        dx = dk = None
        if x is not None and fctx.needs_input_grad[0]:
            if ks == 1:                                   # dX = dY @ W^T, W (cin, cout) read as an (out=cin, in=cout) matrix
                dx = ctx.dense(g, _c(k), out_in=True)
            elif ks in (2, 3):
                # The input-gradient convolutions run on the fp16-split kernels like the forward ones, and gradients are SMALL
                # (1e-6 .. 1e-8 is ordinary): an fp16 part flushes below 2^-25 and carries 2^-25 absolute error below 2^-14.  The
                # library therefore scales this operand by a power of two per launch (max |g| -> [2^13, 2^14), exact, undone in
                # the epilogue: egonn_ctx_set_operand_autoscale) — the treatment the kernels give their weights.
                ctx.set_operand_autoscale(True)
                try:
                    if ks == 3:                           # nbr[o][k] = j  <=>  nbr[j][26-k] = o
                        dx = ctx.conv(lin, lin, 3, g, _c(k.flip(0).transpose(1, 2)))
                    elif not transposed:                  # strided conv  <->  transposed conv on the same map
                        dx = ctx.conv_transpose(lout, g, _c(k.transpose(1, 2)))
                    else:
                        dx = ctx.conv(lout, lin, 2, g, _c(k.transpose(1, 2)))
                finally:
                    ctx.set_operand_autoscale(False)
            else:
                raise NotImplementedError(f"input gradient of a k={ks} convolution")
        if fctx.needs_input_grad[1]:
            dk = ctx.conv_backward_weight(lin, lout, ks, transposed, x, g, tuple(kernel.shape))
        return dx, dk, None, None, None, None, None


def sparse_conv(ctx, x, conv_module, level_in, level_out):
    return SparseConvFn.apply(x, conv_module.kernel, ctx, level_in, level_out, conv_module.kernel_size,
                              bool(conv_module.transpose))


# ----------------------------------------------------------------------------- batch norm (batch statistics)
def _all_reduce(t: torch.Tensor, group):
    if group is not None:
        from .distributed import all_reduce_sum
        all_reduce_sum(t, group)
    return t


def combine_batch_stats(sum_x: torch.Tensor, count: torch.Tensor, group=None):
    """(sum, count) of this rank -> global (mean, total count); one all-reduce of C+1 values."""
    buf = torch.cat([sum_x.double(), count.double().reshape(1)])
    _all_reduce(buf, group)
    total = buf[-1]
    return (buf[:-1] / total).float(), total


def level_totals(ctx: _lib.Context, group=None) -> List[float]:
    """rows of every level summed over the ranks of `group` (the N of the whole-batch BatchNorm statistics):
    one all-reduce of 8 values per step."""
    counts = [float(ctx.level_count(l)) for l in range(8)]
    if group is None:
        return counts
    t = torch.tensor(counts, dtype=torch.float64, device=ctx.device)
    _all_reduce(t, group)
    return t.tolist()


BN_MAX_COLUMNS = 256       # egonn_col_stats: 1..256 channels


class BatchNormFn(Function):
    """nn.BatchNorm1d over all rows in train mode (MinkowskiBatchNorm), optional fused ReLU, optional SyncBN.
    Statistics: ONE pass of shifted sums (sum d, sum d^2 with d = x - running_mean: additive over ranks), formed and kept
    in fp64 ((2, C) doubles through the all-reduce and both finalize kernels): the shift is 0 on a first step and lags the
    batch mean after it, and var = S2/n - (S1/n)^2 loses (mean/std)^2 of the sums' relative precision, which fp32 sums
    could not afford.  All-reduced when `group` is given; the per-channel
    bookkeeping (mean, invstd, folded scale/shift, running statistics; A/B/C, dgamma, dbeta in backward) runs in one
    small kernel each."""

    @staticmethod
    def forward(fctx, x, weight, bias, ctx: _lib.Context, bn: torch.nn.BatchNorm1d, relu: bool, group, total):
        n, c = x.shape
        track = bn.track_running_stats and bn.running_mean is not None
        shift_pt = bn.running_mean if track else torch.zeros(c, dtype=torch.float32, device=x.device)
        s = ctx.col_stats(3, x, mean=shift_pt)
        _all_reduce(s, group)
        total = float(total if total is not None else n)
        if track:
            mom = bn.momentum if bn.momentum is not None else 1.0 / float(int(bn.num_batches_tracked) + 1)
        else:
            mom = 0.0
        out4 = ctx.bn_train_finalize(s, shift_pt, total, weight, bias, bn.eps, mom, bn.running_mean if track else None,
                                     bn.running_var if track else None)
        if track:
            bn.num_batches_tracked += 1
        y = ctx.affine_act(x, out4[2], out4[3], relu)
        fctx.save_for_backward(x, y if relu else None, out4, weight)
        fctx.meta = (ctx, group, total)
        return y

    @staticmethod
    def backward(fctx, g):
        x, y, out4, weight = fctx.saved_tensors
        ctx, group, total = fctx.meta
        g = _c(g)
        s = ctx.col_stats(2, g, b=x, mask=y, mean=out4[0])          # sum g', sum g' (x - mean)   (this rank's rows)
        sg = s
        if group is not None:
            sg = _all_reduce(s.clone(), group)                      # whole-batch sums for the input gradient
        out5 = ctx.bn_backward_finalize(s, sg, total, weight, out4[0], out4[1])
        dx = ctx.affine3(g, y, x, out5[0], out5[1], out5[2])
        return dx, out5[3], out5[4], None, None, None, None, None


def batch_norm(ctx, x, bn_module, relu: bool, group=None, total=None):
    bn = bn_module.bn
    return BatchNormFn.apply(x, bn.weight, bn.bias, ctx, bn, relu, group, total)


# ----------------------------------------------------------------------------- per-sample pooling / ECA tail
class SegmentMeanFn(Function):
    """ME.MinkowskiGlobalPooling (per-sample mean of the rows) -> (B, C)."""

    @staticmethod
    def forward(fctx, x, ctx: _lib.Context, level: int):
        fctx.meta = (ctx, level)
        return ctx.global_avg_pool(level, x)

    @staticmethod
    def backward(fctx, g):
        ctx, level = fctx.meta
        return ctx.segment_broadcast(level, _c(g), mean=True), None, None


class GateResidualFn(Function):
    """relu(x * gate[sample] + residual): MinkowskiBroadcastMultiplication + `out += residual` + MinkowskiReLU."""

    @staticmethod
    def forward(fctx, x, gate, residual, ctx: _lib.Context, level: int):
        """gate None: plain ME BasicBlock tail relu(x + residual)."""
        out = ctx.gate_residual(level, x, None if gate is None else _c(gate.detach()), residual, relu=True)
        fctx.save_for_backward(x, gate, out)
        fctx.meta = (ctx, level)
        return out

    @staticmethod
    def backward(fctx, g):
        x, gate, out = fctx.saved_tensors
        ctx, level = fctx.meta
        g = _c(g)
        dx, dres = ctx.gate_residual_backward(level, g, out, None if gate is None else _c(gate.detach()),
                                              want_residual=fctx.needs_input_grad[2])
        dgate = ctx.segment_sums(level, 2, g, b=out, x2=x) if gate is not None and fctx.needs_input_grad[1] else None
        return dx, dgate, dres, None, None


class EcaGateFn(Function):
    """sigmoid(Conv1d_k(mean)) over the channel axis of the (B, C) per-sample means (layers/eca_block.py:28-31)."""

    @staticmethod
    def forward(fctx, mean, weight, ctx: _lib.Context):
        gate = ctx.eca_gate(mean, _c(weight.detach().reshape(-1)))
        fctx.save_for_backward(mean, weight, gate)
        fctx.meta = ctx
        return gate

    @staticmethod
    def backward(fctx, g):
        mean, weight, gate = fctx.saved_tensors
        ctx = fctx.meta
        dmean, dw = ctx.eca_gate_backward(_c(g), gate, mean, _c(weight.detach().reshape(-1)))
        return dmean, dw.reshape(weight.shape), None


def eca_tail(ctx, level, x, residual, eca_module):
    """layers/eca_block.py:21-36,66-73: gate = sigmoid(Conv1d_k(mean_b(x))), out = relu(x * gate + residual)."""
    m = SegmentMeanFn.apply(x, ctx, level)                                       # (B, C)
    gate = EcaGateFn.apply(m, eca_module.conv.weight, ctx)                       # fixed-order sums: deterministic
    return GateResidualFn.apply(x, gate, residual, ctx, level)


class SeGateFn(Function):
    """sigmoid(W2 relu(W1 mean + b1) + b2) on the (B, C) per-sample means (SELayer.fc, layers/senet_block.py:39-43,49):
    egonn_se_gate / egonn_se_gate_backward, one launch each.  The parameter gradients are serial sums over the samples in
    order, so two runs agree bitwise."""

    @staticmethod
    def forward(fctx, mean, w1, b1, w2, b2, ctx: _lib.Context):
        mean = _c(mean)
        assert all(t.is_contiguous() and t.dtype == torch.float32 for t in (w1, b1, w2, b2))
        gate, hid = ctx.se_gate(mean, w1, b1, w2, b2, want_hidden=True)
        fctx.save_for_backward(mean, w1, w2, gate, hid)
        fctx.meta = ctx
        return gate

    @staticmethod
    def backward(fctx, g):
        mean, w1, w2, gate, hid = fctx.saved_tensors
        return (*fctx.meta.se_gate_backward(_c(g), gate, hid, mean, w1, w2), None)


def se_tail(ctx, level, x, residual, se_module):
    """layers/senet_block.py:47-50,81-87: gate = sigmoid(fc(mean_b(x))), out = relu(x * gate + residual).  The gate is a
    function of ONE sample's rows, which one rank holds whole, so under a SyncBN process group it needs no collective; the
    gradients of the four fc tensors are summed over the ranks with every other parameter's (all_reduce_gradients)."""
    m = SegmentMeanFn.apply(x, ctx, level)                                       # (B, C)
    gate = SeGateFn.apply(m, *se_module.tensors(), ctx)
    return GateResidualFn.apply(x, gate, residual, ctx, level)


class AddFn(Function):
    @staticmethod
    def forward(fctx, a, b, ctx: _lib.Context):
        return ctx.add(a, b)

    @staticmethod
    def backward(fctx, g):
        return g, g, None


# ----------------------------------------------------------------------------- dense layers / GeM
class LinearFn(Function):
    """ME.MinkowskiLinear (+ fused MinkowskiReLU / Tanh / Softplus): act(rows @ W^T + b), W (out, in).
    `act`: True/False (ReLU or none) or an ACT_* code."""

    @staticmethod
    def forward(fctx, x, weight, bias, ctx: _lib.Context, act):
        act = int(act)
        y = ctx.dense(x, _c(weight.detach()), out_in=True, bias=None if bias is None else _c(bias.detach()), act=act)
        fctx.save_for_backward(x, weight, y if act else None)
        fctx.meta = (ctx, act, bias is not None)
        return y

    @staticmethod
    def backward(fctx, g):
        x, weight, y = fctx.saved_tensors
        ctx, act, has_bias = fctx.meta
        g = _c(g)
        if act:
            g = ctx.act_backward(act, g, y)
        dx = ctx.dense(g, _c(weight.detach()), out_in=False) if fctx.needs_input_grad[0] else None
        dw = ctx.dense_backward_weight(g, x) if fctx.needs_input_grad[1] else None
        db = ctx.col_stats(0, g)[0].float() if has_bias and fctx.needs_input_grad[2] else None
        return dx, dw, db, None, None


class L2NormalizeFn(Function):
    """ME.MinkowskiFunctional.normalize (F.normalize over the channels of every row)."""

    @staticmethod
    def forward(fctx, x, ctx: _lib.Context):
        fctx.save_for_backward(x)
        fctx.meta = ctx
        return ctx.l2_normalize(x)

    @staticmethod
    def backward(fctx, g):
        (x,) = fctx.saved_tensors
        return fctx.meta.l2_normalize(x, _c(g)), None


class GeMFn(Function):
    """layers/pooling.py:82-86: (mean_b clamp(x, 1e-6)^p)^(1/p)."""

    @staticmethod
    def forward(fctx, x, p, ctx: _lib.Context, level: int):
        out = ctx.gem(level, x, p)
        fctx.save_for_backward(x, p, out)
        fctx.meta = (ctx, level)
        return out

    @staticmethod
    def backward(fctx, g):
        x, p, out = fctx.saved_tensors
        ctx, level = fctx.meta
        off = ctx.level_batch_offsets(level)
        cnt = torch.tensor([off[b + 1] - off[b] for b in range(ctx.batch_size)], dtype=torch.float32,
                           device=x.device).clamp_(min=1).unsqueeze(1)
        pv = p.detach().reshape(()).float()
        g = _c(g)
        dx = dp = None
        if fctx.needs_input_grad[0]:
            # an empty sample has out = 0: its coefficient is 0, not 0 * inf
            coef = torch.where(out > 0, g * out.clamp_min(1e-30).pow(1.0 - pv) / cnt, torch.zeros_like(out))
            dx = ctx.gem_backward(level, x, _c(coef), _c(p.detach().reshape(-1).float()))
        if fctx.needs_input_grad[1]:
            T = ctx.segment_sums(level, 1, x, p=_c(p.detach().reshape(-1).float()))    # sum_r t^p ln t
            S = out.pow(pv) * cnt                                                       # sum_r t^p
            # dout/dp = out/p (T/S - ln out): ln(out) directly, not ln(out^p)/p, which is -inf once out^p underflows (out near
            # the 1e-6 clamp with p > 6.3).  An empty sample (out = 0, S = 0) pools to a constant 0 and contributes nothing:
            # 0 * (inf + nan) would be NaN for the whole batch.
            live = out > 0
            dout_dp = torch.where(live, out / pv * (T / S - torch.log(out.clamp_min(1e-30))), torch.zeros_like(out))
            dp = (g * dout_dp).sum().reshape(p.shape)
        return dx, dp, None, None


# ----------------------------------------------------------------------------- MAC / NetVLAD pooling (layers/pooling.py)
class GlobalMaxFn(Function):
    """ME.MinkowskiGlobalMaxPooling (MAC, layers/pooling.py:46-56) -> (B, C); the gradient of (b, c) goes to the one plan
    row that holds the maximum (ties: the lowest row; an empty scan gets none)."""

    @staticmethod
    def forward(fctx, x, ctx: _lib.Context, level: int):
        out, rows = ctx.global_max_pool_argmax(level, _c(x))
        fctx.save_for_backward(rows)
        fctx.meta = (ctx, level)
        return out

    @staticmethod
    def backward(fctx, g):
        (rows,) = fctx.saved_tensors
        ctx, level = fctx.meta
        return ctx.global_max_pool_backward(level, _c(g), rows), None, None


class MatmulFn(Function):
    """rows @ W with W (in, out): GatingContext's gating_weights (layers/netvlad.py:101)."""

    @staticmethod
    def forward(fctx, x, weight, ctx: _lib.Context):
        fctx.save_for_backward(x, weight)
        fctx.meta = ctx
        return ctx.dense(x, _c(weight.detach()), out_in=False)

    @staticmethod
    def backward(fctx, g):
        x, weight = fctx.saved_tensors
        ctx = fctx.meta
        g = _c(g)
        dx = ctx.dense(g, _c(weight.detach()), out_in=True) if fctx.needs_input_grad[0] else None     # g @ W^T
        dw = ctx.dense_backward_weight(x, g) if fctx.needs_input_grad[1] else None
        return dx, dw, None


class SigmoidGateFn(Function):
    """y * sigmoid(t) (GatingContext, layers/netvlad.py:108-110)."""

    @staticmethod
    def forward(fctx, y, t, ctx: _lib.Context):
        fctx.save_for_backward(y, t)
        fctx.meta = ctx
        return ctx.sigmoid_gate(y, t)

    @staticmethod
    def backward(fctx, g):
        y, t = fctx.saved_tensors
        dy, dt = fctx.meta.sigmoid_gate(y, t, _c(g))
        return dy, dt, None


class NetVLADFn(Function):
    """The row part of NetVLADLoupe.forward in train mode (layers/netvlad.py:44-73 under NetVLADWrapper's zero padding to the
    largest scan): bn1 on the statistics of all B * Nmax rows (pad rows included), soft assignment, aggregation, the two
    normalisations and the projection: (B, D) before bn2.  Forward and backward are egonn_netvlad_train_forward /
    _backward; Nmax comes from the host offsets of the plan."""

    @staticmethod
    def forward(fctx, x, cluster_weights, cluster_weights2, bn1_weight, bn1_bias, hidden1_weights, ctx: _lib.Context,
                level: int, bn1: torch.nn.BatchNorm1d):
        off = ctx.level_batch_offsets(level)
        nmax = max(off[b + 1] - off[b] for b in range(ctx.batch_size))
        x = _c(x)
        y, saved = ctx.netvlad_train_forward(level, x, nmax, cluster_weights, cluster_weights2, bn1, hidden1_weights)
        bn1.num_batches_tracked += 1
        fctx.save_for_backward(x, cluster_weights, cluster_weights2, bn1_weight, hidden1_weights, *saved)
        fctx.meta = (ctx, level, nmax)
        return y

    @staticmethod
    def backward(fctx, g):
        x, wc, w2, g1, H, *saved = fctx.saved_tensors
        ctx, level, nmax = fctx.meta
        dx, dwc, dw2, dg1, db1, dH = ctx.netvlad_train_backward(level, x, nmax, wc, w2, g1, H, _c(g), saved)
        return dx, dwc, dw2.reshape(w2.shape), dg1, db1, dH, None, None, None


def netvlad_pool(ctx, level: int, x: torch.Tensor, nv, group=None) -> torch.Tensor:
    """NetVLADLoupe (+ GatingContext) in train mode over the rows of `level`: NetVLADFn, then bn2 and the gating on the
    (B, D) descriptors through the differentiable row operators (batch statistics over the B descriptors)."""
    if group is not None:
        raise NotImplementedError("NetVLAD pooling with a SyncBN process group: Nmax and the B-row statistics would have to "
                                  "span the ranks")
    if ctx.batch_size < 2:            # nn.BatchNorm1d's own rule for bn2, before any device work
        raise ValueError(f"Expected more than 1 value per channel when training, got input size "
                         f"torch.Size([{ctx.batch_size}, {nv.output_dim}])")
    if nv.output_dim > BN_MAX_COLUMNS:
        # bn2 and the gating's BatchNorm would refuse only after NetVLADFn had stepped bn1's running statistics
        raise _lib.EgonnError(f"netvlad_pool: output_dim {nv.output_dim} unsupported in train mode (BatchNormFn holds at most "
                              f"{BN_MAX_COLUMNS} columns)", 1)
    for w in (nv.cluster_weights, nv.cluster_weights2, nv.hidden1_weights):
        assert w.is_contiguous() and w.dtype == torch.float32
    y = NetVLADFn.apply(x, nv.cluster_weights, nv.cluster_weights2, nv.bn1.weight, nv.bn1.bias, nv.hidden1_weights, ctx, level,
                        nv.bn1)
    y = BatchNormFn.apply(y, nv.bn2.weight, nv.bn2.bias, ctx, nv.bn2, False, None, None)
    if nv.gating:
        cg = nv.context_gating
        t = MatmulFn.apply(y, cg.gating_weights, ctx)
        t = BatchNormFn.apply(t, cg.bn1.weight, cg.bn1.bias, ctx, cg.bn1, False, None, None)
        y = SigmoidGateFn.apply(y, t, ctx)
    return y


class TrainOps:
    """train mode: the op set of graph.py on the differentiable operators.  `totals`: level_totals of the plan, the N of every
    BatchNorm (needed by conv_bn only)."""

    def __init__(self, ctx: _lib.Context, group=None, totals: Optional[List[float]] = None):
        self.ctx, self.group, self.totals = ctx, group, totals

    def conv_bn(self, level_in, level_out, x, conv, bn, relu):
        y = sparse_conv(self.ctx, x, conv, level_in, level_out)
        return batch_norm(self.ctx, y, bn, relu, self.group, self.totals[level_out])

    def conv(self, level_in, level_out, x, conv):
        return sparse_conv(self.ctx, x, conv, level_in, level_out)

    def tail(self, level, t, residual, block):
        if hasattr(block, 'eca'):
            return eca_tail(self.ctx, level, t, residual, block.eca)
        if hasattr(block, 'se'):
            return se_tail(self.ctx, level, t, residual, block.se)
        return GateResidualFn.apply(t, None, residual, self.ctx, level)

    def add(self, a, b):
        return AddFn.apply(a, b, self.ctx)

    def gem(self, level, x, p):
        return GeMFn.apply(x, p, self.ctx, level)

    def max_pool(self, level, x):
        return GlobalMaxFn.apply(x, self.ctx, level)

    def avg_pool(self, level, x):
        return SegmentMeanFn.apply(x, self.ctx, level)

    def netvlad(self, level, x, wrapper):
        return netvlad_pool(self.ctx, level, x, wrapper.net_vlad, self.group)


def pool(ctx, level: int, x: torch.Tensor, pooling, method: str, group=None) -> torch.Tensor:
    """PoolingWrapper.forward in train mode (layers/pooling.py:13-43): `pooling` is the GeM / MAC / SPoC / NetVLADWrapper
    module, `method` its name."""
    return graph.pool(TrainOps(ctx, group), level, x, pooling, method)


# ----------------------------------------------------------------------------- the graph
def trunk_forward(model, ctx, group=None) -> Dict[int, torch.Tensor]:
    """MinkTrunk.forward (reference models/minkgl.py:136-153) with all-ones input features."""
    t = model.trunk
    ops = TrainOps(ctx, group, level_totals(ctx, group))
    x = ops.conv_bn(0, 0, None, t.convs['0'], t.bn['0'], True)
    levels = {}
    for i in range(1, len(t.planes) + 1):
        x = ops.conv_bn(i - 1, i, x, t.convs[str(i)], t.bn[str(i)], True)
        for blk in t.blocks[str(i)]:
            x = graph.residual_block(ops, i, x, blk)
        levels[i] = x
    return levels


def head_forward(head, ctx, levels: Dict[int, torch.Tensor]):
    """MinkHead.forward (reference models/minkgl.py:46-60)."""
    ops, top = TrainOps(ctx), head.max_level
    y = ops.conv(top, top, levels[top], head.conv1x1[str(top)])
    return graph.top_down(ops, top, y, [(head.tconv[str(l + 1)],) + ((levels[l], head.conv1x1[str(l)]) if l in head.in_levels
                                                                     else (None, None))
                                        for l in range(top - 1, head.min_level - 1, -1)])


def global_branch(model, ctx, group=None, levels=None) -> torch.Tensor:
    """trunk -> global head -> descriptor decoder -> GeM / MAC / SPoC  (reference models/minkgl.py:269-287)."""
    if levels is None:
        levels = trunk_forward(model, ctx, group)
    lvl, x = head_forward(model.global_head, ctx, levels)
    net = model.global_descriptor_decoder.net
    x = LinearFn.apply(x, net[0].linear.weight, net[0].linear.bias, ctx, True)
    x = LinearFn.apply(x, net[2].linear.weight, net[2].linear.bias, ctx, False)
    return pool(ctx, lvl, x, model.global_pooling.pooling, getattr(model, "global_pool_method", "GeM"), group)


def minkfpn_forward(fpn, ctx, group=None):
    """MinkFPN.forward in train mode (all-ones input features): graph.minkfpn on the differentiable operators."""
    assert fpn.conv0.kernel_size == 5 and fpn.conv0.kernel.shape[1] == 1, "train mode: k=5, 1-channel input layer"
    return graph.minkfpn(TrainOps(ctx, group, level_totals(ctx, group)), fpn, None)


def local_branch(model, ctx, levels: Dict[int, torch.Tensor]):
    """local head -> descriptor decoder (+L2 norm), keypoint regressor (+tanh), sigma regressor (+softplus)
    (reference models/minkgl.py:289-308).  Returns (level, descriptors, keypoint offsets, sigma), rows of `level`."""
    lvl, x = head_forward(model.local_head, ctx, levels)
    d = model.local_descriptor_decoder.net
    desc = LinearFn.apply(x, d[0].linear.weight, d[0].linear.bias, ctx, ACT_RELU)
    desc = LinearFn.apply(desc, d[2].linear.weight, d[2].linear.bias, ctx, ACT_NONE)
    if model.local_descriptor_decoder.normalize:
        desc = L2NormalizeFn.apply(desc, ctx)
    k = model.local_keypoint_regressor.net
    kp = LinearFn.apply(x, k[0].linear.weight, k[0].linear.bias, ctx, ACT_RELU)
    kp = LinearFn.apply(kp, k[2].linear.weight, k[2].linear.bias, ctx, ACT_TANH)
    g = model.local_sigma_regressor.net
    sg = LinearFn.apply(x, g[0].linear.weight, g[0].linear.bias, ctx, ACT_RELU)
    sg = LinearFn.apply(sg, g[2].linear.weight, g[2].linear.bias, ctx, ACT_SOFTPLUS)
    return lvl, desc, kp, sg


# ----------------------------------------------------------------------------- sharded step plumbing
def all_reduce_gradients(params: List[torch.nn.Parameter], group=None, world_size: Optional[int] = None):
    """Sum the gradients of all ranks in ONE flat RCCL all-reduce (4.71 M values = 18.8 MB for EgoNN; with the loss
    evaluated on the all-gathered embeddings each rank holds the contribution of its own scans, so the sum is the
    gradient of the whole batch — no averaging)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return
    ps = [p for p in params if p.grad is not None]
    if not ps:
        return
    from .distributed import all_reduce_sum
    flat = torch.cat([p.grad.reshape(-1) for p in ps])
    all_reduce_sum(flat, group)
    o = 0
    for p in ps:
        n = p.grad.numel()
        p.grad.copy_(flat[o:o + n].view_as(p.grad))
        o += n


class TrainStep:
    """One optimisation step of the reference's global phase (training/trainer.py:157-175,193), sharded over the
    ranks of the default process group (BASELINE configs[3]: batch 256 = 32 scans per GPU on 8 GPUs):

        forward of this rank's scans (SyncBN statistics over the whole batch: one all-reduce of C+1 and one of C
        values per BatchNorm layer and direction)
        -> RCCL all-gather of the (b_local, 256) global descriptors (differentiable, distributed.py)
        -> batch-hard triplet (or, with `loss_fn`, contrastive) loss on the gathered (B, 256) matrix with the (B, B) masks
           every rank holds
        -> backward (each rank back-propagates the rows it produced)
        -> ONE flat SUM all-reduce of the parameter gradients -> optimizer.step()

    With a single process it is exactly the reference's step."""

    def __init__(self, model, optimizer, margin: float = 0.2, loss_fn=None):
        """loss_fn: a global loss with the call (embeddings, positives_mask, negatives_mask) -> (loss, stats, hard_triplets),
        e.g. loss.BatchHardContrastiveLossWithMasks(0.2, 0.65); None = the batch-hard triplet loss with `margin`."""
        from .loss import BatchHardTripletLossWithMasks
        self.model, self.optimizer = model, optimizer
        self.loss_fn = BatchHardTripletLossWithMasks(margin) if loss_fn is None else loss_fn

    def __call__(self, batch: Dict[str, torch.Tensor], positives_mask: torch.Tensor, negatives_mask: torch.Tensor,
                 step_optimizer: bool = True, shard_sizes=None):
        """shard_sizes: scans per rank when every rank knows them from the sampler (e.g. `distributed.shard_bounds` of the
        B = positives_mask.shape[0] scans): the embedding exchange is then ONE all-gather with no host synchronisation.
        Default (None): the sizes are exchanged first, so ANY sharding works and a mismatch can never leave some ranks
        inside a collective the others did not enter."""
        import torch.distributed as dist
        from .distributed import all_gather_embeddings
        sharded = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        model = self.model
        model.train()
        model.sync_bn_group = dist.group.WORLD if sharded else None
        self.optimizer.zero_grad(set_to_none=True)
        y = model(batch, disable_local_head=True)
        emb = all_gather_embeddings(y['global'], shard_sizes if sharded else None)
        dev = emb.device
        loss, stats, _ = self.loss_fn(emb, positives_mask.to(dev), negatives_mask.to(dev))
        loss.backward()
        if sharded:
            all_reduce_gradients(list(model.parameters()))
        if step_optimizer:
            self.optimizer.step()
        return loss.detach(), stats


class EgoNNTrainStep:
    """One full optimisation step of the reference (training/trainer.py:160-193), both phases:

        zero the gradients
        -> the global phase exactly as `TrainStep` runs it (forward, batch-hard loss, backward; no optimizer step)
        -> forward of the anchor batch and of the positive batch in train mode (:183-184)
        -> the local loss of the (anchor, positive) pairs in one library call (`BatchedKeypointCorrLoss`, :186-189)
        -> backward, accumulating onto the gradients of the global phase (:192)
        -> ONE optimizer step (:193)

    Single process only: sharding the pairs over ranks is not implemented."""

    def __init__(self, model, optimizer, margin: float = 0.2, loss_fn=None, local_loss_fn=None):
        """loss_fn: the global loss as in `TrainStep`; local_loss_fn: a local loss with the call of `KeypointCorrLoss`
        (None = `make_local_loss(batched=True)`)."""
        from .local_loss import make_local_loss
        self.model, self.optimizer = model, optimizer
        self.global_step = TrainStep(model, optimizer, margin, loss_fn)
        self.local_loss_fn = make_local_loss(batched=True) if local_loss_fn is None else local_loss_fn

    def __call__(self, batch: Dict[str, torch.Tensor], positives_mask: torch.Tensor, negatives_mask: torch.Tensor,
                 local_batch: Dict):
        """local_batch: the dict of the reference's make_collate_fn_6DOF (datasets/dataset_utils.py:98-151): anc_batch,
        pos_batch, anc_pcd, pos_pcd, T_gt, len_batch.  Returns (global_loss, local_loss, stats): device tensors; stats holds
        the global loss's stats and the local metrics (the local ones win a name clash, e.g. 'loss')."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("EgoNNTrainStep runs in a single process: the local phase is not sharded over ranks")
        model = self.model
        global_loss, stats = self.global_step(batch, positives_mask, negatives_mask, step_optimizer=False)   # zeroes the gradients
        dev = global_loss.device
        # two graphs are alive until the backward: each forward gets a context (plan + kernel maps) of its own.  The global
        # head runs too, as in the reference (its output is unused, its gradient zero).
        y1 = model(local_batch['anc_batch'], context_slot=1)
        y2 = model(local_batch['pos_batch'], context_slot=2)
        local_loss, local_stats = self.local_loss_fn(local_batch['anc_pcd'].to(dev), y1['keypoints'], y1['sigma'], y1['descriptors'],
                                                     local_batch['pos_pcd'].to(dev), y2['keypoints'], y2['sigma'], y2['descriptors'],
                                                     local_batch['T_gt'], local_batch['len_batch'])
        local_loss.backward()
        self.optimizer.step()
        out = dict(stats)
        out.update(local_stats)
        return global_loss, local_loss.detach(), out

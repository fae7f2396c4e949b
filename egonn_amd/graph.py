"""Each model graph stated once, against an op set.

An op set says what a convolution (+ BatchNorm), a block tail, an addition and the poolings ARE in one mode: `EvalOps` (here:
folded BatchNorm in the convolution's epilogue, no tape) and `train.TrainOps` (batch-statistics BatchNorm, autograd Functions).
The graphs below only say in which order they come, so the eval and the train path of a model cannot drift apart, and the
sequence of library calls of both is pinned by tests/test_graph_calls_host.py.
"""
from __future__ import annotations

from . import _lib


class EvalOps:
    """eval mode on the per-operator entry points (run under torch.no_grad)"""

    def __init__(self, ctx: _lib.Context):
        self.ctx = ctx

    def conv_bn(self, level_in, level_out, x, conv, bn, relu):
        scale, shift = self.ctx.bn_fold(bn.bn)          # folded right before the convolution that applies it
        return self.ctx.conv(level_in, level_out, conv.kernel_size, x, conv.kernel.detach(), scale, shift, relu=relu)

    def conv(self, level_in, level_out, x, conv):
        if conv.transpose:
            return self.ctx.conv_transpose(level_in, x, conv.kernel.detach())
        return self.ctx.conv(level_in, level_out, conv.kernel_size, x, conv.kernel.detach())

    def tail(self, level, t, residual, block):
        if hasattr(block, 'se'):      # SEBasicBlock tail (layers/senet_block.py:81-87): pool -> fc gate -> relu(t * gate + res)
            gate = self.ctx.se_gate(self.ctx.global_avg_pool(level, t), *block.se.tensors())
            return self.ctx.gate_residual(level, t, gate, residual, relu=True)
        return self.ctx.block_tail(level, t, residual, block.eca.conv.weight if hasattr(block, 'eca') else None)

    def add(self, a, b):
        return self.ctx.add(a, b)

    def gem(self, level, x, p):
        return self.ctx.gem(level, x, p)

    def max_pool(self, level, x):
        return self.ctx.global_max_pool(level, x)

    def avg_pool(self, level, x):
        return self.ctx.global_avg_pool(level, x)

    def netvlad(self, level, x, wrapper):
        return wrapper.run(self.ctx, level, x)


def residual_block(ops, level, x, block):
    """ME BasicBlock.forward / ECABasicBlock (layers/eca_block.py:56-73) / SEBasicBlock (layers/senet_block.py:72-87):
    conv1 norm1 relu, conv2 norm2, [downsample], tail.  The EgoNN trunk and MinkFPN both use it."""
    t = ops.conv_bn(level, level, x, block.conv1, block.norm1, True)
    t = ops.conv_bn(level, level, t, block.conv2, block.norm2, False)
    res = x
    if block.downsample is not None:
        res = ops.conv_bn(level, level, x, block.downsample[0], block.downsample[1], False)
    return ops.tail(level, t, res, block)


def top_down(ops, level, x, steps):
    """The top-down pass of MinkFPN and MinkHead.  steps: one (tconv, lateral feature map or None, its conv1x1) per level
    downwards from `level`."""
    for tconv, f, lateral in steps:
        x = ops.conv(level, level - 1, x, tconv)
        level -= 1
        if f is not None:
            x = ops.add(x, ops.conv(level, level, f, lateral))
    return level, x


def minkfpn(ops, fpn, x0):
    """MinkFPN.forward (reference models/minkfpn.py:65-93) on the plan of ops.ctx; x0: level-0 features (None: all ones).
    Returns (level, features) of the finest map of the top-down pass."""
    x = ops.conv_bn(0, 0, x0, fpn.conv0, fpn.bn0, True)
    fmaps = []
    if fpn.num_top_down == fpn.num_bottom_up:
        fmaps.append((0, x))
    level = 0
    for ndx, (conv, bn, blocks) in enumerate(zip(fpn.convs, fpn.bn, fpn.blocks)):
        x = ops.conv_bn(level, level + 1, x, conv, bn, True)
        level += 1
        for b in blocks:
            x = residual_block(ops, level, x, b)
        if fpn.num_bottom_up - 1 - fpn.num_top_down <= ndx < len(fpn.convs) - 1:
            fmaps.append((level, x))
    assert len(fmaps) == fpn.num_top_down and [l for l, _ in fmaps] == list(range(level - len(fmaps), level))
    x = ops.conv(level, level, x, fpn.conv1x1[0])
    return top_down(ops, level, x, [(tconv, fmaps[-ndx - 1][1], fpn.conv1x1[ndx + 1]) for ndx, tconv in enumerate(fpn.tconvs)])


# PoolingWrapper.forward (layers/pooling.py:13-43): method -> f(ops, level, x, the pooling module)
POOLING = {
    'GeM': lambda ops, level, x, m: ops.gem(level, x, m.p),
    'MAC': lambda ops, level, x, m: ops.max_pool(level, x),
    'SPoC': lambda ops, level, x, m: ops.avg_pool(level, x),
    'netvlad': lambda ops, level, x, m: ops.netvlad(level, x, m),
    'netvladgc': lambda ops, level, x, m: ops.netvlad(level, x, m),
}


def pool(ops, level, x, pooling, method: str):
    """global pooling over the rows of `level`: `pooling` is the GeM / MAC / SPoC / NetVLADWrapper module, `method` its name"""
    if method not in POOLING:
        raise NotImplementedError(f'Unknown pooling method: {method}')
    return POOLING[method](ops, level, x, pooling)

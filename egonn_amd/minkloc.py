"""MinkLoc / MinkLoc3D (MinkFPN backbone + GeM) with the reference's Python surface, executed through the
per-operator entry points of libegonn_hip (reference: models/minkfpn.py, models/minkloc.py,
third_party/minkloc3d/minkloc.py, models/resnet.py:81-117; blocks: ME BasicBlock, layers/eca_block.py ECABasicBlock,
layers/senet_block.py SEBasicBlock).  Same kernels as EgoNN, second graph; the module
tree only holds parameters (identical state_dict keys/shapes), there is no PyTorch fallback.  MinkLoc's pooling
(layers/pooling.py:13-43) is GeM, MAC, SPoC, netvlad or netvladgc.  The graph itself (MinkFPN walk, residual block, pooling
dispatch) is stated once in egonn_amd/graph.py; eval mode runs it on graph.EvalOps, train mode on train.TrainOps.
"""
from __future__ import annotations

from typing import Dict, Sequence

import torch
import torch.nn as nn

from . import _lib, graph, train
from .model import SparseConv, BatchNorm, BasicBlock, SELayer, PlanModule, PoolingWrapper, GeM  # noqa: F401 (SELayer: re-export)


class MinkFPN(nn.Module):
    """reference models/minkfpn.py:9-93 (parameter layout of network_initialization :26-63)."""

    def __init__(self, in_channels, out_channels, num_top_down=1, conv0_kernel_size=5, block='BasicBlock',
                 layers: Sequence[int] = (1, 1, 1), planes: Sequence[int] = (32, 64, 64)):
        super().__init__()
        assert len(layers) == len(planes) and 1 <= len(layers) and 0 <= num_top_down <= len(layers)
        if block == 'Bottleneck':
            raise NotImplementedError(
                "block 'Bottleneck': the reference cannot run it either, so there is nothing to match: a Bottleneck layer emits "
                "planes[-1] * 4 channels (models/resnet.py:107) while MinkFPN builds its lateral conv1x1[0] for planes[-1] input "
                "channels (models/minkfpn.py:49)")
        if block not in ('BasicBlock', 'ECABasicBlock', 'SEBasicBlock'):
            raise NotImplementedError(f'block {block!r}: the MI355X path implements BasicBlock, ECABasicBlock and SEBasicBlock')
        self.num_bottom_up, self.num_top_down = len(layers), num_top_down
        self.layers, self.planes, self.lateral_dim = list(layers), list(planes), out_channels
        eca, se = block == 'ECABasicBlock', block == 'SEBasicBlock'
        self.convs, self.bn, self.blocks = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        self.tconvs, self.conv1x1 = nn.ModuleList(), nn.ModuleList()
        inplanes = planes[0]
        self.conv0 = SparseConv(in_channels, inplanes, conv0_kernel_size)
        self.bn0 = BatchNorm(inplanes)
        for plane, layer in zip(planes, layers):
            self.convs.append(SparseConv(inplanes, inplanes, 2))
            self.bn.append(BatchNorm(inplanes))
            down = None
            if inplanes != plane:
                down = nn.Sequential(SparseConv(inplanes, plane, 1), BatchNorm(plane))
            blocks = [BasicBlock(inplanes, plane, down, eca, se)]
            inplanes = plane
            blocks += [BasicBlock(inplanes, plane, None, eca, se) for _ in range(1, layer)]
            self.blocks.append(nn.Sequential(*blocks))
        for i in range(num_top_down):
            self.conv1x1.append(SparseConv(planes[-1 - i], out_channels, 1))
            self.tconvs.append(SparseConv(out_channels, out_channels, 2, transpose=True))
        if num_top_down < self.num_bottom_up:
            self.conv1x1.append(SparseConv(planes[-1 - num_top_down], out_channels, 1))
        else:
            self.conv1x1.append(SparseConv(planes[0], out_channels, 1))

    def run(self, ctx: _lib.Context, feats0: torch.Tensor):
        """eval-mode forward on the plan of `ctx`: (level, features) of the finest top-down map"""
        return graph.minkfpn(graph.EvalOps(ctx), self, feats0)


class _MinkLocBase(PlanModule):
    sync_bn_group = None          # process group of the SyncBN statistics in train mode (None = this process)

    pooling_method = 'GeM'
    block = 'BasicBlock'
    quantizer = None              # model_factory attaches the configuration's quantizer (what GlobalExtractor voxelises with)
    # egonn_minkfpn_forward: run every top-down step as one launch on the fp16 matrix pipe (egonn_topdown_step's split arithmetic)
    # instead of the exact sequence.  Off: tools/time_minkloc.py did not measure it faster.
    split_topdown = False
    _handle = None
    _registered = None

    # ------------------------------------------------------------------ the one-call path (egonn_minkfpn_forward)
    def minkfpn_spec(self):
        """(planes, layers, num_top_down, feature_size, block, pooling) as egonn_minkfpn_finalize takes them; raises
        NotImplementedError for a model the one-call path does not cover (the per-operator `forward` runs those)."""
        fpn = self.backbone
        if self.block not in _lib.MINKFPN_BLOCKS:
            raise NotImplementedError(f"block {self.block!r}: the one-call MinkFPN forward covers BasicBlock and ECABasicBlock; "
                                      f"model(batch) runs this model on the per-operator path")
        if self.pooling_method not in _lib.MINKFPN_POOLING:
            raise NotImplementedError(f"pooling {self.pooling_method!r}: the one-call MinkFPN forward covers GeM, MAC and SPoC; "
                                      f"model(batch) runs this model on the per-operator path")
        if fpn.conv0.kernel.shape[1] != 1 or fpn.conv0.kernel_size != 5:
            raise NotImplementedError("the one-call MinkFPN forward assumes the k=5 input layer on unit (one-channel) features")
        return (tuple(fpn.planes), tuple(fpn.layers), fpn.num_top_down, fpn.lateral_dim, _lib.MINKFPN_BLOCKS[self.block],
                _lib.MINKFPN_POOLING[self.pooling_method])

    @property
    def out_level(self) -> int:
        """level of the feature map the pooling reads"""
        return self.backbone.num_bottom_up - self.backbone.num_top_down

    def _sync_weights(self):
        """(Re)register the weights with the HIP model and fold / pack them when any tensor moved or was written to
        (as MinkGL._sync_weights: num_batches_tracked carries the version of the running statistics)."""
        spec = self.minkfpn_spec()
        sig = tuple((k, v.data_ptr(), v._version) for k, v in self.state_dict(keep_vars=True).items())
        if self._handle is not None and sig == self._registered:
            return
        if self._handle is None:
            self._handle = _lib.ModelHandle()
        for k, v in self.state_dict(keep_vars=True).items():
            if v.dtype != torch.float32:
                continue
            t = v.detach()
            if not t.is_contiguous():
                raise RuntimeError(f"parameter {k} is not contiguous")
            self._handle.set_tensor(k, t)
        self._handle.finalize_minkfpn(*spec)
        self._registered = sig

    @torch.no_grad()
    def forward_on_plan(self, ctx: _lib.Context, outputs=None, want_map: bool = False):
        """The whole eval graph on the plan `ctx` holds (egonn_voxelize / egonn_coords_set, eager or reserved) as ONE library
        call on unit features.  outputs: preallocated (global (B, D), map or None) for a reserved (capturable) plan — the map
        holds `ctx.level_capacity(self.out_level)` rows; no host synchronisation either way.  Returns {'global': (B, D)} and,
        when a map was asked for, 'map': (capacity of the out level, D) whose first level_count(out_level) rows are valid."""
        self._sync_weights()
        if outputs is not None:
            out_g, out_m = outputs
        else:
            dev = ctx.device
            out_g = torch.empty((ctx.batch_size, self.feature_size), dtype=torch.float32, device=dev)
            out_m = None
            if want_map:
                out_m = torch.empty((ctx.level_capacity(self.out_level), self.feature_size), dtype=torch.float32, device=dev)
        flags = _lib.MINKFPN_SPLIT_TOPDOWN if self.split_topdown else 0
        _lib.call(ctx.device, ctx.lib.egonn_minkfpn_forward, ctx.h, self._handle.h, flags, _lib._ptr(out_g), _lib._ptr(out_m))
        y = {'global': out_g}
        if out_m is not None:
            y['map'] = out_m
        return y

    def _forward(self, batch: Dict[str, torch.Tensor], pooling: nn.Module):
        """pooling: the GeM / MAC / SPoC / NetVLADWrapper module of `pooling_method`"""
        method = self.pooling_method
        if self.training and method != 'GeM' and next(self.parameters()).device.type != 'cuda':
            raise NotImplementedError(f"pooling method {method!r} in train mode runs on the HIP device only; there is no "
                                      f"CPU fallback")
        ctx, feats = self._plan(batch)
        if self.training:     # batch-statistics BatchNorm + autograd through the HIP operators (egonn_amd/train.py)
            if not bool((feats == 1).all()):
                raise NotImplementedError("train mode supports the reference's all-ones input features only")
            level, x = train.minkfpn_forward(self.backbone, ctx, self.sync_bn_group)
            assert x.shape[1] == self.feature_size
            return {'global': train.pool(ctx, level, x, pooling, method, self.sync_bn_group)}
        with torch.no_grad():
            level, x = self.backbone.run(ctx, ctx.gather_input(feats))
            assert x.shape[1] == self.feature_size
            g = graph.pool(graph.EvalOps(ctx), level, x, pooling, method)
        assert g.dim() == 2 and g.shape[1] == self.output_dim
        return {'global': g}


class MinkLoc(_MinkLocBase):
    """reference models/minkloc.py:13-75"""

    def __init__(self, in_channels, feature_size, output_dim, planes, layers, num_top_down, conv0_kernel_size,
                 block='BasicBlock', pooling_method='GeM'):
        super().__init__()
        self.in_channels, self.feature_size, self.output_dim, self.block = in_channels, feature_size, output_dim, block
        self.pooling_method = pooling_method
        self.backbone = MinkFPN(in_channels=in_channels, out_channels=feature_size, num_top_down=num_top_down,
                                conv0_kernel_size=conv0_kernel_size, block=block, layers=layers, planes=planes)
        self.pooling = PoolingWrapper(pool_method=pooling_method, in_dim=feature_size, output_dim=output_dim)
        self.pooled_feature_size = self.pooling.output_dim

    def forward(self, batch, disable_local_head: bool = True):
        assert disable_local_head, "MinkLoc model has only the global head"
        return self._forward(batch, self.pooling.pooling)

    def print_info(self):
        print('Model class: MinkLoc')
        print('Total parameters: {}'.format(sum(p.nelement() for p in self.parameters())))
        print('Backbone parameters: {}'.format(sum(p.nelement() for p in self.backbone.parameters())))
        print('Backbone building block: {}'.format(self.block))
        print('Pooling method: {}'.format(self.pooling_method))


class MinkLoc3D(_MinkLocBase):
    """reference third_party/minkloc3d/minkloc.py:9-44"""

    def __init__(self):
        super().__init__()
        self.feature_size = self.output_dim = 256
        self.backbone = MinkFPN(in_channels=1, out_channels=256, num_top_down=1, conv0_kernel_size=5,
                                layers=[1, 1, 1], planes=[32, 64, 64])
        self.pooling = GeM(input_dim=256)

    def forward(self, batch, disable_local_head: bool = True):
        assert disable_local_head, "MinkLoc3D model has only the global head"
        return self._forward(batch, self.pooling)

    def print_info(self):
        print('Model class: MinkLoc')
        print('Total parameters: {}'.format(sum(p.nelement() for p in self.parameters())))

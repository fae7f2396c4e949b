"""Batch-hard triplet and contrastive losses with masks on the device — reference models/loss.py:146-204 (and the miner
:95-143).

    loss_fn = BatchHardTripletLossWithMasks(margin=0.2)
    loss, stats, hard_triplets = loss_fn(embeddings, positives_mask, negatives_mask)

    loss_fn = BatchHardContrastiveLossWithMasks(pos_margin=0.2, neg_margin=0.65)       # same call, its own stats keys

`loss` is a 0-d tensor wired into autograd (its backward hands dLoss/dEmbeddings, computed by the same HIP call,
to whatever produced `embeddings` — e.g. `egonn_amd.distributed.all_gather_embeddings`); `stats` has the
reference's keys; `hard_triplets` = (a, p, n) index tensors.  Arithmetic: libegonn_hip (no torch fallback).
"""
from __future__ import annotations

import torch

from . import _lib


class _TripletLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, embeddings, pos_mask, neg_mask, margin):
        lib = _lib.load()
        e = embeddings.detach().contiguous().float()
        assert e.is_cuda and e.dim() == 2, "batch-hard triplet loss runs on the HIP device only"
        n, d = e.shape
        pm = pos_mask.to(device=e.device, dtype=torch.uint8).contiguous()
        nm = neg_mask.to(device=e.device, dtype=torch.uint8).contiguous()
        assert pm.shape == (n, n) and nm.shape == (n, n)
        stats = torch.empty(10, dtype=torch.float32, device=e.device)
        trip = torch.empty((n, 3), dtype=torch.int32, device=e.device)
        grad = torch.empty_like(e)
        scratch = torch.empty(lib.egonn_triplet_loss_scratch_floats(n), dtype=torch.float32, device=e.device)
        _lib.call(e.device, lib.egonn_triplet_loss, e.data_ptr(), n, d, pm.data_ptr(), nm.data_ptr(), float(margin),
                  stats.data_ptr(), trip.data_ptr(), grad.data_ptr(), scratch.data_ptr())
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(stats, trip)
        return stats[0].clone(), stats, trip

    @staticmethod
    def backward(ctx, g_loss, g_stats, g_trip):
        (grad,) = ctx.saved_tensors
        return grad * g_loss, None, None, None


class BatchHardTripletLossWithMasks:
    def __init__(self, margin: float):
        self.margin = margin

    def __call__(self, embeddings, positives_mask, negatives_mask):
        loss, st, trip = _TripletLossFn.apply(embeddings, positives_mask, negatives_mask, self.margin)
        s = st.tolist()                                    # the reference also syncs here (.item() calls)
        keep = trip[:, 0] >= 0
        hard_triplets = (trip[keep, 0].long(), trip[keep, 1].long(), trip[keep, 2].long())
        stats = {'loss': s[0], 'avg_embedding_norm': s[3], 'num_non_zero_triplets': int(s[2]),
                 'num_triplets': int(s[1]), 'mean_pos_pair_dist': s[4], 'mean_neg_pair_dist': s[7],
                 'max_pos_pair_dist': s[5], 'max_neg_pair_dist': s[8], 'min_pos_pair_dist': s[6],
                 'min_neg_pair_dist': s[9]}
        return loss, stats, hard_triplets


class _ContrastiveLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, embeddings, pos_mask, neg_mask, pos_margin, neg_margin):
        lib = _lib.load()
        e = embeddings.detach().contiguous().float()
        assert e.is_cuda and e.dim() == 2, "batch-hard contrastive loss runs on the HIP device only"
        n, d = e.shape
        pm = pos_mask.to(device=e.device, dtype=torch.uint8).contiguous()
        nm = neg_mask.to(device=e.device, dtype=torch.uint8).contiguous()
        assert pm.shape == (n, n) and nm.shape == (n, n)
        stats = torch.empty(13, dtype=torch.float32, device=e.device)
        trip = torch.empty((n, 3), dtype=torch.int32, device=e.device)
        grad = torch.empty_like(e)
        scratch = torch.empty(lib.egonn_contrastive_loss_scratch_floats(n), dtype=torch.float32, device=e.device)
        _lib.call(e.device, lib.egonn_contrastive_loss, e.data_ptr(), n, d, pm.data_ptr(), nm.data_ptr(), float(pos_margin),
                  float(neg_margin), stats.data_ptr(), trip.data_ptr(), grad.data_ptr(), scratch.data_ptr())
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(stats, trip)
        return stats[0].clone(), stats, trip

    @staticmethod
    def backward(ctx, g_loss, g_stats, g_trip):
        (grad,) = ctx.saved_tensors
        return grad * g_loss, None, None, None, None


class BatchHardContrastiveLossWithMasks:
    """reference models/loss.py:175-204: the same miner, then pytorch_metric_learning's ContrastiveLoss on the mined triplets
    read as the pairs (a, p) and (a, n) (plain Euclidean distance, AvgNonZeroReducer per pair set; egonn_contrastive_loss)."""

    def __init__(self, pos_margin: float, neg_margin: float):
        self.pos_margin, self.neg_margin = pos_margin, neg_margin

    def __call__(self, embeddings, positives_mask, negatives_mask):
        loss, st, trip = _ContrastiveLossFn.apply(embeddings, positives_mask, negatives_mask, self.pos_margin, self.neg_margin)
        s = st.tolist()                                    # the reference also syncs here (.item() calls)
        keep = trip[:, 0] >= 0
        hard_triplets = (trip[keep, 0].long(), trip[keep, 1].long(), trip[keep, 2].long())
        stats = {'loss': s[0], 'avg_embedding_norm': s[6], 'pos_pairs_above_threshold': int(s[2]),
                 'neg_pairs_above_threshold': int(s[3]), 'pos_loss': s[4], 'neg_loss': s[5], 'num_pairs': 2 * int(s[1]),
                 'mean_pos_pair_dist': s[7], 'mean_neg_pair_dist': s[10], 'max_pos_pair_dist': s[8],
                 'max_neg_pair_dist': s[11], 'min_pos_pair_dist': s[9], 'min_neg_pair_dist': s[12]}
        return loss, stats, hard_triplets


def make_losses(margin: float = 0.2, loss: str = 'BatchHardTripletMarginLoss', pos_margin: float = 0.2,
                neg_margin: float = 0.65):
    """The global loss of reference models/loss.py:12-21: loss = BatchHardTripletMarginLoss (config/config_egonn.txt:20-22)
    with `margin`, or BatchHardContrastiveLoss with `pos_margin` / `neg_margin` (defaults: misc/utils.py:158-160)."""
    if loss == 'BatchHardTripletMarginLoss':
        return BatchHardTripletLossWithMasks(margin)
    if loss == 'BatchHardContrastiveLoss':
        return BatchHardContrastiveLossWithMasks(pos_margin, neg_margin)
    raise NotImplementedError(f'Unknown loss: {loss}')

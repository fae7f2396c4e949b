"""Rotational invariance of a global descriptor: the reference's `MyEvaluator.evaluate` (eval/evaluate_with_rotations.py:41-83)
on the device.  The map set is embedded once; for every rotation bound the query scans are rotated about +z by an angle drawn
uniformly in +-bound (the reference's RandomRotation(max_theta=bound, axis=z): the ROTATE stage of `augment_points`), embedded
and scored with `recall_at_k`.  Scans stay on the device between the passes."""
from __future__ import annotations

from typing import Dict, Sequence

import numpy as np
import torch

from . import augment
from .retrieval import recall_at_k


def _embed(extractor, scans, batch_size: int, rotate=None):
    """scans: device tensors (n_i, 3) -> (len(scans), D).  rotate: (AugmentParams, draw) of the rotation, or None"""
    out = []
    for lo in range(0, len(scans), batch_size):
        part = scans[lo:lo + batch_size]
        offsets = [0]
        for p in part:
            offsets.append(offsets[-1] + p.shape[0])
        pts = part[0] if len(part) == 1 else torch.cat(part, dim=0)
        if rotate is not None:
            params, draw = rotate
            dev = pts.device
            off = torch.tensor(offsets, dtype=torch.int64, device=dev)
            ids = torch.arange(lo, lo + len(part), dtype=torch.int32, device=dev)       # the draw's key: the query index
            pts = augment.augment_points(pts.contiguous(), off, ids, params, draw=draw, set_id=0).points
        out.append(extractor.extract_checked(pts.contiguous(), offsets)['global'].clone())
    return torch.cat(out, dim=0)


def evaluate_with_rotations(extractor, map_scans: Sequence, query_scans: Sequence, map_positions, query_positions,
                            radius: Sequence[float], k: int = 20, rotations=np.arange(0., 181., 10.), seed: int = 0,
                            batch_size: int = 16) -> Dict:
    """{rotation: {'recall': {r: [recall@1 .. recall@k]}, 'embeddings': (Q, D) query descriptors of that pass}}.
    extractor: a `GlobalExtractor` (anything with `extract_checked(points, offsets) -> {'global'}` and `.model`).  The angle of
    query scan i under the j-th rotation bound is the ROTATE draw keyed by (seed, j, i): `augment_points(points, offsets,
    scan_ids=[i..], AugmentParams(seed=seed, stages=ROTATE, max_theta=bound), draw=j)`."""
    if len(map_scans) != len(map_positions):
        raise ValueError(f"evaluate_with_rotations: {len(map_scans)} map scans but {len(map_positions)} map positions")
    if len(query_scans) != len(query_positions):
        raise ValueError(f"evaluate_with_rotations: {len(query_scans)} query scans but {len(query_positions)} query positions")
    if len(map_scans) == 0 or len(query_scans) == 0:
        raise ValueError("evaluate_with_rotations: empty map or query set")
    rotations = [float(r) for r in rotations]
    if len(rotations) >= augment.MAX_DRAW:
        raise ValueError(f"evaluate_with_rotations: at most {augment.MAX_DRAW - 1} rotation bounds")
    dev = extractor.model.context().device
    to_dev = lambda scans: [torch.as_tensor(s, dtype=torch.float32).to(dev).contiguous() for s in scans]      # noqa: E731
    maps, queries = to_dev(map_scans), to_dev(query_scans)
    map_emb = _embed(extractor, maps, batch_size)
    metrics = {}
    for j, bound in enumerate(rotations):
        params = augment.AugmentParams(seed=seed, stages=augment.ROTATE, max_theta=bound)
        q_emb = _embed(extractor, queries, batch_size, rotate=(params, j))
        res = recall_at_k(map_emb, q_emb, map_positions, query_positions, radius, k=k)
        metrics[bound] = {'recall': res['recall'], 'embeddings': q_emb}
    return metrics

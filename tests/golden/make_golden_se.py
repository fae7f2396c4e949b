"""Generates the MinkLoc SEBasicBlock fixtures.  RUNS ONLY IN THE BUILD CONTAINER (needs the reference checkout); the
fixtures it writes are plain data and are committed.

Same recipe as the MinkLoc sections of make_golden.py (which stays as it is): the reference's own ModelParams /
model_factory with `block = SEBasicBlock` (models/minkloc.py:30-31, layers/senet_block.py) run over the build's CPU stand-in
of MinkowskiEngine, with seeded weights (egonn_amd.synth) and seeded clouds:
  * minkloc_se_cart03.npz + minkloc_se_cart03_state_dict_shapes.json: eval mode, two scans of different size (a gate
    applied to the wrong sample's rows shows); the fields of minkloc_eca_cart03, backbone features as fp16;
  * minkloc_se_train_cart03.npz: train mode, two scans; the fields of minkloc_eca_train_cart03 (global, the loss of the
    seeded linear functional, gradient digests of every parameter, BatchNorm running statistics).
Every SE gate the reference evaluates is printed with its range, and generation FAILS unless the gates of each block span
at least 0.3 .. 0.7 over samples x channels: gates that all sit near 0.5, or that all saturate, would let a broken gate
kernel pass.  No reference source text is stored, only arrays the reference code computed.

    python tests/golden/make_golden_se.py
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import bootstrap_reference, minkloc_params, kitti_like_filter, grad_digest  # noqa: E402

# scan, weight and projection seeds no other fixture uses
EVAL_CASE = ("minkloc_se_cart03", [(121, 20000), (122, 9000)], 135)
TRAIN_CASE = ("minkloc_se_train_cart03", [(123, 9000), (124, 7000)], 136, 137)
GATE_LO, GATE_HI = 0.3, 0.7


def watch_gates(model, seen):
    """forward hooks on every SELayer.fc: (block name, (B, C) gate) of each evaluation, in call order"""
    hooks = []
    for name, m in model.named_modules():
        if name.endswith(".se.fc"):
            hooks.append(m.register_forward_hook(lambda mod, i, o, name=name: seen.append((name, o.F.detach().numpy().copy()))))
    return hooks


def check_gates(tag, seen, n_blocks):
    assert len(seen) == n_blocks, (len(seen), n_blocks)
    for name, g in seen:
        print(f"{tag} {name}: gate {g.shape} min {g.min():.4f} max {g.max():.4f}")
        assert g.min() <= GATE_LO and g.max() >= GATE_HI, \
            f"{name}: gates span {g.min():.3f} .. {g.max():.3f}, not {GATE_LO} .. {GATE_HI}: change the weight seed"


def build(mp, wseed, train):
    import torch
    from models.model_factory import model_factory
    from egonn_amd.synth import seeded_state_dict
    model = model_factory(mp)
    shapes = {k: [int(s) for s in v.shape] for k, v in model.state_dict().items()}
    new = seeded_state_dict(wseed, {k: tuple(v) for k, v in shapes.items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in new.items()})
    return (model.train() if train else model.eval()), shapes


def batch(mp, scans):
    import torch
    import MinkowskiEngine as ME
    from egonn_amd.synth import lidar_scan
    coords_list = []
    for seed, n in scans:
        pc = kitti_like_filter(lidar_scan(seed, n_points=n))
        coords, _ = mp.quantizer(torch.from_numpy(pc))
        coords_list.append(coords)
    bc = ME.utils.batched_coordinates(coords_list)
    return bc, torch.ones((bc.shape[0], 1), dtype=torch.float32)


def main():
    bootstrap_reference()
    import numpy as np
    import torch
    import MinkowskiEngine as ME

    torch.manual_seed(0)
    mp = minkloc_params("MinkLoc", "0.3", "SEBasicBlock")

    # ---- eval
    name, scans, wseed = EVAL_CASE
    model, shapes = build(mp, wseed, train=False)
    with open(os.path.join(HERE, f"{name}_state_dict_shapes.json"), "w") as f:
        json.dump(shapes, f, indent=0)                          # insertion order = reference state_dict order
    bc, feats = batch(mp, scans)
    seen = []
    hooks = watch_gates(model, seen)
    with torch.no_grad():
        y = model({"coords": bc, "features": feats})
        check_gates(name, seen, 3)
        for h in hooks:
            h.remove()
        xb = model.backbone(ME.SparseTensor(feats, coordinates=bc))
    c = xb.C.numpy().astype(np.int32)
    order = np.lexsort((c[:, 3], c[:, 2], c[:, 1], c[:, 0]))
    out = {"weight_seed": np.int64(wseed), "coordinates": np.array("cartesian"), "block": np.array("SEBasicBlock"),
           "model": np.array("MinkLoc"), "quantization_step": np.array([0.3]), "n_scans": np.int64(len(scans)),
           "coords": bc.numpy().astype(np.int32), "global": y["global"].numpy(), "backbone_coords": c[order],
           "backbone_feats": xb.F.numpy()[order].astype(np.float16)}
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, "voxels", bc.shape[0], "backbone rows", len(c), f"{os.path.getsize(path) / 1e6:.2f} MB")

    # ---- train
    name, scans, wseed, pseed = TRAIN_CASE
    model, _ = build(mp, wseed, train=True)
    bc, feats = batch(mp, scans)
    seen = []
    hooks = watch_gates(model, seen)
    g = model({"coords": bc, "features": feats})["global"]
    check_gates(name, seen, 3)
    for h in hooks:
        h.remove()
    R = torch.from_numpy(np.random.default_rng(pseed).standard_normal(tuple(g.shape)).astype(np.float32))
    loss = (g * R).sum()
    loss.backward()
    out = {"weight_seed": np.int64(wseed), "proj_seed": np.int64(pseed), "model": np.array("MinkLoc"),
           "block": np.array("SEBasicBlock"), "quantization_step": np.array([0.3]), "n_scans": np.int64(len(scans)),
           "coords": bc.numpy().astype(np.int32), "global": g.detach().numpy(), "loss": np.float64(loss.item())}
    for k, p in model.named_parameters():
        if p.grad is not None:
            out["grad/" + k] = grad_digest(k, p.grad.numpy())
    for k, v in model.state_dict().items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            out["buf/" + k] = v.numpy()
    norms = {k[5:]: float(v[0]) for k, v in out.items() if k.startswith("grad/") and ".se.fc." in k}
    assert len(norms) == 12 and min(norms.values()) > 0, norms       # every SE tensor receives a gradient
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, "voxels", bc.shape[0], "params with grad", sum(1 for k in out if k.startswith("grad/")),
          f"{os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()

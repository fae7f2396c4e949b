"""Generates the MinkLoc pooling fixtures (NetVLAD, NetVLAD-GC, MAC, SPoC).  RUNS ONLY IN THE BUILD CONTAINER (needs the
reference checkout); the fixtures it writes are plain data and are committed.

Same recipe as the MinkLoc section of make_golden.py (which stays as it is): the reference's own ModelParams /
model_factory run over the build's CPU stand-in of MinkowskiEngine, with seeded weights (egonn_amd.synth) and seeded
clouds.  Per case it stores
  * coords / global: the batched input voxels and the reference's descriptors;
  * backbone_coords / backbone_feats / backbone_offsets: the backbone output at the pooling level (fp32, rows sorted by
    (b, x, y, z)) and its per-scan split, so that a restatement of the pooling alone can be checked on the host;
  * global_alone (NetVLAD-GC case): the small scan run on its own — with the reference's zero padding to the largest scan
    of the batch (layers/pooling.py:103) it differs from the same scan's row of `global`;
  * <name>_state_dict_shapes.json: the reference model's state_dict keys / shapes in state_dict order.
No reference source text is stored — only arrays the reference code computed.

    python tests/golden/make_golden_netvlad.py
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import bootstrap_reference, kitti_like_filter  # noqa: E402

SCANS = [(61, 20000), (62, 6000)]          # (seed, points): unequal sizes, scan 1 is the small one

CASES = [
    # name,                      block,           pooling,     output_dim, weight seed, small scan alone
    ("minkloc_netvlad_cart03",   "BasicBlock",    "netvlad",   256,        71,          False),
    ("minkloc_netvladgc_cart03", "ECABasicBlock", "netvladgc", 128,        72,          True),
    ("minkloc_mac_cart03",       "BasicBlock",    "MAC",       256,        73,          False),
    ("minkloc_spoc_cart03",      "ECABasicBlock", "SPoC",      256,        74,          False),
]


def minkloc_params(block: str, pooling: str, output_dim: int):
    from misc.utils import ModelParams
    f = tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False)
    f.write(f"[MODEL]\nmodel = MinkLoc\ncoordinates = cartesian\nquantization_step = 0.3\noutput_dim = {output_dim}\n"
            f"planes = 32,64,64\nlayers = 1,1,1\nnum_top_down = 1\nconv0_kernel_size = 5\nfeature_size = 256\n"
            f"block = {block}\npooling = {pooling}\n")
    f.close()
    mp = ModelParams(f.name)
    os.unlink(f.name)
    return mp


def main():
    bootstrap_reference()
    import numpy as np
    import torch
    import MinkowskiEngine as ME
    from models.model_factory import model_factory
    from egonn_amd.synth import lidar_scan, seeded_state_dict

    torch.manual_seed(0)
    only = sys.argv[1] if len(sys.argv) > 1 else None
    for name, block, pooling, output_dim, wseed, alone in CASES:
        if only and name != only:
            continue
        mp = minkloc_params(block, pooling, output_dim)
        model = model_factory(mp)
        model.eval()
        shapes = {k: [int(s) for s in v.shape] for k, v in model.state_dict().items()}
        with open(os.path.join(HERE, f"{name}_state_dict_shapes.json"), "w") as f:
            json.dump(shapes, f, indent=0)                      # insertion order = reference state_dict order
        new = seeded_state_dict(wseed, {k: tuple(v) for k, v in shapes.items()})
        model.load_state_dict({k: torch.from_numpy(v) for k, v in new.items()})
        out = {"weight_seed": np.int64(wseed), "coordinates": np.array("cartesian"), "block": np.array(block),
               "model": np.array("MinkLoc"), "pooling": np.array(pooling), "output_dim": np.int64(output_dim),
               "quantization_step": np.array([0.3]), "n_scans": np.int64(len(SCANS))}
        coords_list = []
        for seed, n in SCANS:
            pc = kitti_like_filter(lidar_scan(seed, n_points=n))
            coords, _ = mp.quantizer(torch.from_numpy(pc))
            coords_list.append(coords)
        bc = ME.utils.batched_coordinates(coords_list)
        feats = torch.ones((bc.shape[0], 1), dtype=torch.float32)
        with torch.no_grad():
            y = model({"coords": bc, "features": feats})                              # REFERENCE forward
            xb = model.backbone(ME.SparseTensor(feats, coordinates=bc))               # REFERENCE backbone
            if alone:
                bc1 = ME.utils.batched_coordinates(coords_list[1:])
                y1 = model({"coords": bc1, "features": torch.ones((bc1.shape[0], 1), dtype=torch.float32)})
                out["global_alone"] = y1["global"].numpy()
                out["alone_scan"] = np.int64(1)
        out["coords"] = bc.numpy().astype(np.int32)
        out["global"] = y["global"].numpy()
        c = xb.C.numpy().astype(np.int32)
        order = np.lexsort((c[:, 3], c[:, 2], c[:, 1], c[:, 0]))
        out["backbone_coords"] = c[order]
        out["backbone_feats"] = xb.F.numpy()[order].astype(np.float32)
        out["backbone_offsets"] = np.searchsorted(c[order][:, 0], np.arange(len(SCANS) + 1)).astype(np.int64)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print(name, "voxels", bc.shape[0], "backbone rows", np.diff(out["backbone_offsets"]).tolist(),
              f"{os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()

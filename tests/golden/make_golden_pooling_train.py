"""Generates the train-mode pooling fixtures (NetVLAD, NetVLAD-GC, MAC, SPoC).  RUNS ONLY IN THE BUILD CONTAINER (needs
the reference checkout); the fixtures it writes are plain data and are committed.

A. Operator fixture `netvlad_train_ref*.npz`: the reference's own `layers.netvlad.NetVLADLoupe` in `.train()` and float64
   on zero-padded ragged inputs (what NetVLADWrapper's pad_sequence hands it), seeded parameters (egonn_amd.synth), an
   upstream gradient, and everything autograd returns: output, every parameter gradient in full, grad x per scan, the
   BatchNorm running buffers after the step.  Two cases (C=16, D=16, no gating) and (C=64, D=32, gating), each also as the
   `alone` variant: one scan repeated B times (n_b = Nmax for every scan: the pad terms vanish).  The arrays of the
   larger case are spread over several files so that each stays under the committed-file size limit.
B. End-to-end fixtures `minkloc_{netvlad,netvladgc,mac,spoc}_train_cart03.npz`: the recipe of make_golden.py's
   main_train_minkloc (seeded weights, loss (g * R).sum(), grad_digest per parameter, running buffers, global, loss) with
   FIVE scans of unequal size (with B = 2 the B-row bn2 maps every descriptor to +-gamma + beta and the gradients
   upstream of it collapse to the order of eps).

C. Clamp fixture `netvlad_train_edges.npz` (mode `edges`, see main_edges): the recipe of A on the two eps-clamp cases of
   tests/netvlad_edges_data.py.

No reference source text is stored — only arrays the reference code computed.

    python tests/golden/make_golden_pooling_train.py [ops|e2e|edges]
"""
from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import bootstrap_reference, kitti_like_filter, grad_digest  # noqa: E402
from make_golden_netvlad import minkloc_params  # noqa: E402

ROWS = [1, 63, 64, 65, 129, 300, 17, 128]      # rows per scan: straddle the 64-row tile and the 128-row chunk
ALONE_SCAN = 4                                 # the scan the `alone` variant repeats (129 rows)
OP_CASES = [
    # tag,  C,  D,  gating, seed
    ("c16", 16, 16, False, 81),
    ("c64", 64, 32, True, 82),
]
PARAM_KEYS = ["cluster_weights", "cluster_weights2", "hidden1_weights", "bn1.weight", "bn1.bias", "bn2.weight", "bn2.bias",
              "context_gating.gating_weights", "context_gating.bn1.weight", "context_gating.bn1.bias"]
LIMIT = 1 << 20                                # committed-file size limit


def op_files():
    """file name -> predicate on the array key: which arrays the file holds"""
    big = ("c64/grad/hidden1_weights", "c64_alone/grad/hidden1_weights")
    return {
        "netvlad_train_ref.npz": lambda k: k.startswith(("c16/", "c16_alone/", "meta/")),
        "netvlad_train_ref_c64.npz": lambda k: k.startswith("c64/") and k not in big,
        "netvlad_train_ref_c64_gradh.npz": lambda k: k == big[0],
        "netvlad_train_ref_c64_alone.npz": lambda k: k.startswith("c64_alone/") and k not in big,
        "netvlad_train_ref_c64_alone_gradh.npz": lambda k: k == big[1],
    }


def main_ops():
    bootstrap_reference()
    import numpy as np
    import torch
    from layers.netvlad import NetVLADLoupe
    from egonn_amd.synth import seeded_tensor, _key_seed

    out = {"meta/rows": np.asarray(ROWS, dtype=np.int64), "meta/alone_scan": np.int64(ALONE_SCAN)}
    for tag, C, D, gating, seed in OP_CASES:
        scans = []
        for b, n in enumerate(ROWS):
            rng = np.random.default_rng(_key_seed(seed, f"rows{b}"))
            scans.append((rng.standard_normal((n, C)) * 0.8 + 0.3 * rng.standard_normal((1, C))).astype(np.float32))
        for variant, rows in ((tag, scans), (tag + "_alone", [scans[ALONE_SCAN]] * len(ROWS))):
            torch.manual_seed(0)
            m = NetVLADLoupe(feature_size=C, cluster_size=64, output_dim=D, gating=gating, add_batch_norm=True)
            sd = {k: torch.from_numpy(seeded_tensor(seed, k, tuple(v.shape))) for k, v in m.state_dict().items()}
            m.load_state_dict(sd)
            m = m.double().train()
            xs = [torch.from_numpy(r).double().requires_grad_(True) for r in rows]
            padded = torch.nn.utils.rnn.pad_sequence(xs, batch_first=True)          # what NetVLADWrapper builds
            y = m(padded)
            g = np.random.default_rng(_key_seed(seed, "upstream")).standard_normal(tuple(y.shape)).astype(np.float32)
            (y * torch.from_numpy(g).double()).sum().backward()
            p = variant + "/"
            out[p + "C"], out[p + "D"], out[p + "gating"] = np.int64(C), np.int64(D), np.int64(gating)
            out[p + "seed"] = np.int64(seed)
            out[p + "offsets"] = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
            out[p + "x"] = np.concatenate(rows, axis=0)                              # float32 rows, scan after scan
            out[p + "out"] = y.detach().numpy()
            out[p + "upstream"] = g
            out[p + "grad_x"] = np.concatenate([x.grad.numpy() for x in xs], axis=0)
            params = dict(m.named_parameters())
            for k in PARAM_KEYS:
                if k in params:
                    out[p + "grad/" + k] = params[k].grad.numpy()
            for k, v in m.state_dict().items():
                if "running" in k or k.endswith("num_batches_tracked"):
                    out[p + "buf/" + k] = v.numpy()
            print(variant, "M =", padded.shape[0] * padded.shape[1], "out", tuple(y.shape),
                  "|grad x| max", float(np.abs(out[p + "grad_x"]).max()))
    for fname, pred in op_files().items():
        part = {k: v for k, v in out.items() if pred(k)}
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **part)
        size = os.path.getsize(path)
        print(fname, len(part), "arrays", f"{size / 1e6:.3f} MB")
        assert size <= LIMIT, (fname, size)
    assert sum(1 for k in out for pred in op_files().values() if pred(k)) == len(out)


SCANS = [(91, 9000), (92, 3000), (93, 7000), (94, 5000), (95, 4000)]     # (seed, points): five scans, unequal sizes
E2E_CASES = [
    # name,                              block,           pooling,     output_dim, weight seed, projection seed
    ("minkloc_netvlad_train_cart03",   "BasicBlock",    "netvlad",   256,        75,          85),
    ("minkloc_netvladgc_train_cart03", "ECABasicBlock", "netvladgc", 128,        76,          86),
    ("minkloc_mac_train_cart03",       "BasicBlock",    "MAC",       256,        77,          87),
    ("minkloc_spoc_train_cart03",      "ECABasicBlock", "SPoC",      256,        78,          88),
]


def main_e2e():
    bootstrap_reference()
    import numpy as np
    import torch
    import MinkowskiEngine as ME
    from models.model_factory import model_factory
    from egonn_amd.synth import lidar_scan, seeded_state_dict

    only = sys.argv[2] if len(sys.argv) > 2 else None
    for name, block, pooling, output_dim, wseed, pseed in E2E_CASES:
        if only and name != only:
            continue
        mp = minkloc_params(block, pooling, output_dim)
        model = model_factory(mp)
        shapes = {k: [int(s) for s in v.shape] for k, v in model.state_dict().items()}
        new = seeded_state_dict(wseed, {k: tuple(v) for k, v in shapes.items()})
        model.load_state_dict({k: torch.from_numpy(v) for k, v in new.items()})
        model.train()
        coords_list = []
        for seed, n in SCANS:
            pc = kitti_like_filter(lidar_scan(seed, n_points=n))
            coords, _ = mp.quantizer(torch.from_numpy(pc))
            coords_list.append(coords)
        bc = ME.utils.batched_coordinates(coords_list)
        feats = torch.ones((bc.shape[0], 1), dtype=torch.float32)
        if pooling == "MAC":                       # the argmax routing is only pinned where the maximum is unique
            xb = model.backbone(ME.SparseTensor(feats, coordinates=bc))
            for rows in xb._batchwise_row_indices:
                f = xb.F.detach()[rows]
                top2 = torch.topk(f, 2, dim=0).values
                assert bool((top2[0] > top2[1]).all()), "tied maximum in the MAC fixture: change the scan seeds"
            model.load_state_dict({k: torch.from_numpy(v) for k, v in new.items()})      # undo the running-stat update
            model.train()
        g = model({"coords": bc, "features": feats})["global"]
        R = torch.from_numpy(np.random.default_rng(pseed).standard_normal(tuple(g.shape)).astype(np.float32))
        loss = (g * R).sum()
        loss.backward()
        out = {"weight_seed": np.int64(wseed), "proj_seed": np.int64(pseed), "model": np.array("MinkLoc"),
               "block": np.array(block), "pooling": np.array(pooling), "output_dim": np.int64(output_dim),
               "quantization_step": np.array([0.3]), "n_scans": np.int64(len(SCANS)),
               "mac_no_tie": np.int64(pooling == "MAC"),
               "coords": bc.numpy().astype(np.int32), "global": g.detach().numpy(), "loss": np.float64(loss.item())}
        norms = {}
        for k, p in model.named_parameters():
            if p.grad is not None:
                out["grad/" + k] = grad_digest(k, p.grad.numpy())
                norms[k] = float(out["grad/" + k][0])
        for k, v in model.state_dict().items():
            if k.endswith("running_mean") or k.endswith("running_var"):
                out["buf/" + k] = v.numpy()
        lo, hi = min(norms, key=norms.get), max(norms, key=norms.get)
        print(name, "smallest digest norm", lo, norms[lo], "largest", hi, norms[hi], "ratio", norms[lo] / norms[hi])
        if pooling.startswith("netvlad"):
            assert norms[lo] >= 1e-6 * norms[hi], "a gradient is numerically dead: change the scan seeds"
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        print(name, "voxels", bc.shape[0], "params with grad", len(norms), "of", sum(1 for _ in model.parameters()),
              f"{size / 1e6:.2f} MB")
        assert size <= LIMIT, (name, size)


def main_edges():
    """C. `netvlad_train_edges.npz`: main_ops' recipe on the two clamp cases of tests/netvlad_edges_data.py (one scan all zero;
    one column, or all, of cluster_weights2 zero, so that a per-cluster norm, or the whole descriptor's, is exactly 0 and
    F.normalize divides by its eps).  Writes this file only."""
    bootstrap_reference()
    import numpy as np
    import torch
    from layers.netvlad import NetVLADLoupe
    from egonn_amd.synth import seeded_tensor
    from tests import netvlad_edges_data as E

    out = {}
    for name in E.CLAMP_CASES:
        case = E.BY_NAME[name]
        rows, state = E.features(case, "train"), E.state(case, "train")
        torch.manual_seed(0)
        m = NetVLADLoupe(feature_size=case.C, cluster_size=64, output_dim=case.D, gating=case.gating, add_batch_norm=True)
        sd = {k: torch.from_numpy(state[k] if k in state else seeded_tensor(case.seed, k, tuple(v.shape)))
              for k, v in m.state_dict().items()}
        assert all(k in sd for k in state)
        m.load_state_dict(sd)
        m = m.double().train()
        xs = [torch.from_numpy(r).double().requires_grad_(True) for r in rows]
        padded = torch.nn.utils.rnn.pad_sequence(xs, batch_first=True)
        y = m(padded)
        g = E.upstream(case)
        (y * torch.from_numpy(g).double()).sum().backward()
        p = name + "/"
        out[p + "C"], out[p + "D"], out[p + "gating"] = np.int64(case.C), np.int64(case.D), np.int64(case.gating)
        out[p + "seed"] = np.int64(case.seed)
        out[p + "offsets"] = E.offsets(case)
        out[p + "x"] = np.concatenate(rows, axis=0)
        out[p + "cluster_weights2"] = state["cluster_weights2"]                  # the edited tensor, as the module held it
        out[p + "out"] = y.detach().numpy()
        out[p + "upstream"] = g
        out[p + "grad_x"] = np.concatenate([x.grad.numpy() for x in xs], axis=0)
        params = dict(m.named_parameters())
        for k in PARAM_KEYS:
            if k in params:
                out[p + "grad/" + k] = params[k].grad.numpy()
        for k, v in m.state_dict().items():
            if "running" in k or k.endswith("num_batches_tracked"):
                out[p + "buf/" + k] = v.numpy()
        print(name, "M =", padded.shape[0] * padded.shape[1], "out", tuple(y.shape),
              "|grad x| max", float(np.abs(out[p + "grad_x"]).max()))
    path = os.path.join(HERE, "netvlad_train_edges.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("netvlad_train_edges.npz", len(out), "arrays", f"{size / 1e6:.3f} MB")
    assert size <= LIMIT, size


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what == "edges":                 # a mode of its own: `all` regenerates the earlier fixtures only
        main_edges()
    if what in ("all", "ops"):
        main_ops()
    if what in ("all", "e2e"):
        main_e2e()

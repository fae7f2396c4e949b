"""The case table of the NetVLAD edge tests (tests/test_netvlad_edges_host.py on the CPU, tests/test_gpu_netvlad_edges.py on the
device, the `edges` mode of tests/golden/make_golden_pooling_train.py): batches that reach every arm of the row kernels'
dispatch on C, the chunk cap of nv_chunks() from both sides, an empty and a one-row scan, every instantiation of the projection
on ceil(D / 256), partial 16-scan blocks, more scans than one stride of the Nmax reduction, and both eps clamps of F.normalize.

A case: rows per scan, C, D, gating, the modes it runs in, a seed, and edits to the seeded state / the features.  Modes: `eval`
(egonn_netvlad), `train` (egonn_amd.train.netvlad_pool: NetVLADFn, bn2, gating) and `core` (NetVLADFn alone, y before bn2: the
cases with D > TRAIN_MAX_D, which netvlad_pool refuses because BatchNormFn holds at most that many columns while
egonn_netvlad_train_forward / _backward take D up to 1024).  Weights are
op_state()'s seeded tensors; the features follow the operator fixture's recipe (standard_normal * 0.8 + 0.3 * a per-scan offset,
float32).  The restatements at the bottom run the same torch code in float64 (the reference value) and in float32 on the CPU
(e_ref: what fp32 arithmetic alone costs on these inputs)."""
from collections import namedtuple

import numpy as np

from tests import helpers as H

CHUNK_ROWS = H.kernel_constant("NV_CHUNK_ROWS")
MAX_CHUNKS = H.kernel_constant("NV_MAX_CHUNKS")
CAP = CHUNK_ROWS * MAX_CHUNKS                 # the largest scan whose chunks are still CHUNK_ROWS rows
ARM_LIMITS = (64, 128, 256, 512)              # the largest C of <4,4>, <8,4>, <16,4>, <32,2> (netvlad_forward / launch_rows)
NV_BB = 16                                    # scans per workgroup of netvlad_project_kernel
FINISH_STRIDE = 256                           # threads of netvlad_finish_kernel's Nmax reduction
TRAIN_MAX_D = 256                             # egonn_amd.train.BN_MAX_COLUMNS (asserted by the host test)
CLAMP_SCAN, CLAMP_CLUSTER = 1, 3
TINY = 1e-12                                  # feature scale of cluster_clamp_tiny's scan 1
PARAM_KEYS = ["cluster_weights", "cluster_weights2", "hidden1_weights", "bn1.weight", "bn1.bias", "bn2.weight", "bn2.bias",
              "context_gating.gating_weights", "context_gating.bn1.weight", "context_gating.bn1.bias"]

Case = namedtuple("Case", "name rows C D gating modes seed edit")
CLAMP_ROWS = [40, 7, 90, 12, 3]

CASES = [
    # cap on and off by one row, uneven capped chunks (CAP + 1 rows over MAX_CHUNKS chunks), empty scan, one-row scan
    Case("chunk_cap", [0, 5, CAP + 1, 1, CAP, CAP - 1], 16, 16, False, ("eval", "train"), 101, {}),
    # <8,4>; ND = 2 with D % 256 = 16; both sides of one and of two chunks
    Case("arm_8", [CHUNK_ROWS - 1, CHUNK_ROWS, CHUNK_ROWS + 1, 0, CHUNK_ROWS + 2, 2 * CHUNK_ROWS + 1], 96, 272, True,
         ("eval", "core"), 102, {}),
    # <32,2>; 32-row tile edges; capped chunks of (2 CAP + 8) / MAX_CHUNKS = 256.25 rows
    Case("arm_32", [300, 2 * CAP + 8, 33, 31, 32], 512, 16, False, ("eval", "train"), 103, {}),
    # the smallest C of each upper arm, none a multiple of 64
    Case("arm_floor_80", [65, 1, 63, 200], 80, 32, False, ("eval", "train"), 104, {}),
    Case("arm_floor_144", [65, 1, 63, 200], 144, 32, False, ("eval", "train"), 105, {}),
    Case("arm_floor_272", [65, 1, 63, 200], 272, 32, False, ("eval", "train"), 106, {}),
    # ND = 3 ragged, ND = 4, the 1024-wide gating GEMM
    Case("wide_d_528", [64, 65, 1, 17, 300, 129], 16, 528, True, ("eval", "core"), 107, {}),
    Case("wide_d_1024", [64, 65, 1, 17, 300, 129], 16, 1024, True, ("eval", "core"), 108, {}),
    # partial 16-scan blocks of the projection: 16 + 1 and 32 + 1 scans
    Case("many_scans_17", list(range(1, 18)), 48, 48, True, ("eval", "train"), 109, {}),
    Case("many_scans_33", list(range(1, 34)), 48, 48, True, ("eval", "train"), 110, {}),
    # B = 1: no pad term at all (train mode refuses one scan: bn2 needs two rows)
    Case("eval_b1", [CAP + 1], 32, 16, False, ("eval",), 111, {}),
    # the Nmax reduction beyond one stride
    Case("eval_b300", [1, 2, 3] * 100, 16, 16, False, ("eval",), 112, {}),
    # scan 1 all zero and cluster_weights2[0, :, 3] = 0: V[:, 3] of scan 1 is exactly 0 (per-cluster clamp, s_kclamp)
    Case("cluster_clamp", CLAMP_ROWS, 16, 16, False, ("eval", "train"), 113,
         {"zero_scan": CLAMP_SCAN, "w2_zero_cluster": CLAMP_CLUSTER}),
    # scan 1 all zero and cluster_weights2 = 0: scan 1's whole V is 0 (global clamp, s_gclamp): its descriptor is bn2 of a zero row
    Case("global_clamp", CLAMP_ROWS, 16, 16, False, ("eval", "train"), 114, {"zero_scan": CLAMP_SCAN, "w2_zero": True}),
    # scan 1 scaled by TINY instead of zeroed: V[:, 3] of scan 1 is tiny but NOT zero (norm of the order 1e-13 < eps), so the clamp
    # decides the values: the column is V / 1e-12 (norm 0.1, not 1) and its backward has no projection term.  With an exactly zero
    # column both hold trivially (u = 0); here a kernel that ignored the clamp would be off by per cent
    Case("cluster_clamp_tiny", CLAMP_ROWS, 16, 16, False, ("eval", "train"), 116,
         {"scale_scan": (CLAMP_SCAN, TINY), "w2_zero_cluster": CLAMP_CLUSTER}),
    # logits of order 10^2: the softmax must subtract the row maximum.  eval: features x 30; train: bn1.weight x 20
    Case("saturated", [40, 7, 90, 130], 32, 16, False, ("eval", "train"), 115,
         {"x_scale_eval": 30.0, "bn1_weight_scale_train": 20.0}),
]
BY_NAME = {c.name: c for c in CASES}
RUNS = [(c.name, m) for c in CASES for m in c.modes]           # (case, mode) pairs: the parametrisation of both test files
TRAIN_RUNS = [(n, m) for n, m in RUNS if m != "eval"]
REFUSED_CASES = [c.name for c in CASES if "core" in c.modes]
CLAMP_CASES = ["cluster_clamp", "global_clamp", "cluster_clamp_tiny"]
PERMUTED_CASES = ["chunk_cap", "arm_8"]                          # also run under permuted batch indices


def nv_chunks(n):
    """kernels.h nv_chunks(): the chunks of a scan of n rows"""
    return 0 if n <= 0 else min((n + CHUNK_ROWS - 1) // CHUNK_ROWS, MAX_CHUNKS)


def arm(c):
    """index of the row kernels' instantiation a channel count is dispatched to"""
    return next(i for i, lim in enumerate(ARM_LIMITS) if c <= lim)


def offsets(case):
    return np.concatenate([[0], np.cumsum(case.rows)]).astype(np.int64)


def features(case, mode):
    """per-scan float32 feature rows (the operator fixture's recipe), with the case's edits for `mode`"""
    from egonn_amd.synth import _key_seed
    out = []
    for b, n in enumerate(case.rows):
        rng = np.random.default_rng(_key_seed(case.seed, f"rows{b}"))
        out.append((rng.standard_normal((n, case.C)) * 0.8 + 0.3 * rng.standard_normal((1, case.C))).astype(np.float32))
    if "zero_scan" in case.edit:
        out[case.edit["zero_scan"]][:] = 0.0
    if "scale_scan" in case.edit:
        b, f = case.edit["scale_scan"]
        out[b] = (out[b] * np.float32(f)).astype(np.float32)
    if mode == "eval" and "x_scale_eval" in case.edit:
        out = [(f * np.float32(case.edit["x_scale_eval"])).astype(np.float32) for f in out]
    return out


def state(case, mode):
    """the seeded NetVLADLoupe state (float32 numpy, reference key names) with the case's edits for `mode`"""
    from tests.test_netvlad_train_host import op_state
    s = op_state({"C": case.C, "D": case.D, "gating": int(case.gating), "seed": case.seed})
    s = {k: np.array(v, dtype=np.float32) for k, v in s.items()}
    if "w2_zero_cluster" in case.edit:
        s["cluster_weights2"][0, :, case.edit["w2_zero_cluster"]] = 0.0
    if case.edit.get("w2_zero"):
        s["cluster_weights2"][:] = 0.0
    if mode == "train" and "bn1_weight_scale_train" in case.edit:
        s["bn1.weight"] *= np.float32(case.edit["bn1_weight_scale_train"])
    return s


def upstream(case):
    """the upstream gradient of the train step, (B, D) float32"""
    from egonn_amd.synth import _key_seed
    return np.random.default_rng(_key_seed(case.seed, "upstream")).standard_normal((len(case.rows), case.D)).astype(np.float32)


# ------------------------------------------------------------------ restatements in a chosen precision (torch, CPU)
def _bn_eval(s, name, t, dt, eps=1e-5):
    import torch
    g = lambda k: torch.from_numpy(s[name + "." + k]).to(dt)             # noqa: E731
    return (t - g("running_mean")) / torch.sqrt(g("running_var") + eps) * g("weight") + g("bias")


def eval_restated(x, off, s, gating, dtype="float64", parts=False, fold=None):
    """tests/test_netvlad_host.py's netvlad_f64 in torch and in the precision asked for: (B, D) numpy.  parts=True: also the
    per-cluster norms (B, 64) and the global norm (B,) of every scan's V before the clamps.  fold = (scale, shift): bn1 as that
    affine map instead of the running statistics (train_fold: the batch statistics of the train step)."""
    import torch
    import torch.nn.functional as F
    dt = getattr(torch, dtype)
    t = lambda k: torch.from_numpy(s[k]).to(dt)                          # noqa: E731
    x = torch.from_numpy(np.asarray(x, dtype=np.float32)).to(dt)
    wc, w2, hid = t("cluster_weights"), t("cluster_weights2")[0], t("hidden1_weights")
    n = np.diff(np.asarray(off))
    nmax = int(n.max())
    if fold is None:
        bn1 = lambda z: _bn_eval(s, "bn1", z, dt)                        # noqa: E731
    else:
        bn1 = lambda z: z * torch.from_numpy(fold[0]).to(dt) + torch.from_numpy(fold[1]).to(dt)      # noqa: E731
    a_pad = torch.softmax(bn1(torch.zeros(64, dtype=dt)), dim=0)
    rows, nk, ng = [], [], []
    for b in range(len(n)):
        xb = x[int(off[b]):int(off[b + 1])]
        A = torch.softmax(bn1(xb @ wc), dim=1)
        V = xb.t() @ A - (A.sum(0) + float(nmax - n[b]) * a_pad)[None, :] * w2
        nk.append(torch.linalg.vector_norm(V, dim=0))
        V = F.normalize(V, dim=0, p=2)
        ng.append(torch.linalg.vector_norm(V))
        rows.append(F.normalize(V.reshape(1, -1), dim=1, p=2)[0])
    y = _bn_eval(s, "bn2", torch.stack(rows) @ hid, dt)
    if gating:
        y = y * torch.sigmoid(_bn_eval(s, "context_gating.bn1", y @ t("context_gating.gating_weights"), dt))
    return (y.numpy(), torch.stack(nk).numpy(), torch.stack(ng).numpy()) if parts else y.numpy()


def train_fold(x, off, s, eps=1e-5):
    """bn1 of the train step as (scale, shift), float64: the statistics of the B * Nmax zero-padded rows"""
    z = np.asarray(x, dtype=np.float64) @ s["cluster_weights"].astype(np.float64)
    M = float((len(off) - 1) * int(np.diff(off).max()))
    mean = z.sum(0) / M
    scale = s["bn1.weight"].astype(np.float64) / np.sqrt((z * z).sum(0) / M - mean * mean + eps)
    return scale, s["bn1.bias"].astype(np.float64) - mean * scale


def train_restated(x, off, s, gating, up, dtype="float64", head=True):
    """tests/test_netvlad_train_host.py's run_f64 in the precision asked for: (y, grad x, {param: grad}, {buffer: value}).
    head=False: NetVLADFn alone (y before bn2; the parameters and buffers of bn2 and the gating do not appear)"""
    import torch
    from tests.test_netvlad_train_host import netvlad_train_f64
    dt = getattr(torch, dtype)
    p = {k: torch.from_numpy(v).to(dt).requires_grad_(True) for k, v in s.items() if "running" not in k}
    buf = {k: torch.from_numpy(v).to(dt) for k, v in s.items() if "running" in k}
    xt = torch.from_numpy(np.asarray(x, dtype=np.float32)).to(dt).requires_grad_(True)
    y, new = netvlad_train_f64(xt, off, p, buf, gating, head=head)
    (y * torch.from_numpy(np.asarray(up, dtype=np.float32)).to(dt)).sum().backward()
    return (y.detach().numpy(), xt.grad.numpy(), {k: v.grad.numpy() for k, v in p.items() if v.grad is not None},
            {k: v.numpy() for k, v in new.items()})


_CACHE = {}


def reference(name, mode):
    """(float64 result, float32 CPU result) of a case in a mode, computed once per process and shared (read-only)"""
    key = (name, mode)
    if key not in _CACHE:
        case = BY_NAME[name]
        x, off, s = np.concatenate(features(case, mode)), offsets(case), state(case, mode)      # core: train's inputs
        if mode == "eval":
            _CACHE[key] = tuple(eval_restated(x, off, s, case.gating, d) for d in ("float64", "float32"))
        else:
            _CACHE[key] = tuple(train_restated(x, off, s, case.gating, upstream(case), d, head=mode == "train")
                                for d in ("float64", "float32"))
    return _CACHE[key]


def train_tensors(res):
    """a train result as {name: array}: y, grad x, the parameter gradients, the running buffers"""
    y, gx, gp, bufs = res
    out = {"y": y, "grad x": gx}
    out.update({"grad " + k: v for k, v in gp.items()})
    out.update({"buf " + k: v for k, v in bufs.items()})
    return out

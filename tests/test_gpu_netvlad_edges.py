"""GPU tests of NetVLAD / NetVLAD-GC pooling at its edges (run with -m gpu on an MI355X): every case of
tests/netvlad_edges_data.py through egonn_netvlad (eval) and egonn_netvlad_train_forward / _backward (train) against the float64
restatements, held to the project's run-time bound 8 x e_ref (e_ref: the same restatement in float32 on the CPU; floor
16 x 2^-24; tests/helpers.py stage_bound) per tensor and, for y and grad x, per scan in the scan's own scale.  Nothing in a bound
comes from the kernels' output; tests/test_netvlad_edges_host.py caps e_ref at 1e-4.  Plus the exact facts of the clamp cases,
bitwise reruns, and bitwise per-scan results under permuted batch indices.

What the cases reach: all four arms of the row kernels' dispatch on C (netvlad_assign_kernel, nvt_rows1_kernel, nvt_rows2_kernel),
the chunk cap of nv_chunks() from both sides and uneven capped chunks, an empty and a one-row scan, the projection's four
instantiations on ceil(D / 256), partial 16-scan blocks, B = 1 and B > 256, both eps clamps of F.normalize in
netvlad_project_kernel and nvt_norm_bwd_kernel, and logits of order 10^2."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import netvlad_edges_data as E
from tests.test_gpu_netvlad import _Op, _bn_module, _scan_coords
from tests.test_gpu_pooling_train import _module, _step
from tests.test_netvlad_host import PREFIX

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    g.build()
    import egonn_amd
    return egonn_amd


def _np(t):
    return t.detach().cpu().numpy()


class _EdgeOp(_Op):
    """_Op on a case's own (edited) state instead of _weights()"""

    def __init__(self, gpu, case, state):
        self.ctx = gpu._lib.Context(torch.device("cuda", 0))
        self.c, self.d, self.gating = case.C, case.D, case.gating
        self.w = {PREFIX + k: v for k, v in state.items()}
        t = lambda k: torch.from_numpy(self.w[PREFIX + k]).cuda()            # noqa: E731
        self.bn2 = _bn_module(self.w, PREFIX + "bn2.")
        self.args = [t("cluster_weights"), t("cluster_weights2"), _bn_module(self.w, PREFIX + "bn1."),
                     t("hidden1_weights"), self.bn2]
        self.args += [t("context_gating.gating_weights"), _bn_module(self.w, PREFIX + "context_gating.bn1.")] if case.gating \
            else [None, None]


def _coords(case):
    rng = np.random.default_rng(case.seed)
    return [_scan_coords(rng, n) for n in case.rows]


def _scan_of_rows(case):
    return np.repeat(np.arange(len(case.rows)), case.rows)


def _report(table, fails):
    """the table of the run (case x mode x tensor: e_ref, e_gpu, bound, and the ratio e_gpu / e_ref), then the verdict"""
    print(H.format_table(table))
    for batch, config, stage, e_ref, e_gpu, bound in table:
        print(f"ratio {batch:<15}{config:<6}{stage:<42}{e_gpu / max(e_ref, 2.0 ** -24):>9.2f}")
    assert not fails, "\n".join(fails)


def _perm(case):
    """a permutation of the batch indices that moves every scan, the empty one included"""
    B = len(case.rows)
    p = np.random.default_rng(2).permutation(B)
    return p if not (p == np.arange(B)).any() else np.roll(np.arange(B), 1)


# ------------------------------------------------------------------ eval: egonn_netvlad
@pytest.mark.parametrize("name", [n for n, m in E.RUNS if m == "eval"])
def test_netvlad_eval_edges_match_float64(gpu, name):
    case = E.BY_NAME[name]
    B = len(case.rows)
    want, ref32 = E.reference(name, "eval")
    op = _EdgeOp(gpu, case, E.state(case, "eval"))
    coords, feats = _coords(case), E.features(case, "eval")
    x = op.plan(coords, feats)
    assert list(np.diff(op.ctx.level_batch_offsets(0))) == list(case.rows)       # the empty scan is a scan of the plan
    y0 = op.run(x).clone()
    y1 = op.run(x).clone()
    assert torch.equal(y0, y1)                                                   # bitwise-equal reruns
    y = _np(y0)
    assert y.shape == (B, case.D) and np.isfinite(y).all()
    table, fails = [], []
    fails += H.check_stage(table, name, "eval", "y", y, want, ref32, np.arange(B), B)
    if name == "global_clamp":
        # scan 1's V is all zero: both norms clamp, vlad = 0 / 1e-12 / 1e-12 = 0 and the descriptor is bn2 of a zero row
        sc2, sh2 = op.ctx.bn_fold(op.bn2)
        assert torch.equal(y0[E.CLAMP_SCAN], torch.zeros_like(sc2) * sc2 + sh2)
    if name in E.PERMUTED_CASES:
        # the same scans under other batch indices (same Nmax): every scan's descriptor is bitwise the same
        perm = _perm(case)
        y2 = op.run(op.plan(coords, feats, order=list(perm)))
        assert torch.equal(y2[torch.from_numpy(perm).cuda()], y0)
    _report(table, fails)


# ------------------------------------------------------------------ train: egonn_netvlad_train_forward / _backward
def _core_step(gpu, nv, coords, feats, upstream, order=None):
    """tests/test_gpu_pooling_train.py's _step with NetVLADFn alone in place of netvlad_pool: y is the (B, D) product before bn2,
    `upstream` its gradient; only the parameters and buffers NetVLADFn touches are returned"""
    from egonn_amd import train
    B = len(coords)
    order = list(range(B)) if order is None else [int(o) for o in order]
    ctx = gpu._lib.Context(torch.device("cuda", 0))
    c4 = np.concatenate([np.c_[np.full(len(c), order[b], np.int32), c] for b, c in enumerate(coords)])
    ctx.coords_set(torch.from_numpy(c4).cuda(), B)
    idx = ctx.input_index()
    x = ctx.gather_input(torch.from_numpy(np.concatenate(feats)).cuda()).requires_grad_(True)
    nv.zero_grad(set_to_none=True)
    y = train.NetVLADFn.apply(x, nv.cluster_weights, nv.cluster_weights2, nv.bn1.weight, nv.bn1.bias, nv.hidden1_weights, ctx, 0,
                              nv.bn1)
    up = torch.empty_like(y)
    up[torch.tensor(order, device="cuda")] = torch.from_numpy(np.asarray(upstream, dtype=np.float32)).cuda()
    (y * up).sum().backward()
    gx = torch.empty_like(x)
    gx[idx] = x.grad
    grads = {k: p.grad.detach().clone() for k, p in nv.named_parameters() if p.grad is not None}
    bufs = {k: v.detach().clone() for k, v in nv.state_dict().items() if k.startswith("bn1.") and ("running" in k or "num_" in k)}
    return y.detach()[torch.tensor(order, device="cuda")], gx, grads, bufs


def _tensors(run):
    out = {"y": run[0], "grad x": run[1]}
    out.update({"grad " + k: v for k, v in run[2].items()})
    out.update({"buf " + k: v for k, v in run[3].items() if "running" in k})
    return out


@pytest.mark.parametrize("name,mode", E.TRAIN_RUNS)
def test_netvlad_train_edges_match_float64(gpu, name, mode):
    """mode `train`: netvlad_pool (NetVLADFn, bn2, gating); mode `core`: NetVLADFn alone, for the cases netvlad_pool refuses.
    Both clamp cases: the reference (tests/golden/netvlad_train_edges.npz) divides by the clamped eps as by a constant, so the
    gradient of the all-zero scan is dvlad / 1e-12 (cluster_clamp, cluster 3) or dvlad / 1e-24 (global_clamp) and is not zero;
    grad x of that scan is held to the same bound as every other scan, in its own scale (1e10 and 1e24).  In cluster_clamp and
    cluster_clamp_tiny that column also dominates max |grad cluster_weights2|, so the other 63 columns are compared once more on
    their own.  cluster_clamp_tiny's clamped column is not zero: there the clamp decides the values (see the case table)."""
    case = E.BY_NAME[name]
    B = len(case.rows)
    want, ref32 = (E.train_tensors(r) for r in E.reference(name, mode))
    state = E.state(case, mode)
    coords, feats, up = _coords(case), E.features(case, mode), E.upstream(case)
    step = _step if mode == "train" else _core_step
    runs = [step(gpu, _module(state, case.C, case.D, case.gating), coords, feats, up) for _ in range(2)]
    got, again = _tensors(runs[0]), _tensors(runs[1])
    assert set(got) == set(want)
    for k in got:
        assert torch.isfinite(got[k]).all(), k
        assert torch.equal(got[k], again[k]), k                                 # bitwise-equal reruns
    assert int(runs[0][3]["bn1.num_batches_tracked"]) == 1
    table, fails = [], []
    scans = {"y": np.arange(B), "grad x": _scan_of_rows(case)}
    for k in want:
        g = _np(got[k]).reshape(want[k].shape)
        fails += H.check_stage(table, name, mode, k, g, want[k], ref32[k], scans.get(k, np.zeros(0)), B)
    if name in ("cluster_clamp", "cluster_clamp_tiny"):
        keep = np.arange(64) != E.CLAMP_CLUSTER
        k = "grad cluster_weights2"
        fails += H.check_stage(table, name, mode, k + " (k != 3)", _np(got[k]).reshape(want[k].shape)[..., keep],
                               want[k][..., keep], ref32[k][..., keep], np.zeros(0), B)
    if name in E.PERMUTED_CASES:
        # the same scans under other batch indices (same Nmax): per-scan grad x bitwise, everything else within the bounds
        other = step(gpu, _module(state, case.C, case.D, case.gating), coords, feats, up, order=_perm(case))
        assert torch.equal(other[1], runs[0][1])
        o = {"y": other[0], **{"grad " + k: v for k, v in other[2].items()}}
        for k in o:
            fails += H.check_stage(table, name, mode, k + " (permuted)", _np(o[k]).reshape(want[k].shape), want[k], ref32[k],
                                   scans.get(k, np.zeros(0)), B)
    _report(table, fails)


@pytest.mark.parametrize("name", E.REFUSED_CASES)
def test_netvlad_pool_refuses_a_wide_output_dim_before_it_steps_bn1(gpu, name):
    """train mode with output_dim > 256 is unsupported by design (BatchNormFn's egonn_col_stats holds at most 256 columns): status
    1 (EGONN_ERR_INVALID), raised before NetVLADFn has updated bn1's running statistics or counted the batch"""
    from egonn_amd._lib import EgonnError
    case = E.BY_NAME[name]
    nv = _module(E.state(case, "core"), case.C, case.D, case.gating)
    before = {k: v.detach().clone() for k, v in nv.state_dict().items()}
    with pytest.raises(EgonnError, match="unsupported") as e:
        _step(gpu, nv, _coords(case), E.features(case, "core"), E.upstream(case))
    assert e.value.code == 1
    for k, v in nv.state_dict().items():
        assert torch.equal(v, before[k]), k

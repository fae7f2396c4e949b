"""GPU tests of MinkLoc's pooling (run with -m gpu on an MI355X): NetVLAD / NetVLAD-GC (egonn_netvlad), MAC
(egonn_global_max_pool) and SPoC end to end against the reference graph's fixtures, the reference's zero-padding rule,
the operator against the float64 restatement of tests/test_netvlad_host.py at product sizes, determinism / batch-order
invariance / graph replay, and the argument checks."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_netvlad_host import POOLING_CASES, PREFIX, netvlad_f64

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


def _minkloc(gpu, name):
    case = H.load_case(name)
    mp = gpu.ModelParams(model="MinkLoc", coordinates="cartesian", quantization_step=0.3, block=str(case["block"]),
                         pooling=str(case["pooling"]), output_dim=int(case["output_dim"]))
    m = gpu.model_factory(mp)
    w = H.seeded_weights(case["weight_seed"], name)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return case, m.to("cuda").eval()


def _check(g, want):
    assert g.shape == want.shape
    assert H.cosine_err(g, want).max() < 1e-4
    np.testing.assert_allclose(g, want, rtol=1e-3, atol=1e-4)


# ------------------------------------------------------------------ 1. end to end vs the reference graph
@pytest.mark.parametrize("name", POOLING_CASES)
def test_minkloc_pooling_matches_reference_graph(gpu, name):
    case, m = _minkloc(gpu, name)
    c4 = case["coords"]
    order = np.random.default_rng(3).permutation(len(c4))
    y = m({"coords": torch.from_numpy(c4[order]), "features": torch.ones((len(c4), 1))})
    assert set(y.keys()) == {"global"}
    _check(_np(y["global"]), case["global"])


# ------------------------------------------------------------------ 2. the reference's zero padding to Nmax
def test_netvlad_pad_rule(gpu):
    case, m = _minkloc(gpu, "minkloc_netvladgc_cart03")
    s = int(case["alone_scan"])
    c4 = case["coords"]
    batched = _np(m({"coords": torch.from_numpy(c4), "features": torch.ones((len(c4), 1))})["global"])
    one = c4[c4[:, 0] == s].copy()
    one[:, 0] = 0
    alone = _np(m({"coords": torch.from_numpy(one), "features": torch.ones((len(one), 1))})["global"])
    _check(batched, case["global"])
    _check(alone, case["global_alone"])
    assert np.abs(alone[0] - batched[s]).max() > 1e-4          # the pad term is reproduced, not dropped


# ------------------------------------------------------------------ 3./4. the operator on a seeded plan
ROWS = [1, 3100, 50, 777, 2500, 129, 128, 256, 1900, 10, 3000, 640, 17, 2049, 400, 1200]     # B = 16, ragged


def _scan_coords(rng, n):
    """n distinct voxel coordinates of one scan"""
    flat = rng.choice(64 * 64 * 16, size=n, replace=False)
    return np.stack([flat // (64 * 16) - 32, (flat // 16) % 64 - 32, flat % 16 - 8], axis=1).astype(np.int32)


def _batch(rows, seed, c):
    rng = np.random.default_rng(seed)
    coords = [_scan_coords(rng, n) for n in rows]
    feats = [rng.standard_normal((n, c)).astype(np.float32) for n in rows]
    return coords, feats


def _weights(c, d, gating, seed=5):
    from egonn_amd.synth import seeded_tensor
    shapes = {"cluster_weights": (c, 64), "cluster_weights2": (1, c, 64), "hidden1_weights": (c * 64, d)}
    for bn, n in (("bn1", 64), ("bn2", d)) + ((("context_gating.bn1", d),) if gating else ()):
        shapes.update({f"{bn}.weight": (n,), f"{bn}.bias": (n,), f"{bn}.running_mean": (n,), f"{bn}.running_var": (n,)})
    if gating:
        shapes["context_gating.gating_weights"] = (d, d)
    return {PREFIX + k: seeded_tensor(seed, PREFIX + k, s) for k, s in shapes.items()}


def _bn_module(w, prefix):
    n = w[prefix + "weight"].shape[0]
    bn = torch.nn.BatchNorm1d(n).eval().cuda()
    bn.load_state_dict({k: torch.from_numpy(w[prefix + k]) for k in ("weight", "bias", "running_mean", "running_var")},
                       strict=False)
    return bn


class _Op:
    """egonn_netvlad on a plan built from per-scan coordinates (scan b gets batch index order[b])"""

    def __init__(self, gpu, c, d, gating):
        self.ctx = gpu._lib.Context(torch.device("cuda", 0))
        self.c, self.d, self.gating = c, d, gating
        self.w = _weights(c, d, gating)
        t = lambda k: torch.from_numpy(self.w[PREFIX + k]).cuda()            # noqa: E731
        self.args = [t("cluster_weights"), t("cluster_weights2"), _bn_module(self.w, PREFIX + "bn1."),
                     t("hidden1_weights"), _bn_module(self.w, PREFIX + "bn2.")]
        self.args += [t("context_gating.gating_weights"), _bn_module(self.w, PREFIX + "context_gating.bn1.")] if gating \
            else [None, None]

    def plan(self, coords, feats, order=None):
        order = list(range(len(coords))) if order is None else order
        c4 = np.concatenate([np.c_[np.full(len(c), order[b], np.int32), c] for b, c in enumerate(coords)])
        f = np.concatenate(feats)
        self.ctx.coords_set(torch.from_numpy(c4).cuda(), len(coords))
        return self.ctx.gather_input(torch.from_numpy(f).cuda())              # plan row order

    def run(self, x):
        return self.ctx.netvlad(0, x, *self.args)


@pytest.mark.parametrize("c,d,gating", [(64, 128, False), (64, 256, True), (256, 128, True), (256, 256, False)])
def test_netvlad_operator_matches_f64_restatement(gpu, c, d, gating):
    op = _Op(gpu, c, d, gating)
    coords, feats = _batch(ROWS, 11 + c + d, c)
    x = op.plan(coords, feats)
    off = op.ctx.level_batch_offsets(0)
    assert np.array_equal(np.diff(off), ROWS)
    y = _np(op.run(x))
    want = netvlad_f64(_np(x), off, op.w, gating)
    rel = np.linalg.norm(y - want, axis=1) / np.linalg.norm(want, axis=1)
    assert y.shape == (len(ROWS), d) and np.isfinite(y).all()
    assert rel.max() < 1e-5, rel


def test_netvlad_deterministic_order_invariant_and_graph_replay(gpu):
    op = _Op(gpu, 256, 256, True)
    coords, feats = _batch(ROWS, 7, 256)
    x = op.plan(coords, feats)
    y0 = op.run(x).clone()
    y1 = op.run(x).clone()
    assert torch.equal(y0, y1)                                              # bitwise-equal reruns
    # eager vs a captured replay of the pooling call (one stream)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        yg = op.run(x)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(yg, y0)
    # the same scans in another batch order (same Nmax): every scan's descriptor is bitwise the same
    perm = np.random.default_rng(2).permutation(len(ROWS))
    x2 = op.plan(coords, feats, order=list(perm))
    y2 = op.run(x2)
    assert torch.equal(y2[torch.from_numpy(perm).cuda()], y0)


# ------------------------------------------------------------------ 5. argument checks
def test_netvlad_argument_checks(gpu):
    from egonn_amd._lib import EgonnError
    for c, d in ((72, 128), (64, 8), (64, 24), (64, 1040)):
        op = _Op(gpu, c, d, True)
        coords, feats = _batch([5, 9], 3, c)
        x = op.plan(coords, feats)
        with pytest.raises(EgonnError, match="unsupported") as e:
            op.run(x)
        assert e.value.code == 1                                             # EGONN_STATUS_INVALID

"""GPU tests of the streaming form of the 1x1-convolution kernel (dense_stream_kernel, egonn_amd/csrc/dense.hip), run with -m gpu on
an MI355X through egonn_debug_dense: the streaming form gathering the caller's weights (form 1), the streaming form on the packed
fragments of egonn_dense_pack_fragments, and the persistent LDS kernel it replaces (form 0) must give np.array_equal rows, for
both weight layouts and for the fp32 and bf16 map combinations the forward uses, on the four channel plans of the forward:
    32 -> 64 and 64 -> 128  BatchNorm + gated residual (the tails of levels 2 and 4)
    128 -> 64               plain (the local head's level-4 lateral)
    64 -> 64                residual without a gate (the unfused level-3 lateral)
Row counts: 8 192 is the smallest capacity that reaches these kernels; 8 193 and 8 207 end in a ragged tile.  The streaming form
gives every wave exactly ONE tile (its grid is ceil(tiles / 4) workgroups of four waves, from the capacity alone), so no wave takes
a tile more than another and none loops; what its grid rule does produce, a last workgroup with idle waves, is the 513 tiles of
capacity 8 207 (three idle waves) and the 8 193 case.  Device row counts below the capacity leave a canary in every row from n_dev
on.  Scan boundaries: B = 1, a boundary inside the first tile plus an empty scan, a boundary on a multiple of 16, 16 uneven scans;
gates differ per scan and column.  Reruns are bitwise, and a scan's rows are bitwise the same alone and inside a batch.

Value check: one case per plan against the float64 restatement relu(t2 * g + ((y @ Wd) * scale + shift)) (the plain and ungated
plans: their own expression), bound 8 x e_ref where e_ref is the error of the same restatement in float32 numpy against float64
on the same inputs (the factor of tests/test_gpu_netvlad_edges.py: another summation order, not another algorithm); nothing in
the bound comes from the kernels' output.  The ratios e_gpu / e_ref are printed."""
import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

# name -> cin, cout, folded BatchNorm, residual, gate, (in, residual, out) bf16 flags of the forward under EGONN_FLAG_BF16
PLANS = {
    "32-64-bn-gated": (32, 64, True, True, True, (1, 1, 1)),
    "64-128-bn-gated": (64, 128, True, True, True, (1, 1, 1)),
    "128-64-plain": (128, 64, False, False, False, (1, 0, 1)),
    "64-64-residual": (64, 64, False, True, False, (1, 1, 0)),
}
CAP = 8207


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    g.build()
    import egonn_amd
    return egonn_amd


_DATA = {}


def _data(plan, B=16):
    """host inputs of a plan, made once: rows for the largest capacity, one gate row per scan of the largest batch"""
    key = (plan, B)
    if key not in _DATA:
        cin, cout, bn, res, gate, _ = PLANS[plan]
        rng = np.random.default_rng(1000 + cin * 7 + cout)
        d = {"x": rng.standard_normal((CAP, cin)).astype(np.float32),
             "w": (rng.standard_normal((cin, cout)) / np.sqrt(cin)).astype(np.float32),
             "scale": rng.uniform(0.5, 1.5, cout).astype(np.float32) if bn else None,
             "shift": rng.standard_normal(cout).astype(np.float32) if bn else None,
             "res": rng.standard_normal((CAP, cout)).astype(np.float32) if res else None,
             "gate": rng.uniform(0.05, 0.95, (B, cout)).astype(np.float32) if gate else None}
        for v in d.values():
            if v is not None:
                v.setflags(write=False)
        _DATA[key] = d
    return _DATA[key]


def _dev(a, bf16=False):
    if a is None:
        return None
    t = torch.from_numpy(np.array(a, order="C")).cuda()          # (a row-major copy: the shared inputs are read-only)
    return t.to(torch.bfloat16) if bf16 else t


def _bits(t):
    """the rows as integers: bitwise comparison also of NaN-free bf16 maps"""
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)).cpu().numpy()


def _run(gpu, plan, cap, n_live, boff, flags=(0, 0, 0), out_in=False, forms=("stream", "packed", "lds"), data=None, gate_rows=None):
    """-> {form: (out tensor, canary tensor)} of one case; n_live None = no device count"""
    L = gpu._lib
    cin, cout, bn, res, gate, _ = PLANS[plan]
    d = data or _data(plan)
    x = _dev(d["x"][:cap], flags[0])
    r = _dev(d["res"][:cap], flags[1]) if res else None
    w = _dev(d["w"].T if out_in else d["w"])
    g = None
    bo = None
    if gate:
        g = _dev(d["gate"][:len(boff) - 1] if gate_rows is None else gate_rows)
        bo = torch.tensor(boff, dtype=torch.int32, device="cuda")
    nd = None if n_live is None else torch.tensor([n_live], dtype=torch.int32, device="cuda")
    packed = L.dense_pack_fragments(w, out_in)
    outs = {}
    for f in forms:
        out = torch.full((cap, cout), -12345.0, device="cuda", dtype=torch.bfloat16 if flags[2] else torch.float32)
        canary = out.clone()
        L.debug_dense(x, w, out_in, out, 0 if f == "lds" else 1, n_dev=nd, packed=packed if f == "packed" else None,
                      scale=_dev(d["scale"]), shift=_dev(d["shift"]), residual=r, gate=g, boff=bo)
        outs[f] = (out, canary)
    torch.cuda.synchronize()
    return outs


def _same(outs, n_live, what):
    ref = _bits(outs["lds"][0])
    for f, (out, canary) in outs.items():
        got = _bits(out)
        assert np.array_equal(got[:n_live], ref[:n_live]), f"{what}: form {f} differs from the persistent kernel"
        assert np.array_equal(got[n_live:], _bits(canary)[n_live:]), f"{what}: form {f} wrote rows from n_dev = {n_live} on"
    assert n_live == 0 or not np.array_equal(ref[:n_live], _bits(outs["lds"][1])[:n_live]), f"{what}: nothing was computed"


def _boff(B, n):
    """B uneven scans over n rows"""
    rng = np.random.default_rng(B * 31 + n)
    cuts = np.sort(rng.choice(np.arange(1, n), B - 1, replace=False)) if B > 1 else np.zeros(0, dtype=np.int64)
    return [0] + [int(c) for c in cuts] + [n]


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("bf16", [False, True])
def test_forms_bitwise_over_layouts_and_capacities(gpu, plan, bf16):
    flags = PLANS[plan][5] if bf16 else (0, 0, 0)
    for cap in (8192, 8193, 8207):
        for out_in in (False, True):
            outs = _run(gpu, plan, cap, None, _boff(3, cap), flags, out_in)
            _same(outs, cap, f"{plan} bf16={bf16} capacity {cap} out_in={out_in}")


@pytest.mark.parametrize("plan", list(PLANS))
def test_device_count_below_capacity_keeps_the_canary(gpu, plan):
    for bf16 in (False, True):
        flags = PLANS[plan][5] if bf16 else (0, 0, 0)
        for n_live in (0, 1, 15, 16, 17, CAP - 5):
            boff = [0, min(7, n_live), min(7, n_live), n_live]
            outs = _run(gpu, plan, CAP, n_live, boff, flags)
            _same(outs, n_live, f"{plan} bf16={bf16} n_dev={n_live}")


@pytest.mark.parametrize("plan", ["32-64-bn-gated", "64-128-bn-gated"])
def test_scan_boundaries(gpu, plan):
    cases = {"B=1": [0, CAP], "first tile + empty scan": [0, 7, 7, CAP], "multiple of 16": [0, 4096, CAP], "B=16 uneven": _boff(16, CAP)}
    d = _data(plan)
    for name, boff in cases.items():
        outs = _run(gpu, plan, CAP, CAP, boff)
        _same(outs, CAP, f"{plan} {name}")
        # a wrong scan index changes the rows: the float32 restatement with the right scan of every row is close, and the
        # restatement with every scan index shifted by one is not (gates differ per scan and column)
        scan = np.repeat(np.arange(len(boff) - 1), np.diff(boff))
        got = outs["stream"][0].cpu().numpy()
        z = (d["x"] @ d["w"]) * d["scale"] + d["shift"]
        want = np.maximum(d["res"] * d["gate"][scan] + z, 0)
        assert H.rel_err(got, want) < 1e-5, f"{plan} {name}: rows do not follow their scan's gate"
        if len(boff) > 2:
            wrong = np.maximum(d["res"] * d["gate"][(scan + 1) % (len(boff) - 1)] + z, 0)
            assert H.rel_err(wrong, want) > 1e-2


@pytest.mark.parametrize("plan", list(PLANS))
def test_rerun_and_scan_alone_bitwise(gpu, plan):
    boff = [0, 1000, 5003, CAP]
    a = _run(gpu, plan, CAP, CAP, boff, forms=("stream", "packed"))
    b = _run(gpu, plan, CAP, CAP, boff, forms=("stream", "packed"))
    for f in a:
        assert np.array_equal(_bits(a[f][0]), _bits(b[f][0])), f"{plan}: form {f} is not bitwise repeatable"
    d = _data(plan)
    for s in range(3):
        lo, hi = boff[s], boff[s + 1]
        alone = {k: None if v is None else v[lo:hi] for k, v in d.items() if k in ("x", "res")}
        pad = lambda v: None if v is None else np.concatenate([v, np.zeros((8192 - len(v), v.shape[1]), np.float32)])  # noqa: E731
        one = dict(d, x=pad(alone["x"]), res=pad(alone.get("res")))
        grow = None if d["gate"] is None else d["gate"][s:s + 1]
        outs = _run(gpu, plan, 8192, hi - lo, [0, hi - lo], forms=("stream", "packed"), data=one, gate_rows=grow)
        for f in outs:
            assert np.array_equal(_bits(outs[f][0])[:hi - lo], _bits(a[f][0])[lo:hi]), f"{plan}: scan {s} alone differs from the batch ({f})"


@pytest.mark.parametrize("plan", list(PLANS))
def test_values_against_float64(gpu, plan):
    cin, cout, bn, res, gate, _ = PLANS[plan]
    d = _data(plan)
    boff = _boff(16, CAP)
    scan = np.repeat(np.arange(16), np.diff(boff))

    def restate(dt):
        z = d["x"].astype(dt) @ d["w"].astype(dt)
        if bn:
            z = z * d["scale"].astype(dt) + d["shift"].astype(dt)
        if gate:
            return np.maximum(d["res"].astype(dt) * d["gate"].astype(dt)[scan] + z, 0)
        return z + d["res"].astype(dt) if res else z

    want, ref32 = restate(np.float64), restate(np.float32)
    assert ref32.dtype == np.float32
    e_ref = H.rel_err(ref32, want)
    outs = _run(gpu, plan, CAP, CAP, boff)
    for f, (out, _) in outs.items():
        e_gpu = H.rel_err(out.cpu().numpy(), want)
        print(f"ratio {plan:<18}{f:<8} e_ref {e_ref:.3e} e_gpu {e_gpu:.3e} ratio {e_gpu / e_ref:.2f}")
        assert e_gpu <= 8.0 * e_ref, f"{plan} form {f}: {e_gpu:.3e} above 8 x e_ref = {8 * e_ref:.3e}"


def test_device_packer_equals_host_packer(gpu):
    rng = np.random.default_rng(5)
    for cin in (32, 64, 128):
        for cout in (64, 128):
            for out_in in (False, True):
                w = rng.standard_normal((cout, cin) if out_in else (cin, cout)).astype(np.float32)
                host = gpu._lib.dense_pack_fragments(w, out_in)
                dev = gpu._lib.dense_pack_fragments(torch.from_numpy(w).cuda(), out_in).cpu().numpy()
                assert np.array_equal(host.view(np.int32), dev.view(np.int32)), f"{cin}->{cout} out_in={out_in}"

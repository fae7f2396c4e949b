"""GPU tests of the tail of the global head (run with -m gpu on an MI355X): the descriptor decoder (Linear 128 -> 192 + ReLU,
Linear 192 -> 256) with the global pooling, as the three launches of the unfused path (form 0 of egonn_debug_global_tail:
dense_small_kernel, dense_lds_kernel, segment_partial_kernel) and as the one fused launch (form 1: global_tail_kernel,
egonn_amd/csrc/global_tail.hip); and the grouped lateral launch of MinkHead on packed fragments against the raw kernels.

Rows per scan.  The pooling cuts every scan into SEG_CHUNKS = 32 chunks and the fused kernel walks a chunk in 16-row tiles, so:
[0] and [1] (all chunks empty / all but one), [31, 32, 33] (one chunk empty, every chunk one row, one chunk two rows),
[7, 0, 16, 17] (an empty scan between others), [511, 512, 513, 1100] (chunks of 15 / 16, 16, 16 / 17 and 34 / 35 rows: a tile that is
exactly full, a second tile of one row, three tiles), 16 uneven scans, and a live count below the capacity with NaN in every row
from the live count on (a NaN read anywhere would reach the output through the MFMA or the sums).  Inputs and decoder outputs have
both signs, so the GeM clamp acts.  GeM, MAC and SPoC are covered everywhere.

Assertions: form 1 equals form 0 bitwise in `partial` and in the pooled output; a rerun is bitwise the same; a scan alone equals
the same scan inside a batch; values against a float64 numpy restatement with the rule of tests/test_gpu_dense_stream.py:
e_gpu <= 8 x e_ref, e_ref being the error of the same restatement in float32 numpy (another summation order, not another algorithm;
nothing in the bound comes from the kernels' output), ratios printed.  Laterals: packed-fragment results of the grouped launch are
bitwise those of egonn_dense on the raw kernel.  End to end: 4 scans of 5 000 points extract bitwise equal outputs (fp32 and bf16
maps) with each new measurement switch on and off, one child process per setting (the switches are read once per process)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("EGONN_NO_FUSED_GTAIL", "EGONN_NO_PACKED_LATERALS")


def _child():
    """one setting of the switches (from the environment): digests of everything a packed extraction returns, per precision"""
    sys.path.insert(0, REPO)
    import torch
    import __graft_entry__ as g
    g.build()
    import egonn_amd as E
    from egonn_amd.synth import lidar_scan, seeded_state_dict
    m = E.model_factory(E.ModelParams(model="egonn", coordinates="cartesian", quantization_step=0.1))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(7, shapes).items()})
    m = m.to("cuda").eval()
    scans = [lidar_scan(300 + i, 5000) for i in range(4)]
    off = [0]
    for s in scans:
        off.append(off[-1] + len(s))
    pts = torch.from_numpy(np.concatenate(scans)).cuda()
    for prec in ("fp32", "bf16"):
        m.precision = prec
        out = E.DescriptorExtractor(m, n_k=128).extract_packed(pts, off)
        h = hashlib.sha256()
        for k in ("global", "keypoints", "descriptors", "rows"):
            h.update(out[k].cpu().numpy().tobytes())
        assert np.isfinite(out["global"].cpu().numpy()).all()
        print("DIGEST", prec, h.hexdigest())


if __name__ == "__main__":
    _child()
    sys.exit(0)

import torch  # noqa: E402

from tests import helpers as H  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {
    "[0]": ([0], 1),
    "[1]": ([1], 0),
    "[31,32,33]": ([31, 32, 33], 0),
    "[7,0,16,17]": ([7, 0, 16, 17], 0),
    "[511,512,513,1100]": ([511, 512, 513, 1100], 0),
    "16 uneven": ([int(v) for v in np.random.default_rng(16).integers(0, 200, 16)], 0),
    "live below capacity": ([40, 3, 100], 37),
}                            # name -> rows per scan, rows of capacity beyond the live count (NaN)
MODES = ("GeM", "MAC", "SPoC")
ROWS = max(sum(r) for r, _ in CASES.values())


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    g.build()
    import egonn_amd
    return egonn_amd


_HOST = {}


def _host():
    """rows and decoder, made once and read-only"""
    if not _HOST:
        rng = np.random.default_rng(2024)
        d = {"x": rng.standard_normal((ROWS, 128)).astype(np.float32),
             "w0": (rng.standard_normal((192, 128)) / np.sqrt(128)).astype(np.float32),
             "b0": (0.1 * rng.standard_normal(192)).astype(np.float32),
             "w1": (rng.standard_normal((256, 192)) / np.sqrt(192)).astype(np.float32),
             "b1": (0.1 * rng.standard_normal(256)).astype(np.float32),
             "p": np.array([3.0], np.float32)}
        for v in d.values():
            v.setflags(write=False)
        _HOST.update(d)
    return _HOST


_DEV = {}


def _dev():
    if not _DEV:
        _DEV.update({k: torch.from_numpy(np.array(v)).cuda() for k, v in _host().items() if k != "x"})
    return _DEV


def _bits(t):
    return t.view(torch.int32).cpu().numpy()


def _run(gpu, rows, pad, mode, form, x=None):
    """-> (partial, out) of one call on the first sum(rows) rows of x, followed by `pad` NaN rows"""
    n = sum(rows)
    x = _host()["x"] if x is None else x
    g5 = np.full((max(n + pad, 1), 128), np.nan, np.float32)
    g5[:n] = x[:n]
    boff = torch.tensor(np.concatenate([[0], np.cumsum(rows)]), dtype=torch.int32, device="cuda")
    nd = torch.tensor([n], dtype=torch.int32, device="cuda")
    d = _dev()
    part, out = gpu._lib.debug_global_tail(torch.from_numpy(g5).cuda(), boff, nd, d["w0"], d["b0"], d["w1"], d["b1"], d["p"], mode, form)
    torch.cuda.synchronize()
    return part, out


def _restate(dt, rows, mode):
    """pooled (B, 256) in the numpy type dt; an empty scan pools to 0 (the finish kernels' rule)"""
    h = _host()
    n = sum(rows)
    x = h["x"][:n].astype(dt)
    hid = np.maximum(x @ h["w0"].astype(dt).T + h["b0"].astype(dt), 0)
    y = hid @ h["w1"].astype(dt).T + h["b1"].astype(dt)
    p = h["p"].astype(dt)[0]
    out = np.zeros((len(rows), 256), dt)
    lo = 0
    for b, r in enumerate(rows):
        if r:
            s = y[lo:lo + r]
            if mode == "GeM":
                out[b] = np.power(np.power(np.maximum(s, dt(1e-6)), p).mean(axis=0), dt(1) / p)
            else:
                out[b] = s.max(axis=0) if mode == "MAC" else s.mean(axis=0)
        lo += r
    assert out.dtype == dt
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(CASES))
def test_fused_equals_three_launches_bitwise(gpu, case, mode):
    rows, pad = CASES[case]
    p0, o0 = _run(gpu, rows, pad, mode, 0)
    p1, o1 = _run(gpu, rows, pad, mode, 1)
    assert np.array_equal(_bits(p1), _bits(p0)), f"{case} {mode}: partial sums differ"
    assert np.array_equal(_bits(o1), _bits(o0)), f"{case} {mode}: pooled output differs"
    assert np.isfinite(o1.cpu().numpy()).all(), f"{case} {mode}: a row beyond the live count was read"
    if sum(rows) > 1:
        assert np.abs(o1.cpu().numpy()).max() > 0, f"{case} {mode}: nothing was computed"
    ident = -np.inf if mode == "MAC" else 0.0              # chunks without rows hold the identity
    lens = np.array([[(r * (c + 1)) // 32 - (r * c) // 32 for c in range(32)] for r in rows])
    assert (p1.cpu().numpy()[lens == 0] == ident).all(), f"{case} {mode}: an empty chunk does not hold the identity"


@pytest.mark.parametrize("mode", MODES)
def test_rerun_bitwise(gpu, mode):
    for case in ("[511,512,513,1100]", "16 uneven"):
        rows, pad = CASES[case]
        a, b = _run(gpu, rows, pad, mode, 1), _run(gpu, rows, pad, mode, 1)
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1])), f"{case} {mode}: not repeatable"


@pytest.mark.parametrize("mode", MODES)
def test_scan_alone_equals_scan_in_batch(gpu, mode):
    x = _host()["x"]
    for case in ("[7,0,16,17]", "[511,512,513,1100]"):
        rows, _ = CASES[case]
        part, out = _run(gpu, rows, 0, mode, 1)
        lo = 0
        for b, r in enumerate(rows):
            pa, oa = _run(gpu, [r], 0, mode, 1, x=x[lo:lo + r] if r else x)
            assert np.array_equal(_bits(pa[0]), _bits(part[b])), f"{case} {mode}: scan {b} alone has other partial sums"
            assert np.array_equal(_bits(oa[0]), _bits(out[b])), f"{case} {mode}: scan {b} alone pools differently"
            lo += r


@pytest.mark.parametrize("mode", MODES)
def test_values_against_float64(gpu, mode):
    for case in ("[31,32,33]", "[511,512,513,1100]", "16 uneven"):
        rows, pad = CASES[case]
        want, ref32 = _restate(np.float64, rows, mode), _restate(np.float32, rows, mode)
        e_ref = H.rel_err(ref32, want)
        for form in (0, 1):
            e_gpu = H.rel_err(_run(gpu, rows, pad, mode, form)[1].cpu().numpy(), want)
            print(f"ratio {case:<20}{mode:<5} form {form} e_ref {e_ref:.3e} e_gpu {e_gpu:.3e} ratio {e_gpu / e_ref:.2f}")
            assert e_gpu <= 8.0 * e_ref, f"{case} {mode} form {form}: {e_gpu:.3e} above 8 x e_ref = {8 * e_ref:.3e}"


def test_laterals_on_packed_fragments_equal_the_raw_kernel(gpu):
    """three (n, 128) @ (128, 128) products of one grouped launch reading packed fragments against egonn_dense on the raw
    (cin, cout) kernels, over row counts on both sides of the 64-row workgroup and with live counts below the capacity"""
    L = gpu._lib
    rng = np.random.default_rng(77)
    ws = [torch.from_numpy((rng.standard_normal((128, 128)) / np.sqrt(128)).astype(np.float32)).cuda() for _ in range(3)]
    for counts, caps in (((0, 1, 65), (0, 1, 65)), ((64, 128, 1), (64, 128, 1)), ((65, 0, 130), (70, 9, 192))):
        xs = [torch.from_numpy(rng.standard_normal((max(c, 1), 128)).astype(np.float32)).cuda() for c in caps]
        for packed in (True, False):
            outs = L.debug_dense_group3(xs, list(caps), list(counts), ws, packed)
            torch.cuda.synchronize()
            for q in range(3):
                n = counts[q]
                want = torch.empty((n, 128), device="cuda")
                if n:
                    L.call(xs[q].device, L.load().egonn_dense, xs[q].data_ptr(), n, 128, ws[q].data_ptr(), 0, None, 128, 0, want.data_ptr())
                torch.cuda.synchronize()
                assert np.array_equal(_bits(outs[q][:n]), _bits(want)), f"rows {counts} capacity {caps} packed={packed}: product {q} differs"
                assert (outs[q][n:] == -12345.0).all().item(), f"rows {counts} capacity {caps} packed={packed}: product {q} wrote past its live count"


def test_extraction_bitwise_with_each_switch():
    digests = {}
    for name in (None,) + SWITCHES:
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        if name:
            env[name] = "1"
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, env=env, cwd=REPO)
        lines = sorted(l for l in r.stdout.splitlines() if l.startswith("DIGEST"))
        assert r.returncode == 0 and len(lines) == 2, r.stderr[-2000:]
        digests[name] = lines
        print(name, lines)
    for name in SWITCHES:
        assert digests[name] == digests[None], f"{name}=1 changes the extraction's bits"

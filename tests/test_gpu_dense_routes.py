"""GPU tests of the 1x1-layer kernels below the 8192 rows of tests/test_gpu_dense_stream.py (egonn_amd/csrc/dense.hip), run with -m gpu
on an MI355X through egonn_debug_dense with form 0: there only the whole forward exercised their epilogue options.  Shapes are the
smallest at which each kernel can go wrong (which kernel a shape gets is pinned by tests/test_dense_route_host.py, not here):
    small kernel          64 -> 100 (a ragged last column tile), both weight layouts, 1 / 15 / 16 / 17 / 63 / 64 / 65 rows
    64-column tile kernel 192 -> 256 at 65 and 2047 rows
    persistent LDS kernel 192 -> 256 (two column blocks of 128) and 256 -> 256 (three of 96, the last one ragged: 64 columns)
    with column blocks    at 2048 and 2049 rows (a ragged last tile)
    thread per output     48 -> 3 at 65 rows, bias and activation only
Options: each of the three MFMA kernels runs what the forward asks of a 1x1 layer — bias + ReLU (the decoders), folded BatchNorm
(the downsample branches), an fp32 residual (the laterals), and under EGONN_FLAG_BF16 bf16 input rows with a bf16 output, with
BatchNorm, or with a bf16 residual and an fp32 or bf16 output — and one case with a device row count below the capacity and a
canary in every row from n_dev on.

Value check (as tests/test_gpu_dense_stream.py): |got - want| <= 8 x e_ref against the float64 restatement `want` of the layer on
the values the kernel reads (bf16 operands rounded first), where e_ref is the largest error of the same restatement in float32
numpy on the same inputs — another summation order, not another algorithm; nothing in the bound comes from the kernels' output.
A bf16 output adds the rounding of the store, elementwise 2^-8 |want|: bf16 keeps 8 significant bits, so round to nearest errs by
at most half an ulp, which is at most 2^-8 of the value (reached just above a power of two: the printed ratios of the bf16 cases
sit at 0.99 of the bound, those of the fp32 cases below 0.6).  The restatement is made once per plan and option on the plan's largest row count;
smaller row counts are checked against its first rows.  The ratios are printed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# option -> bias, activation, folded BatchNorm, residual, (in, residual, out) bf16
OPTIONS = {
    "bias-relu": (True, 1, False, False, (0, 0, 0)),
    "bn": (False, 0, True, False, (0, 0, 0)),
    "residual": (False, 0, False, True, (0, 0, 0)),
    "bf16-in-out": (False, 0, False, False, (1, 0, 1)),
    "bn-bf16-in-out": (False, 0, True, False, (1, 0, 1)),
    "bf16-residual-f32-out": (False, 0, False, True, (1, 1, 0)),
    "bf16-residual-bf16-out": (False, 0, False, True, (1, 1, 1)),
}
# plan -> cin, cout, largest row count
PLANS = {"small": (64, 100, 65), "tile": (192, 256, 2047), "lds-2-blocks": (192, 256, 2049), "lds-3-blocks": (256, 256, 2049),
         "plain": (48, 3, 65)}
CANARY = -12345.0


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    g.build()
    import egonn_amd
    return egonn_amd


def _bf16(a):
    """float32 array rounded to bf16 (round to nearest even, as torch), as float32"""
    return torch.from_numpy(np.array(a, order="C")).to(torch.bfloat16).to(torch.float32).numpy()


_DATA, _REF = {}, {}


def _data(plan):
    if plan not in _DATA:
        cin, cout, rows = PLANS[plan]
        rng = np.random.default_rng(2000 + cin * 7 + cout)
        d = {"x": rng.standard_normal((rows, cin)).astype(np.float32),
             "w": (rng.standard_normal((cin, cout)) / np.sqrt(cin)).astype(np.float32),
             "bias": rng.standard_normal(cout).astype(np.float32),
             "scale": rng.uniform(0.5, 1.5, cout).astype(np.float32),
             "shift": rng.standard_normal(cout).astype(np.float32),
             "res": rng.standard_normal((rows, cout)).astype(np.float32)}
        for v in d.values():
            v.setflags(write=False)
        _DATA[plan] = d
    return _DATA[plan]


def _act(z, act):
    return np.maximum(z, 0) if act == 1 else (np.tanh(z) if act == 2 else z)


def _reference(plan, option):
    """-> (want float64, e_abs = largest |float32 restatement - want|) on the plan's largest row count, made once"""
    key = (plan, option) if isinstance(option, str) else (plan,) + option
    if key not in _REF:
        bias, act, bn, res, flags = OPTIONS[option] if isinstance(option, str) else option
        d = _data(plan)
        x = _bf16(d["x"]) if flags[0] else d["x"]
        r = _bf16(d["res"]) if flags[1] else d["res"]

        def restate(dt):
            z = x.astype(dt) @ d["w"].astype(dt)
            if bias:
                z = z + d["bias"].astype(dt)
            if bn:
                z = z * d["scale"].astype(dt) + d["shift"].astype(dt)
            z = _act(z, act)
            return z + r.astype(dt) if res else z

        want, ref32 = restate(np.float64), restate(np.float32)
        assert ref32.dtype == np.float32 and want.dtype == np.float64
        want.setflags(write=False)
        _REF[key] = (want, float(np.abs(ref32 - want).max()))
    return _REF[key]


def _run(gpu, plan, option, rows, out_in=False, n_live=None):
    """one launch on the first `rows` rows of the plan's data into a buffer full of CANARY -> out as float64 numpy"""
    bias, act, bn, res, flags = OPTIONS[option] if isinstance(option, str) else option
    d = _data(plan)
    cout = PLANS[plan][1]
    dev = lambda a, bf=0: torch.from_numpy(np.array(a, order="C")).cuda().to(torch.bfloat16 if bf else torch.float32)  # noqa: E731
    out = torch.full((rows, cout), CANARY, device="cuda", dtype=torch.bfloat16 if flags[2] else torch.float32)
    nd = None if n_live is None else torch.tensor([n_live], dtype=torch.int32, device="cuda")
    gpu._lib.debug_dense(dev(d["x"][:rows], flags[0]), dev(d["w"].T if out_in else d["w"]), out_in, out, 0, n_dev=nd,
                         bias=dev(d["bias"]) if bias else None, scale=dev(d["scale"]) if bn else None,
                         shift=dev(d["shift"]) if bn else None, act=act, residual=dev(d["res"][:rows], flags[1]) if res else None)
    torch.cuda.synchronize()
    return out.to(torch.float64).cpu().numpy()


def _check(got, plan, option, what):
    flags = (OPTIONS[option] if isinstance(option, str) else option)[4]
    want, e_abs = _reference(plan, option)
    want = want[:got.shape[0]]
    err = np.abs(got - want)
    bound = 8.0 * e_abs + (2.0 ** -8 * np.abs(want) if flags[2] else 0.0)
    print(f"ratio {what:<58} e_ref {e_abs:.3e} e_gpu {err.max():.3e} largest err / bound {float((err / bound).max()):.3f}")
    assert np.all(err <= bound), f"{what}: error {err.max():.3e}, {float((err / bound).max()):.2f} x the bound (8 x e_ref = {8 * e_abs:.3e})"


@pytest.mark.parametrize("out_in", [False, True])
def test_small_kernel_row_counts_and_layouts(gpu, out_in):
    for rows in (1, 15, 16, 17, 63, 64, 65):
        for option in ("bias-relu", "residual"):
            _check(_run(gpu, "small", option, rows, out_in), "small", option, f"small {option} rows {rows} out_in={out_in}")


@pytest.mark.parametrize("plan,row_counts", [("small", (65,)), ("tile", (65, 2047)), ("lds-2-blocks", (2048, 2049)),
                                             ("lds-3-blocks", (2048, 2049))])
def test_epilogue_options(gpu, plan, row_counts):
    for rows in row_counts:
        for option in OPTIONS:
            _check(_run(gpu, plan, option, rows), plan, option, f"{plan} {option} rows {rows}")


def test_column_blocks_with_the_linear_layout(gpu):
    for plan in ("tile", "lds-2-blocks", "lds-3-blocks"):
        rows = PLANS[plan][2]
        _check(_run(gpu, plan, "bn", rows, out_in=True), plan, "bn", f"{plan} bn rows {rows} out_in=True")


@pytest.mark.parametrize("plan,n_live", [("small", 17), ("tile", 1000), ("lds-2-blocks", 2040), ("lds-3-blocks", 1), ("plain", 17)])
def test_device_count_below_capacity_keeps_the_canary(gpu, plan, n_live):
    rows = PLANS[plan][2]
    options = [(True, 2, False, False, (0, 0, 0))] if plan == "plain" else ["residual", "bf16-residual-bf16-out"]
    for option in options:
        got = _run(gpu, plan, option, rows, n_live=n_live)
        bf16_out = isinstance(option, str) and OPTIONS[option][4][2]
        canary = float(torch.tensor(CANARY).to(torch.bfloat16)) if bf16_out else CANARY
        assert np.all(got[n_live:] == canary), f"{plan} {option}: rows from n_dev = {n_live} on were written"
        assert not np.any(got[:n_live] == canary), f"{plan} {option}: a live row was not written"
        _check(got[:n_live], plan, option, f"{plan} {option} n_dev {n_live} of {rows}")


def test_thread_per_output_kernel(gpu):
    for act in (0, 1, 2):                    # none, ReLU, tanh (the keypoint regressor's)
        for bias in (False, True):
            option = (bias, act, False, False, (0, 0, 0))
            _check(_run(gpu, "plain", option, 65), "plain", option, f"plain bias={bias} act={act} rows 65")

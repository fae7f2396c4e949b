"""The sequence of library calls every model graph makes, recorded on the CPU against a fake library and compared
exactly with tests/golden/graph_calls.json.

Every call of the package goes through `_lib.call` (or a direct `check(lib.egonn_*(...))` for the entry points without a
stream), so a recording object in place of `Context.lib` sees the whole graph: the entry point, every integer and float
argument, and null / non-null for every pointer.  Tensor values are irrelevant (the fake computes nothing); the plan is a
fixed table of eight levels with two scans.

A pull request that changes a graph on purpose regenerates the file and shows the diff:

    python -m tests.test_graph_calls_host --write
"""
import ctypes as C
import json
import os
import sys
import types

import pytest
import torch

from egonn_amd import ModelParams, _lib, model_factory

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_calls.json")
ROWS, B = [40, 20, 10, 6, 4, 3, 2, 2], 2
CPU = torch.device("cpu")
_SIG = {name: args for name, _, args in _lib._SIGS}
_INTS = (C.c_int, C.c_int64, C.c_uint64)
_FLOATS = (C.c_float, C.c_double)


def _offsets(level):
    return [0, ROWS[level] // 2, ROWS[level]]


def _show(arg, argtype):
    if argtype in _INTS:
        return str(int(arg))
    if argtype in _FLOATS:
        return repr(float(arg))
    if argtype is C.c_char_p:
        return repr(arg.decode())
    if arg is None or (isinstance(arg, int) and arg == 0):
        return "-"
    if isinstance(arg, C.Array) and argtype is C.POINTER(C.c_float):        # the quantiser's step: an input
        return "[" + " ".join(repr(float(v)) for v in arg) + "]"
    return "p"


class FakeLib:
    """stands in for libegonn_hip: records every call, answers the plan queries from ROWS, returns status 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("egonn_"):
            raise AttributeError(name)
        argtypes = _SIG[name]

        def fn(*args):
            if name.endswith("_destroy"):
                return None
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            self.calls.append(f"{name}({','.join(_show(a, t) for a, t in zip(args, argtypes))})")
            if name == "egonn_level_count":
                args[2]._obj.value = ROWS[args[1]]
            elif name == "egonn_level_batch_offsets":
                args[2][:] = _offsets(args[1])
            elif name == "egonn_map_groups":
                args[3]._obj.value = (ROWS[args[2]] + 15) // 16
                args[4][:] = [0, 1, (ROWS[args[2]] + 15) // 16]
            return 0
        self.__dict__[name] = fn
        return fn


class _AsDevice:
    """a CPU tensor that answers is_cuda like the device tensor the plan entry points insist on"""
    is_cuda = True

    def __init__(self, t):
        self._t = t

    def __getattr__(self, k):
        return getattr(self._t, k)


def _context(lib):
    ctx = object.__new__(_lib.Context)          # no egonn_ctx_create
    ctx.lib, ctx.device, ctx.h, ctx.batch_size, ctx._keep = lib, CPU, 1, 0, []
    ctx.coords_set = lambda coords, bs: _lib.Context.coords_set(ctx, _AsDevice(coords), bs)
    return ctx


def _stand(model, lib, train):
    """the model on the CPU with the fake behind it"""
    ctxs = {}

    def context(slot=0):
        if slot not in ctxs:
            ctxs[slot] = _context(lib)
        return ctxs[slot]
    model._device = lambda: CPU
    model.context = context
    if train:       # MinkLoc refuses train-mode pooling other than GeM by the device of its parameters
        model.parameters = lambda: iter([types.SimpleNamespace(device=types.SimpleNamespace(type="cuda"))])
    return model.train() if train else model.eval()


def _batch():
    return {"coords": torch.zeros((ROWS[0], 4), dtype=torch.int32), "features": torch.ones((ROWS[0], 1)), "batch_size": B}


def _minkloc(lib, train, model="MinkLoc", **kw):
    if model == "MinkLoc":
        kw = dict(dict(planes=(32, 64, 64), layers=(1, 1, 1), num_top_down=1, block="BasicBlock", pooling="GeM"), **kw)
        kw["output_dim"] = 128 if kw["pooling"].startswith("netvlad") else 256
    m = _stand(model_factory(ModelParams(model=model, coordinates="cartesian", quantization_step=0.3, **kw)), lib, train)
    y = m(_batch())
    if train:
        y["global"].sum().backward()


def _egonn(lib, train, reserved=False, ignore_kp=False, precision="fp32", **kw):
    m = _stand(model_factory(ModelParams(model="egonn", coordinates="polar", quantization_step=[1.0, 0.3, 0.2])), lib, train)
    m.ignore_keypoint_regressor, m.precision = ignore_kp, precision
    m._handle, m._sync_weights = types.SimpleNamespace(h=2), lambda: None       # the weights are not registered
    if reserved:
        ctx = m.context()
        ctx.batch_size = B
        outs = tuple(torch.empty((n, c)) for n, c in ((B, 256), (ROWS[3], 128), (ROWS[3], 3), (ROWS[3], 1)))
        m._forward_on_plan(ctx, None, outputs=outs)
        return
    y = m(_batch(), **kw)
    if train:
        sum(t.sum() for v in y.values() for t in (v if isinstance(v, list) else [v])).backward()


def _cases():
    for mode in ("eval", "train"):
        train = mode == "train"
        for block in ("BasicBlock", "ECABasicBlock", "SEBasicBlock"):
            for ntd in (0, 1, 2, 3):
                yield f"minkloc/{block}/top_down{ntd}/{mode}", _minkloc, dict(train=train, block=block, num_top_down=ntd)
        yield f"minkloc/BasicBlock/layers211/{mode}", _minkloc, dict(train=train, layers=(2, 1, 1))
        for method in ("GeM", "MAC", "SPoC", "netvlad", "netvladgc"):
            yield f"minkloc/ECABasicBlock/{method}/{mode}", _minkloc, dict(train=train, block="ECABasicBlock", pooling=method)
    yield "minkloc3d/eval", _minkloc, dict(train=False, model="MinkLoc3D")
    yield "egonn/eval", _egonn, dict(train=False)
    yield "egonn/eval/disable_global_head", _egonn, dict(train=False, disable_global_head=True)
    yield "egonn/eval/disable_local_head", _egonn, dict(train=False, disable_local_head=True)
    yield "egonn/eval/ignore_keypoint_regressor", _egonn, dict(train=False, ignore_kp=True)
    yield "egonn/eval/bf16", _egonn, dict(train=False, precision="bf16")
    yield "egonn/eval/reserved", _egonn, dict(train=False, reserved=True)
    yield "egonn/train", _egonn, dict(train=True)
    yield "egonn/train/disable_local_head", _egonn, dict(train=True, disable_local_head=True)
    yield "egonn/train/disable_global_head", _egonn, dict(train=True, disable_global_head=True)


def record_all():
    """{case: [call, ...]} of every case"""
    out = {}
    stream = _lib._stream
    _lib._stream = lambda: 0                    # no HIP device: the null stream
    try:
        for name, run, kw in _cases():
            torch.manual_seed(0)
            lib = FakeLib()
            run(lib, **kw)
            out[name] = lib.calls
    finally:
        _lib._stream = stream
    return out


@pytest.fixture(scope="module")
def traces():
    return record_all()


_GOLDEN = {}
if os.path.exists(GOLDEN):
    with open(GOLDEN) as _f:
        _GOLDEN = json.load(_f)


def test_every_case_is_recorded_and_stored(traces):
    assert sorted(traces) == sorted(_GOLDEN)
    assert all(len(v) > 0 for v in traces.values())


@pytest.mark.parametrize("case", sorted(_GOLDEN))
def test_graph_calls_equal_the_stored_trace(traces, case):
    got, want = traces[case], _GOLDEN[case]
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, (f"{case}: {len(got)} calls, stored {len(want)}; first difference at call {first}: "
                         f"{got[first:first + 1]} vs {want[first:first + 1]}")


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    with open(GOLDEN, "w") as f:
        json.dump(record_all(), f, indent=0, sort_keys=True)
        f.write("\n")

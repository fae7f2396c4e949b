"""Host tests of the batched local-head loss (no GPU): the float64 restatement tests/local_loss_ref.py against REAL reference
outputs (tests/golden/local_losses.npz: the reference's own classes run in float64), the margins that make the GPU edge batches
unambiguous, and the C / Python surface of `egonn_local_loss`."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import local_loss_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CASES = ("a", "b", "c")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "local_losses.npz"))


def _pair(fx, name):
    return {k: fx[f"{name}_{k}"] for k in ("pc1", "pc2", "kp1", "kp2", "sigma1", "sigma2", "desc1", "desc2", "M")}


def _gammas(fx):
    return dict(zip(("gamma_chamfer", "gamma_p2p", "gamma_c", "gamma_k", "beta", "dist_th"), fx["gammas"].tolist()))


def _check_pair(fx, name, stats, grads, scale):
    """float64 against float64: the only differences are summation orders and the fixture's float32 gradient storage"""
    assert stats["loss"] == pytest.approx(float(fx[f"{name}_f64_loss_total"]), rel=1e-12)
    for k in R.STAT_KEYS:
        if k in ("loss", "kp_per_cloud"):
            continue
        # (the reference passes repeatability and the arg-max means through .float(): 2^-24 relative)
        assert stats[k] == pytest.approx(float(fx[f"{name}_f64_metric_{k}"]), rel=1.2e-7, abs=1e-13), (name, k)
    for k in R.GRAD_KEYS:
        want = fx[f"{name}_f64_grad_{k}"].astype(np.float64) * scale
        err = np.abs(grads[k] - want).max()
        assert err <= 2e-7 * np.abs(want).max() + 1e-12, (name, k, err)      # 2^-23 relative storage rounding, twice over


@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_matches_reference_pair(fx, name):
    r = R.pair_f64(_pair(fx, name), _gammas(fx))
    assert r["stats"]["kp_per_cloud"] == 0.5 * (len(fx[f"{name}_kp1"]) + len(fx[f"{name}_kp2"]))
    _check_pair(fx, name, r["stats"], r["grads"], 1.0)


def test_float64_restatement_matches_reference_batch(fx):
    b = R.batch_f64([_pair(fx, n) for n in CASES], _gammas(fx))
    assert b["loss"] == pytest.approx(np.mean([float(fx[f"{n}_f64_loss_total"]) for n in CASES]), rel=1e-12)
    for k in R.STAT_KEYS[2:]:
        assert b["stats"][k] == pytest.approx(np.mean([float(fx[f"{n}_f64_metric_{k}"]) for n in CASES]), rel=1.2e-7), k
    for i, n in enumerate(CASES):
        _check_pair(fx, n, b["pair_stats"][i], b["grads"][i], 1.0 / 3.0)


def test_edge_batches_are_unambiguous_in_float64():
    """integer-valued metrics are discontinuous: on the edge inputs every decision (nearest neighbour, inside dist_th, arg-max)
    must have a margin float32 cannot cross; planted exact duplicates are the one exception (ties -> lowest index)."""
    chunk = H.kernel_constant("LL_CLOUD_CHUNK")
    for name, (pairs, expect) in R.edge_batches(chunk).items():
        b = R.batch_f64(pairs, want_margins=True)
        for i, r in enumerate(b["pairs"]):
            mg = r["margins"]
            assert mg["nn"] > 1e-4, (name, i, mg)
            assert mg["dist_th"] > 1e-4, (name, i, mg)
            assert mg["top_logit"] > 1e-4, (name, i, mg)
        for (pi, side, k, row) in expect.get("plants", []):
            assert b["pairs"][pi]["i" + side][k] == row, (name, pi, side, k, row)
        if "kp_tie" in expect:
            pi, k, j = expect["kp_tie"]
            assert b["pairs"][pi]["ndx1"][k] == j and b["pairs"][pi]["keep"][k]
        if "zero_p2p" in expect:
            pi, side, k = expect["zero_p2p"]
            p = pairs[pi]
            assert np.array_equal(p["kp" + side][k], p["pc" + side][b["pairs"][pi]["i" + side][k]])
        if "nan_pair" in expect:
            i = expect["nan_pair"]
            assert not b["pairs"][i]["keep"].any() and np.isnan(b["loss"]) and np.isnan(b["pair_stats"][i]["loss"])
            assert all(np.isfinite(s["loss"]) for j, s in enumerate(b["pair_stats"]) if j != i)
            assert np.isnan(b["grads"][i]["desc1"]).all() and np.isfinite(b["grads"][i]["kp1"]).all()
        if "shared_pair" in expect:
            r = b["pairs"][expect["shared_pair"]]
            tg = r["ndx1"][r["keep"]]
            assert len(tg) - len(set(tg.tolist())) >= 3          # several kept rows share one class
    shapes = {len(p["kp1"]) for ps, _ in R.edge_batches(chunk).values() for p in ps} | \
             {len(p["kp2"]) for ps, _ in R.edge_batches(chunk).values() for p in ps}
    assert {1, 31, 32, 33, 63, 64, 65, 257} <= shapes
    clouds = {len(p[k]) for ps, _ in R.edge_batches(chunk).values() for p in ps for k in ("pc1", "pc2")}
    assert {1, chunk - 1, chunk, chunk + 1, 3 * chunk + 7} <= clouds


# ----------------------------------------------------------------------------- surface
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


def test_symbols_declared_and_exported(built):
    from egonn_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "egonn_hip.h")).read()
    for name in ("egonn_local_loss", "egonn_local_loss_scratch_bytes"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert f" {name}(" in header, name
    assert "EGONN_LOCAL_LOSS_STATS" in header
    assert H.kernel_constant("LL_STATS") == 16 and H.kernel_constant("LL_CLOUD_CHUNK") >= 64
    assert lib.egonn_local_loss_scratch_bytes(8, 7560, 7560, 128) > 0


def test_invalid_arguments_are_rejected_without_a_device(built):
    from egonn_amd import _lib
    lib = _lib.load()
    one = 256       # non-null, aligned, never dereferenced: every call below fails its argument check first
    params = (C.c_float * 6)(1, 1, 1, 1, 2, 0.5)
    big = 1 << 40

    def call(pairs=2, dim=128, totals=(100, 100, 10, 10), ptrs=None, params=params, grads=(one,) * 6, scratch=one, nbytes=big):
        ptrs = [one] * 13 if ptrs is None else ptrs
        return lib.egonn_local_loss(pairs, *totals, dim, *ptrs, params, one, one, *grads, scratch, nbytes, None)

    assert call(pairs=0) == 1 and b"pairs" in lib.egonn_last_error()
    assert call(dim=64) == 1 and b"width" in lib.egonn_last_error()
    assert call(totals=(100, 100, 0, 10)) == 1 and b"totals" in lib.egonn_last_error()
    for i in range(13):
        ptrs = [one] * 13
        ptrs[i] = None
        assert call(ptrs=ptrs) == 1 and b"null" in lib.egonn_last_error(), i
    assert call(params=None) == 1
    assert call(scratch=None) == 1
    assert call(grads=(one, None, one, one, one, one)) == 1 and b"together" in lib.egonn_last_error()
    assert call(nbytes=64) == 1 and b"scratch" in lib.egonn_last_error()
    assert call(scratch=one + 8) == 1 and b"aligned" in lib.egonn_last_error()
    ptrs = [one] * 13
    ptrs[6] = one + 4       # desc1
    assert call(ptrs=ptrs) == 1 and b"aligned" in lib.egonn_last_error()


def test_python_surface():
    import egonn_amd
    from egonn_amd import local_loss as L
    assert type(L.make_local_loss()) is L.KeypointCorrLoss                        # the default keeps today's object
    assert type(L.make_local_loss([1., 1., 1., 2.])) is L.KeypointCorrLoss
    b = L.make_local_loss(batched=True)
    assert type(b) is L.BatchedKeypointCorrLoss and b.gammas == (1., 1., 1., 1., 2., 0.5)
    assert L.BatchedKeypointCorrLoss(gamma_c=3., gamma_k=4., gamma_chamfer=5., gamma_p2p=6., beta=7., dist_th=8.).gammas == \
        (5., 6., 3., 4., 7., 8.)
    for name in ("BatchedKeypointCorrLoss", "local_loss_packed", "EgoNNTrainStep"):
        assert callable(getattr(egonn_amd, name)) and name in egonn_amd.__all__
    assert L.STAT_KEYS == R.STAT_KEYS and len(L.STAT_KEYS) <= L.LOCAL_LOSS_STATS == H.kernel_constant("LL_STATS")
    import torch
    z = torch.zeros
    with pytest.raises(RuntimeError, match="HIP device"):                         # no CPU path
        L.local_loss_packed(z(4, 3), z(2, dtype=torch.int32), z(2, 3), z(2, 1), z(2, 128), z(2, dtype=torch.int32),
                            z(4, 3), z(2, dtype=torch.int32), z(2, 3), z(2, 1), z(2, 128), z(2, dtype=torch.int32),
                            z(1, 4, 4), b.gammas)

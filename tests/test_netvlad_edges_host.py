"""CPU tests of the NetVLAD edge cases (tests/netvlad_edges_data.py): the table reaches every branch it is there for, the clamp
cases really clamp, the float64 restatements are finite on every case, float32 arithmetic alone stays under the discrimination
cap, and the restatement's clamp branch is the reference's (tests/golden/netvlad_train_edges.npz)."""
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import netvlad_edges_data as E
from tests.test_netvlad_host import PREFIX, netvlad_f64
from tests.test_netvlad_train_host import LIMIT, run_f64

E_REF_CAP = 1e-4           # the discrimination cap: 8 x e_ref of the device tests can never exceed 8e-4


def _guard(cases):
    """the properties the table must cover, computed from `cases` and the constants of kernels.h: the list of those missing"""
    cap, mc = E.CAP, E.MAX_CHUNKS
    rows = [n for c in cases for n in c.rows]
    batches = [len(c.rows) for c in cases]
    nd = {(c.D + 255) // 256 for c in cases}
    checks = {
        "a C in each dispatch range": {E.arm(c.C) for c in cases} == {0, 1, 2, 3},
        "the smallest C of each upper arm": {lim + 16 for lim in E.ARM_LIMITS[:3]} <= {c.C for c in cases},
        "a capped scan with uneven chunks": any(n > cap and E.nv_chunks(n) == mc and n % mc != 0 for n in rows),
        "a capped scan with uneven chunks on the <32,2> arm": any(E.arm(c.C) == 3 and n > cap and n % mc != 0
                                                                    for c in cases for n in c.rows),
        "scans of cap - 1, cap, cap + 1 rows": {cap - 1, cap, cap + 1} <= set(rows),
        "a 0-row scan": 0 in rows,
        "a 1-row scan": 1 in rows,
        "ceil(D / 256) = 1..4": nd >= {1, 2, 3, 4},
        "a ragged D above 256": any(c.D > 256 and c.D % 256 for c in cases),
        "B > 16, no multiple of 16": any(E.NV_BB < b < 2 * E.NV_BB and b % E.NV_BB for b in batches),
        "B > 32, no multiple of 16": any(2 * E.NV_BB < b <= E.FINISH_STRIDE and b % E.NV_BB for b in batches),
        "B > 256": any(b > E.FINISH_STRIDE for b in batches),
        "B = 1": 1 in batches,
        "gating at D = 1024": any(c.gating and c.D == 1024 for c in cases),
        "the per-cluster clamp": any(set(c.edit) == {"zero_scan", "w2_zero_cluster"} for c in cases),
        "the per-cluster clamp on a non-zero column": any(set(c.edit) == {"scale_scan", "w2_zero_cluster"} for c in cases),
        "the global clamp": any(set(c.edit) == {"zero_scan", "w2_zero"} for c in cases),
        "saturated logits": any("x_scale_eval" in c.edit and "bn1_weight_scale_train" in c.edit for c in cases),
    }
    return [k for k, ok in checks.items() if not ok]


def test_table_covers_every_edge():
    assert _guard(E.CASES) == []
    for c in E.CASES:
        assert c.C % 16 == 0 and 16 <= c.C <= 512 and c.D % 16 == 0 and 16 <= c.D <= 1024, c.name
        assert set(c.modes) <= {"eval", "train", "core"} and c.modes, c.name
        assert set(c.modes) == {"eval"} or len(c.rows) >= 2, c.name
        # netvlad_pool takes D <= TRAIN_MAX_D; a wider case runs NetVLADFn alone (and the device test asserts the refusal)
        assert ("train" in c.modes) <= (c.D <= E.TRAIN_MAX_D) and ("core" in c.modes) == (c.D > E.TRAIN_MAX_D), c.name
        assert max(c.rows) >= 1, c.name
    assert len({c.name for c in E.CASES}) == len(E.CASES) and len({c.seed for c in E.CASES}) == len(E.CASES)
    for name in E.PERMUTED_CASES + E.CLAMP_CASES:
        assert len(E.BY_NAME[name].modes) == 2                              # eval and a train step
    from egonn_amd import train
    assert E.TRAIN_MAX_D == train.BN_MAX_COLUMNS
    assert {E.BY_NAME[n].D for n in E.REFUSED_CASES} == {272, 528, 1024}    # ND = 2 ragged, 3 ragged, 4 reach the backward too
    assert any(0 in E.BY_NAME[n].rows for n in E.PERMUTED_CASES)          # the batch-order check moves an empty scan too


@pytest.mark.parametrize("name", [c.name for c in E.CASES])
def test_guard_misses_a_deleted_row(name):
    """the guard is not vacuous: without this row of the table a listed property is gone"""
    assert _guard([c for c in E.CASES if c.name != name]) != []


def test_nv_chunks_mirror_follows_the_header():
    """the chunk rule the table is built around, read from kernels.h and not restated as numbers"""
    with open(os.path.join(os.path.dirname(H.GOLDEN), "..", "egonn_amd", "csrc", "kernels.h")) as f:
        src = f.read()
    assert "(len + NV_CHUNK_ROWS - 1) / NV_CHUNK_ROWS" in src and "n < NV_MAX_CHUNKS ? n : NV_MAX_CHUNKS" in src
    assert E.nv_chunks(0) == 0 and E.nv_chunks(1) == 1 and E.nv_chunks(E.CHUNK_ROWS + 1) == 2
    assert E.nv_chunks(E.CAP - E.CHUNK_ROWS) == E.MAX_CHUNKS - 1 and E.nv_chunks(E.CAP) == E.nv_chunks(E.CAP + 1) == E.MAX_CHUNKS


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_clamp_cases_really_clamp(mode):
    """float64: the per-cluster norm of (cluster_clamp, scan 1, cluster 3) and the global norm of (global_clamp, scan 1) are
    exactly 0.0, that of (cluster_clamp_tiny, scan 1, cluster 3) lies in (1e-14, 0.5e-12): below the eps but not zero; every other
    norm of the cases is far above the eps 1e-12 (> 1e-6), so nothing sits near the threshold by accident.  In global_clamp all
    64 per-cluster norms of scan 1 are 0 as well: its whole V is."""
    s, k = E.CLAMP_SCAN, E.CLAMP_CLUSTER
    for name in E.CLAMP_CASES:
        case = E.BY_NAME[name]
        x, off, st = np.concatenate(E.features(case, mode)), E.offsets(case), E.state(case, mode)
        fold = E.train_fold(x, off, st) if mode == "train" else None
        _, nk, ng = E.eval_restated(x, off, st, case.gating, parts=True, fold=fold)
        others = np.ones(nk.shape, dtype=bool)
        if name == "cluster_clamp":
            assert nk[s, k] == 0.0
            others[s, k] = False
            assert ng.min() > 1e-6
        elif name == "cluster_clamp_tiny":
            assert 1e-14 < nk[s, k] < 0.5e-12                         # not zero, and a factor 2 at least below the eps
            others[s, k] = False
            assert ng.min() > 1e-6
        else:
            assert ng[s] == 0.0 and not nk[s].any()
            others[s, :] = False
            assert np.delete(ng, s).min() > 1e-6
        assert nk[others].min() > 1e-6, (name, float(nk[others].min()))


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_saturated_case_keeps_clear_of_the_eps(mode):
    """With logits of order 10^2 some clusters receive next to nothing and their columns of V have norms all the way down to
    1e-14: several fall below the eps (the clamp is live on non-zero columns here too), and none within 10 % of it, where fp32
    and float64 could take different branches."""
    case = E.BY_NAME["saturated"]
    x, off, st = np.concatenate(E.features(case, mode)), E.offsets(case), E.state(case, mode)
    _, nk, ng = E.eval_restated(x, off, st, case.gating, parts=True, fold=E.train_fold(x, off, st) if mode == "train" else None)
    assert (nk < 1e-12).any() and nk.min() > 0 and np.abs(nk / 1e-12 - 1.0).min() > 0.1 and ng.min() > 1.0


@pytest.mark.parametrize("name,mode", E.RUNS)
def test_restatements_are_finite_and_fp32_stays_under_the_cap(name, mode):
    """(`core`: NetVLADFn alone, y before bn2.)  Every float64 output, gradient and buffer is finite, and the same restatement in
    float32 on the CPU deviates from it by at most E_REF_CAP (max |a - b| / max |b| per tensor).  The cap is a condition on the
    CASES: the device tests allow 8 x e_ref, so a case on which fp32 arithmetic alone loses more than 1e-4 could hide a real error
    and has to be changed (more scans, another seed), not the cap.  Measured: at most 3.4e-5 (saturated, grad cluster_weights)."""
    r64, r32 = E.reference(name, mode)
    a, b = ({"y": r64}, {"y": r32}) if mode == "eval" else (E.train_tensors(r64), E.train_tensors(r32))
    case = E.BY_NAME[name]
    assert a["y"].shape == (len(case.rows), case.D)
    if mode != "eval":
        core = ("cluster_weights", "cluster_weights2", "hidden1_weights", "bn1")
        keys = [k for k in E.PARAM_KEYS if (case.gating or "gating" not in k) and (mode == "train" or k.split(".")[0] in core)]
        assert sorted(k[5:] for k in a if k.startswith("grad ") and k != "grad x") == sorted(keys)
    for k in a:
        assert np.isfinite(a[k]).all(), k
        e = H.rel_err(b[k], a[k])
        print(f"{name:<15}{mode:<6}{k:<40} e_ref {e:.2e}")
        assert e <= E_REF_CAP, (k, e)


def test_eval_restatement_is_netvlad_f64():
    """the torch restatement the e_ref comes from is the numpy one the fixtures pin (tests/test_netvlad_host.py)"""
    for name in ("arm_8", "chunk_cap", "global_clamp"):
        case = E.BY_NAME[name]
        x, off, st = np.concatenate(E.features(case, "eval")), E.offsets(case), E.state(case, "eval")
        want = netvlad_f64(x, off, {PREFIX + k: v for k, v in st.items()}, case.gating)
        np.testing.assert_allclose(E.reference(name, "eval")[0], want, rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("name", E.CLAMP_CASES)
def test_clamp_branch_of_the_restatement_matches_the_reference(name):
    """run_f64 against the reference's own NetVLADLoupe (float64, train mode, autograd on the zero-padded tensor) on the clamp
    cases, with the gates of test_restatement_matches_reference_fixture: rtol 1e-9, atol 1e-12 x max |ref| (grad x: per scan, so
    that the clamped scan's huge rows do not loosen the others).  This pins what "the projection term is dropped" means: the
    reference divides by the clamped eps as by a constant, so the zero column's gradient is dvlad / 1e-12 (cluster_clamp) and
    dvlad / 1e-24 (global_clamp) and is NOT zero: grad x of scan 1 is of the order 1e10 and 1e24.  In cluster_clamp_tiny the
    clamped column is not zero, so its values (V / 1e-12, of norm 0.17) and the missing projection term are both in the numbers.
    The empty scan of the other cases cannot be expressed in the reference (a scan without voxels does not exist in its batch); its
    meaning is the restatement's: a scan of Nmax pad rows."""
    fx = {k[len(name) + 1:]: v for k, v in H.load_case("netvlad_train_edges").items() if k.startswith(name + "/")}
    case = E.BY_NAME[name]
    feats, st, off = E.features(case, "train"), E.state(case, "train"), E.offsets(case)
    assert np.array_equal(fx["x"], np.concatenate(feats)) and np.array_equal(fx["offsets"], off)       # the fixture is this case
    assert np.array_equal(fx["upstream"], E.upstream(case)) and np.array_equal(fx["cluster_weights2"], st["cluster_weights2"])
    assert (int(fx["C"]), int(fx["D"]), int(fx["gating"]), int(fx["seed"])) == (case.C, case.D, int(case.gating), case.seed)
    y, gx, gp, bufs = run_f64(fx["x"], off, st, case.gating, fx["upstream"])

    def close(a, b, what):
        assert np.isfinite(b).all(), what
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-12 * float(np.abs(b).max()), err_msg=what)

    close(y, fx["out"], "out")
    for b in range(len(case.rows)):
        close(gx[off[b]:off[b + 1]], fx["grad_x"][off[b]:off[b + 1]], f"grad x of scan {b}")
    keys = [k for k in E.PARAM_KEYS if case.gating or "gating" not in k]
    assert sorted(k[5:] for k in fx if k.startswith("grad/")) == sorted(keys)
    for k in keys:
        close(gp[k], fx["grad/" + k], k)
    for k, v in bufs.items():
        close(v, fx["buf/" + k], k)
    s = E.CLAMP_SCAN
    assert float(np.abs(fx["grad_x"][off[s]:off[s + 1]]).max()) > 1e9             # divided by the eps, not dropped to zero
    assert os.path.getsize(os.path.join(H.GOLDEN, "netvlad_train_edges.npz")) <= LIMIT


def test_netvlad_pool_refuses_a_wide_output_dim_before_any_device_work():
    """train mode takes output_dim <= 256 (BatchNormFn's egonn_col_stats): a wider module is refused with status 1
    (EGONN_ERR_INVALID) before anything touches the device or bn1; B = 1 keeps nn.BatchNorm1d's ValueError"""
    import types
    import torch
    from egonn_amd import train
    from egonn_amd._lib import EgonnError
    from egonn_amd.model import NetVLADLoupe
    ctx = types.SimpleNamespace(batch_size=4)                # no device behind it: any device work would raise AttributeError
    for d in (272, 1024):
        nv = NetVLADLoupe(16, 64, d, gating=True)
        with pytest.raises(EgonnError, match=f"output_dim {d} unsupported") as e:
            train.netvlad_pool(ctx, 0, torch.zeros((5, 16)), nv)
        assert e.value.code == 1 and int(nv.bn1.num_batches_tracked) == 0
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        train.netvlad_pool(types.SimpleNamespace(batch_size=1), 0, torch.zeros((5, 16)), NetVLADLoupe(16, 64, 272))
    with pytest.raises(AttributeError):                      # 256 columns pass the check and go on to the device
        train.netvlad_pool(ctx, 0, torch.zeros((5, 16)), NetVLADLoupe(16, 64, 256))

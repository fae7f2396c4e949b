"""CPU tests of tests/icp_search_data.py: every geometry reaches the edge of the ICP grid search that it is there for (shown
with the grid restatement), the oracle agrees with evaluate_f64 of tests/test_icp_host.py, the planted ties are ties bit for
bit, and the winning squared distances and their sum are exact (shown in rational arithmetic), so that
tests/test_gpu_icp_search.py may compare the device with the oracle bit for bit.

evaluate_f64 asks its search for two neighbours: where more than two targets tie for the minimum it may name any of them, so
on those rows (they are planted: identical targets, cell corners and edges, lattice neighbours of a shifted lattice) its
choice has to be one of the tied targets, and j, n_corr and sum_d2 are compared everywhere else and in full respectively."""
from fractions import Fraction

import numpy as np
import pytest

from tests import icp_search_data as data
from tests.icp_plane_ref import knn_f64
from tests.test_icp_host import evaluate_f64, transform_f64


def _pairs(name):
    g = data.geometry(name)
    return [(g["srcs"][p], g["tgts"][p], g["T"][p], g["max_dist"][p], g["oracle"][p]) for p in range(len(g["srcs"]))]


def _d2(p, q):
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


# ------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("name", data.FINITE)
def test_oracle_equals_evaluate_f64(name):
    for src, tgt, T, md, o in _pairs(name):
        ev = evaluate_f64(src, tgt, T, md)
        assert ev["n_corr"] == o["n_corr"] and ev["sum_d2"] == o["sum_d2"], (name, ev["n_corr"], o["n_corr"])
        if len(src) == 0 or len(tgt) == 0:
            assert (o["j"] == -1).all() and o["n_corr"] == 0 and o["sum_d2"] == 0.0
            continue
        plain = o["mult"] <= 2
        assert np.array_equal(ev["j"][plain], o["j"][plain]) and np.array_equal(ev["nn"][plain], o["nn"][plain])
        assert np.array_equal(ev["d2"], o["d2"]) and np.array_equal(ev["j"] >= 0, o["j"] >= 0)
        p = transform_f64(T, src)
        assert np.array_equal(_d2(p, tgt[ev["nn"]]), o["d2"])                  # a tie of three or more: one of the tied targets


@pytest.mark.parametrize("name", data.FINITE)
def test_winning_distances_and_their_sum_are_exact(name):
    """in rational arithmetic: every winning d2 is the exact squared distance and sum_d2 is the exact sum, whatever the order"""
    F = Fraction
    for src, tgt, T, md, o in _pairs(name):
        total = F(0)
        for i in np.flatnonzero(o["nn"] >= 0):
            s, q = [F(float(v)) for v in src[i]], [F(float(v)) for v in tgt[o["nn"][i]]]
            p = [sum(F(float(T[r, c])) * s[c] for c in range(3)) + F(float(T[r, 3])) for r in range(3)]
            d2 = sum((p[k] - q[k]) ** 2 for k in range(3))
            assert F(float(o["d2"][i])) == d2, (name, i)
            if d2 < F(md) * F(md):
                assert o["j"][i] == o["nn"][i]
                total += d2
            else:
                assert o["j"][i] == -1
        assert F(o["sum_d2"]) == total, name
        # and the partial sums of a workgroup's tree stay exact: every term is a multiple of the smallest term's last bit
        assert total == 0 or total < 2 ** 40


def test_oracle_rules_on_a_handful_of_points():
    tgt = np.array([[0.0, 0.5, 0], [0.0, -0.5, 0], [5.0, 1.0, 0], [np.nan, 0, 0], [0.0, -0.5, 0]])
    src = np.array([[0.0, 0, 0], [5.0, 0, 0], [np.inf, 0, 0], [0.0, -0.5, 0]])
    o = data.oracle(src, tgt, np.eye(4), 1.0)
    assert o["j"].tolist() == [0, -1, -1, 1] and o["nn"].tolist() == [0, 2, -1, 1] and o["mult"].tolist() == [3, 1, 0, 2]
    assert o["n_corr"] == 2 and o["sum_d2"] == 0.25 and data.implied(o, 4) == (0.5, np.sqrt(0.125))
    assert data.oracle(src[:0], tgt, np.eye(4), 1.0)["n_corr"] == 0 and data.oracle(src, tgt[:0], np.eye(4), 1.0)["j"].tolist() == [-1] * 4
    assert data.oracle(src, tgt[3:4], np.eye(4), 1.0)["nn"].tolist() == [-1] * 4


# ------------------------------------------------------------------ every geometry reaches its edge
def test_sizes():
    ns, nt = {a for a, _ in data.SIZES}, {b for _, b in data.SIZES}
    assert ns == {1, 2, 3, 255, 256, 257, 513} and nt == {1, 255, 256, 257, 600}
    g = data.geometry("sizes")
    assert [(len(s), len(t)) for s, t in zip(g["srcs"], g["tgts"])] == data.SIZES
    assert any(0 < o["n_corr"] < len(o["j"]) for o in g["oracle"])              # both sides of the threshold
    assert any((o["mult"] > 1).any() for o in g["oracle"])


def test_one_cell_tiles():
    g = data.geometry("one_cell_tiles")
    src, tgt, T, md, o = _pairs("one_cell_tiles")[0]
    gr, rg, sh = data.shape_of(src, tgt, T, md)
    assert len(tgt) == 700 and len(src) == 64 and gr["dim"] == [1, 1, 1] and gr["ext"] < 0.25
    assert sh["ncol"] == 1 and sh["batches"] == 1 and sh["tiles"].tolist() == [3] and sh["points"] == 700
    p = transform_f64(T, src)
    for row, (a, b) in g["ties"].items():
        assert a < b and a // data.WG != b // data.WG                            # one cell: the visiting order is the index order
        assert _d2(p[row], tgt[a]).tobytes() == _d2(p[row], tgt[b]).tobytes() == o["d2"][row].tobytes()
        assert o["mult"][row] == 2 and o["j"][row] == a
    assert np.array_equal(tgt[5], tgt[650]) and o["d2"][0] == 0.0 and o["d2"][1] == 2.0 ** -14
    assert o["n_corr"] == 64 and len(set(o["j"].tolist())) > 40


@pytest.mark.parametrize("name", ["many_columns", "sparse_columns"])
def test_wide_planes(name):
    src, tgt, T, md, o = _pairs(name)[0]
    gr, rg, sh = data.shape_of(src, tgt, T, md)
    assert len(src) == 256 and gr["h"] == md == 1.0 and gr["dim"] == [95, 95, 1]
    assert rg == ([0, 0, 0], [94, 94, 0]) and sh["ncol"] == 9025 and sh["batches"] == 36 and sh["points"] == len(tgt)
    if name == "many_columns":
        assert len(tgt) == 27075 and sh["empty_columns"] == 0
        assert sh["per_batch"].min() > 0 and sh["per_batch"].max() == 768 and (sh["tiles"][:-1] == 3).all()       # tiles inside a batch
    else:
        assert len(tgt) == 2304 and sh["empty_columns"] == 9025 - 2304             # three columns in four are empty
        assert sh["per_batch"].max() <= 256 and (sh["per_batch"] > 0).all()
    assert 0 < o["n_corr"] < 256 and len(set(o["j"].tolist())) > 60
    # the cell order is not the index order (cells of edge 1: the key ascends with (x, y))
    assert (np.diff(tgt[:, 0] * 1024.0 + tgt[:, 1]) < 0).sum() > len(tgt) // 4


def test_cell_cap():
    g = data.geometry("cell_cap")
    src, tgt, T, md, o = _pairs("cell_cap")[0]
    gr, rg, sh = data.shape_of(src, tgt, T, md)
    assert md == 2.0 ** -10 and gr["ext"] == 96.0 and gr["h"] == gr["hmin"] > md                # the non-dyadic edge
    assert gr["dim"][0] in (data.CELL_MAX - 1, data.CELL_MAX) and gr["dim"][1:] == [1, 1]     # 2^16 - 1 cells: the cap
    assert rg[0] == [0, 0, 0] and rg[1] == [gr["dim"][0] - 1, 0, 0] and sh["batches"] == -(-gr["dim"][0] // 256) == 256
    assert sh["points"] == 400 and sh["empty_columns"] == gr["dim"][0] - 400
    d2 = o["d2"].reshape(3, 64)
    assert (d2[0] == 2.0 ** -22).all() and (d2[1] == 2.0 ** -20).all() and (d2[2] < 2.0 ** -20).all() and (d2[2] > 2.0 ** -21).all()
    j = o["j"].reshape(3, 64)
    assert (j[0] >= 0).all() and (j[1] == -1).all() and (j[2] >= 0).all() and o["n_corr"] == 128    # strict on both sides
    assert np.array_equal(tgt[o["nn"], 0], g["partner_x"]) and (o["mult"] == 1).all()


def test_outside():
    ps = _pairs("outside")
    shapes = [data.shape_of(src, tgt, T, md) for src, tgt, T, md, _ in ps]
    assert all(gr["dim"] == [5, 5, 5] and gr["h"] == 0.5 for gr, _, _ in shapes)
    (_, rg0, sh0), (_, rg1, sh1), (_, rg2, sh2), (_, rg3, sh3) = shapes
    lo, hi = data.source_box(ps[0][0], ps[0][2])
    assert (lo < -2.0).all() and (hi > 4.0).all() and rg0 == ([0, 0, 0], [4, 4, 4]) and sh0["points"] == 125      # clamped on six sides
    assert rg1[0][0] == 5 and sh1["ncol"] == 0 and rg2[1][0] == -1 and rg2[1][2] == -1 and sh2["ncol"] == 0     # no cell at all
    assert rg3 == ([3, 0, 0], [4, 4, 4]) and sh3["ncol"] == 10
    o0, o1, o2, o3 = (p[4] for p in ps)
    assert o1["n_corr"] == o2["n_corr"] == 0 and o3["n_corr"] == 9
    faces = o0["j"][:54].reshape(6, 3, 3)                                        # face, distance beyond it, position on it
    assert (faces[:, 0] >= 0).any(1).all() and (faces[:, 1:] == -1).all()        # 0.25 beyond: within reach of a face point
    assert (o0["d2"][:54].reshape(6, 3, 3)[:, 1] >= 0.5625).all()


def test_degenerate_extent():
    ps = _pairs("degenerate_extent")
    for k, (src, tgt, T, md, o) in enumerate(ps):
        gr, rg, sh = data.shape_of(src, tgt, T, md)
        assert gr["dim"] == [1, 1, 1] and gr["h"] == md and sh["ncol"] == 1, k
        assert (gr["ext"] == 0.0) == (k != 2)
    assert [len(p[1]) for p in ps] == [50, 1, 125, 3] and [p[3] for p in ps] == [0.5, 0.5, 512.0, 2.0 ** -12]
    assert (ps[0][4]["mult"] == 50).all() and set(ps[0][4]["j"].tolist()) == {0, -1} and ps[0][4]["j"].tolist() == ps[1][4]["j"].tolist()
    assert 0 < ps[2][4]["n_corr"] < len(ps[2][0]) and ps[2][4]["d2"].max() > 2.0 ** 17          # 512 m on a 1 m cloud
    assert ps[3][4]["j"].tolist() == [0, -1, -1, -1, -1] and ps[3][4]["d2"][1] == 2.0 ** -24 == ps[3][3] ** 2


def test_far_init():
    g = data.geometry("far_init")
    ps = _pairs("far_init")
    landed = transform_f64(g["T"][0], ps[0][0])
    assert np.array_equal(landed, transform_f64(g["T"][1], ps[1][0]))           # the pre-images are exact
    same = data.oracle(landed, ps[0][1], np.eye(4), ps[0][3])
    for k in (0, 1):
        assert np.array_equal(ps[k][4]["j"], same["j"]) and ps[k][4]["sum_d2"] == same["sum_d2"]
        assert not np.array_equal(g["T"][k][:3, :3], np.eye(3)) and abs(np.linalg.det(g["T"][k][:3, :3]) - 1.0) == 0.0
    assert ps[0][4]["n_corr"] == 125 - 42 and (ps[0][4]["d2"][::3] == 2.0 ** -16).all()        # every third row: exactly max_dist
    for k, sign in ((2, 1.0), (3, -1.0)):                                        # 2^17 cells off: the Morton key's clamp, no cell
        src, tgt, T, md, o = ps[k]
        gr, rg, sh = data.shape_of(src, tgt, T, md)
        f = np.floor((transform_f64(T, src) - gr["org"]) / gr["h"]) + 16384.0
        assert ((f > 1e5).any(1) if sign > 0 else (f < 0).any(1)).all() and sh["ncol"] == 0
        assert o["n_corr"] == 0 and (o["j"] == -1).all()


def test_cross_cell_ties():
    g = data.geometry("cross_cell_ties")
    src, tgt, T, md, o = _pairs("cross_cell_ties")[0]
    gr = data.grid(tgt, md)
    assert gr["h"] == 1.0 and gr["dim"] == [4, 4, 4] and len(src) <= 256
    assert np.array_equal(o["mult"], g["mult"]) and {2, 4, 8} == set(o["mult"].tolist()) and o["n_corr"] == len(src)
    cell = np.floor((tgt - gr["org"]) / gr["h"]).astype(np.int64)
    key = (cell[:, 0] << 32) | (cell[:, 1] << 16) | cell[:, 2]
    late = 0
    for i in range(len(src)):
        tied = np.flatnonzero(_d2(src[i], tgt) == o["d2"][i])
        assert len(tied) == o["mult"][i] and o["j"][i] == tied.min()
        assert len({_d2(src[i], tgt[t]).tobytes() for t in tied}) == 1 and len(set(key[tied].tolist())) == len(tied)     # different cells
        late += int(tied[np.argmin(key[tied])] != tied.min())                  # the first one visited is not the lowest index
    assert late >= len(src) // 3


def test_non_finite():
    g = data.geometry("non_finite")
    assert len(g["srcs"]) == 6
    for p in range(6):
        o, src, tgt = g["oracle"][p], g["srcs"][p], g["tgts"][p]
        clean = data.oracle(np.nan_to_num(src, nan=0.0, posinf=0.0, neginf=0.0), tgt, np.eye(4), 0.5)
        if g["bad_src"][p] is not None:
            r = g["bad_src"][p]
            assert (~np.isfinite(src)).sum() == 1 and np.isfinite(tgt).all() and o["j"][r] == -1 and o["nn"][r] == -1
            keep = np.arange(len(src)) != r
            assert np.array_equal(o["j"][keep], clean["j"][keep]) and o["n_corr"] == clean["n_corr"] - int(clean["j"][r] >= 0)
        else:
            r = g["bad_tgt"][p]
            assert (~np.isfinite(tgt)).sum() == 1 and np.isfinite(src).all() and not (o["j"] == r).any()
            whole = data.oracle(src, g["tgts"][0], np.eye(4), 0.5)
            assert (whole["j"] == r).any()                                     # a row would have chosen it
    vals = [g["srcs"][p][g["bad_src"][p]] for p in range(3)] + [g["tgts"][p][g["bad_tgt"][p]] for p in range(3, 6)]
    assert [float(v[~np.isfinite(v)][0]) for v in vals][1::3] == [np.inf, np.inf] and np.isnan(vals[0]).any() and np.isnan(vals[3]).any()
    assert [float(v[~np.isfinite(v)][0]) for v in vals][2::3] == [-np.inf, -np.inf]


def test_batch():
    g = data.geometry("batch")
    assert [len(s) for s in g["srcs"]] == data.BATCH_NS == [256, 0, 257, 1, 512, 3]
    assert [len(t) for t in g["tgts"]] == data.BATCH_NT == [5, 7, 0, 300, 257, 1]
    assert [o["n_corr"] > 0 for o in g["oracle"]] == [True, False, False, True, True, True]


def test_calls_cover_every_pair():
    for name in data.GEOMETRIES:
        ps = sorted(p for idx, _ in data.calls(name) for p in idx)
        assert ps == list(range(len(data.geometry(name)["srcs"])))
        for a in data.geometry(name)["srcs"] + data.geometry(name)["tgts"]:
            fin = a[np.isfinite(a)]
            assert np.array_equal(fin * 2.0 ** 30, np.round(fin * 2.0 ** 30)) and (np.abs(fin) <= 2.0 ** 10).all()        # dyadic


# ------------------------------------------------------------------ the kNN oracle
def test_knn_exact_is_knn_f64():
    """knn_f64 is brute force up to 1024 points: there the chunked oracle for the larger clouds has to give the same lists, ties
    included, and the lists of a smaller knn are prefixes of those of a larger one (what the GPU test relies on)"""
    tgt = data.geometry("one_cell_tiles")["tgts"][0]
    cap = data.geometry("cell_cap")["tgts"][0]
    plane = data.geometry("sparse_columns")["tgts"][0][:1000]
    for cloud in (tgt, cap, plane, tgt[:2], tgt[:20]):
        big = data.knn_exact(cloud, 32)
        for knn in (3, 20, 32):
            want, _ = knn_f64(cloud, knn)
            assert np.array_equal(data.knn_exact(cloud, knn), want)
            m = min(knn, len(cloud))
            assert np.array_equal(big[:, :m], want[:, :m])
    # beyond knn_f64's brute-force limit: against all pairs, stable in the index (the slabs of knn_exact are narrower than the cloud)
    whole = data.geometry("sparse_columns")["tgts"][0]
    d2 = _d2(whole[:, None, :], whole[None])
    assert np.array_equal(data.knn_exact(whole, 32), np.argsort(d2, axis=1, kind="stable")[:, :32])

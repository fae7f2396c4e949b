"""Host tests of the augmentation restatement (tests/augment_ref.py): against outputs of the reference's own classes
(tests/golden/augment_ref.npz, made by tests/golden/make_golden_augment.py with the restatement's draws patched into the
reference's generators), of the draws themselves, and of the checker the GPU tests rely on (it must accept the float64
answer and the fp32 restatement and reject planted errors).  No GPU."""
import os

import numpy as np
import pytest

from tests import augment_ref as R

U = R.U


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "augment_ref.npz"))


def _case(gold, ci):
    k = f"c{ci}_"
    mode, sid, seed, draw, set_id, on, flip = [int(v) for v in gold[k + "meta"]]
    P = R.Params(seed=seed, draw=draw, set_id=set_id, stages=(R.MODE1 if mode == 1 else R.MODE2) | (R.SET1 if mode == 1 else R.SET2))
    return k, mode, sid, P, bool(on), flip


def test_fixture_covers_what_it_must(gold):
    seen, flips = set(), set()
    for ci in range(int(gold["n_cases"])):
        _, mode, _, _, on, flip = _case(gold, ci)
        seen.add((mode, on))
        flips.add(flip)
    assert seen == {(1, True), (1, False), (2, True), (2, False)} and flips >= {0, 1, -1}


def test_restatement_against_the_reference_classes(gold):
    """discrete outcomes equal; block parameters within counted fp32 roundings; positions within the counted bound E (the
    3 x 3 product's order is BLAS's in the reference, hence a bound and not equality)"""
    for ci in range(int(gold["n_cases"])):
        k, mode, sid, P, on, flip = _case(gold, ci)
        pts = gold[k + "points"]
        n = len(pts)
        P1 = R.Params(**{**P.__dict__, "stages": P.stages & ~(R.SET_ROTATE | R.FLIP)})
        for dt in (np.float32, np.float64):
            r1 = R.augment(pts, [0, n], [sid], P1, dt)
            d = r1["scans"][0]
            assert d["k"] == int(n * d["r"]) == int(gold[k + "removed"].sum())
            assert np.array_equal(r1["removed"], gold[k + "removed"])
            assert d["block_on"] == on
            if on:
                bp = d["block"]
                x, y, w, h = gold[k + "block"]
                # x, y: a handful of fp32 roundings of values up to |min| + span; w, h: sqrt of an fp32 product of three roundings
                scale = np.abs(gold[k + "before_block"]).max()
                tol = (8 * U * scale + d["band"][0]) if dt == np.float64 else 8 * U * scale
                assert abs(float(bp["x0"]) - x) <= tol and abs(float(bp["y0"]) - y) <= tol
                assert abs(bp["w"] - w) <= 4 * U * w + (d["band"][0] if dt == np.float64 else 0)
                assert abs(bp["h"] - h) <= 4 * U * h + (d["band"][1] if dt == np.float64 else 0)
            shares = R.check(pts, [0, n], [sid], P1, gold[k + "stage1"], gold[k + "removed"], gold[k + "erased"])
            assert max(shares) <= 0.001
            r2 = R.augment(pts, [0, n], [sid], P, dt)
            assert r2["set"]["flip"] == flip
            same = r2["erased"] == gold[k + "erased"]
            err = np.abs(r2["out"].astype(np.float64) - gold[k + "stage2"]).max(axis=1)
            assert (err[same] <= 2 * r2["E"][same]).all(), (ci, dt, float((err[same] / r2["E"][same]).max()))
            assert (~same).sum() <= 0.001 * n


def test_rigid_against_apply_transform(gold):
    for ri in range(2):
        sid, seed, draw = [int(v) for v in gold[f"r{ri}_meta"]]
        P = R.Params(seed=seed, draw=draw, stages=R.RIGID, rot_max=np.pi, trans_max=5.0)
        pts = gold[f"r{ri}_points"]
        for dt in (np.float32, np.float64):
            r = R.augment(pts, [0, len(pts)], [sid], P, dt, T_in=gold[f"r{ri}_T_rel"][None])
            assert np.array_equal(r["scans"][0]["m"], gold[f"r{ri}_m"])          # the same fp32 cos, sin and shifts
            err = np.abs(r["out"].astype(np.float64) - gold[f"r{ri}_out"]).max(axis=1)
            assert (err <= 2 * r["E"]).all()
            # m @ T: 4-term fp32 dot products of entries <= 5 in magnitude, in BLAS's order there and ascending here
            assert np.abs(r["T_out"][0].astype(np.float64) - gold[f"r{ri}_T"]).max() <= 4 * U * 4 * 5 * 5


# ------------------------------------------------------------------ draws
def test_removed_set_has_exactly_k_distinct_members_and_is_uniform():
    n = 400
    hits = np.zeros(n)
    total = 0
    for sid in range(3000):
        P = R.Params(seed=5, draw=2, stages=R.REMOVE_POINTS)
        d = R.scan_draws(P, sid, n)
        assert d["removed"].sum() == d["k"] == int(n * d["r"]) and 0 <= d["r"] < 0.1
        hits += d["removed"]
        total += d["k"]
    # every index equally likely: hits_i ~ Binomial(3000, p ~ 0.05), sd ~ 12; 6 sd over 400 indices never trips by chance
    mean = total / n
    assert np.abs(hits - mean).max() < 6 * np.sqrt(mean)
    chi2 = ((hits - mean) ** 2 / mean).sum()
    assert chi2 < n + 6 * np.sqrt(2 * n)


def test_r_at_both_ends_of_its_range():
    for r, k in ((0.0, 0), (1.0, 777), (0.1, 77)):
        P = R.Params(seed=1, stages=R.REMOVE_POINTS, r_min=r, r_max=r)
        d = R.scan_draws(P, 3, 777)
        assert d["k"] == k == d["removed"].sum()
    assert R.scan_draws(R.Params(seed=1, stages=R.REMOVE_POINTS), 3, 5)["k"] == 0     # int(5 * r) = 0 for r < 0.1


def test_moments_of_uniforms_and_normals():
    i = np.arange(1_000_000, dtype=np.uint64)
    z = R.hash64(11, 1, 7, i, 0)
    u, g = R.uniform(z), R.normal(z)
    m = len(i)
    assert 0 <= u.min() and u.max() < 1 and abs(u.mean() - 0.5) < 5 / np.sqrt(12 * m) and abs(u.var() - 1 / 12) < 5e-4
    assert abs(g.mean()) < 5 / np.sqrt(m) and abs(g.var() - 1) < 5 * np.sqrt(2 / m)
    assert abs((g ** 3).mean()) < 5 * np.sqrt(15 / m) and abs((g ** 4).mean() - 3) < 5 * np.sqrt(96 / m)
    u24 = R.uniform24(z)
    assert u24.dtype == np.float32 and 0 <= u24.min() and u24.max() < 1 and abs(float(u24.mean()) - 0.5) < 2e-3


def test_distinct_scan_and_draw_give_distinct_streams():
    i = np.arange(4096, dtype=np.uint64)
    streams = {}
    for sid in (0, 1, 2, (1 << 22) - 1):
        for draw in (0, 1, (1 << 14) - 1):
            for slot in (0, 3):
                streams[(sid, draw, slot)] = R.hash64(9, draw, sid, i, slot)
    keys = list(streams)
    for a in range(len(keys)):
        for b in range(a + 1, len(keys)):
            assert (streams[keys[a]] == streams[keys[b]]).sum() == 0
            c = np.corrcoef(R.uniform(streams[keys[a]]), R.uniform(streams[keys[b]]))[0, 1]
            assert abs(c) < 6 / np.sqrt(len(i))
    with pytest.raises(AssertionError):
        R.hash64(9, 1 << 14, 0, i, 0)
    with pytest.raises(AssertionError):
        R.hash64(9, 0, 1 << 22, i, 0)
    with pytest.raises(AssertionError):
        R.hash64(9, 0, 0, np.array([1 << 24]), 0)


# ------------------------------------------------------------------ the checker
def gpu_inputs():
    """the inputs of the GPU tests' main comparison (tests/test_gpu_augment.py imports this)"""
    sizes = [5000, 0, 1, 256, 257, 4096, 12_345]
    pts, off = R.batch(42, sizes)
    ids = [7, 8, 1000, 5, (1 << 22) - 1, 0, 33]
    return pts, off, ids


def _block_seed(stages, on=True):
    """a seed whose scan 7 (the first, 5000 points) draws the block"""
    for seed in range(100):
        P = R.Params(seed=seed, draw=1, set_id=2, stages=stages)
        if (R.scan_draws(P, 7, 1)["block_u"] < P.block_p) == on:
            return P
    raise AssertionError


@pytest.mark.parametrize("stages", [R.MODE1 | R.SET1, R.MODE2 | R.SET2])
def test_checker_accepts_f64_and_f32_and_rejects_planted_errors(stages):
    pts, off, ids = gpu_inputs()
    P = _block_seed(stages)
    ref = R.augment(pts, off, ids, P, np.float64)
    r32 = R.augment(pts, off, ids, P, np.float32)
    assert max(R.check(pts, off, ids, P, ref["out"], ref["removed"], ref["erased"], ref=ref)) == 0
    shares = R.check(pts, off, ids, P, r32["out"], r32["removed"], r32["erased"], ref=ref)
    assert max(shares) <= 0.001                      # the excused share of the fp32 restatement stays under the cap
    d = ref["scans"][0]
    assert d["block_on"] and ref["erased"][:5000].sum() > 10

    def rejected(out, removed, erased, what):
        with pytest.raises(R.Mismatch):
            R.check(pts, off, ids, P, out, removed, erased, ref=ref)
            pytest.fail(f"the checker accepted: {what}")

    # one extra removed point
    i = int(np.nonzero(~ref["removed"][:5000] & ~ref["erased"][:5000])[0][0])
    rm = r32["removed"].copy()
    rm[i] = True
    rejected(r32["out"], rm, r32["erased"], "one extra removed point")
    # a point on the wrong side of a block edge: well inside the block but kept
    xy, _ = R.stage1_xy(pts, off, ids, P, 0)
    bp = d["block"]
    inside = np.nonzero(ref["erased"][:5000])[0]
    depth = np.minimum.reduce([xy[inside, 0] - float(bp["x0"]), float(bp["x1"]) - xy[inside, 0],
                               xy[inside, 1] - float(bp["y0"]), float(bp["y1"]) - xy[inside, 1]])
    j = int(inside[np.argmax(depth)])
    er = r32["erased"].copy()
    er[j] = False
    rejected(r32["out"], r32["removed"], er, "a row deep inside the block not erased")
    # the wrong flip axis
    wrong = r32["out"].copy()
    fl = ref["set"]["flip"]
    if fl >= 0:
        wrong[:, fl] = -wrong[:, fl]
    wrong[:, (fl + 1) % 3 if fl >= 0 else 0] *= -1
    rejected(wrong, r32["removed"], r32["erased"], "the wrong flip axis")
    # a jitter beyond the clip: 0.2 + 1e-3 on one coordinate of one kept point
    far = r32["out"].copy()
    far[i, 2] += np.float32(1e-3)
    rejected(far, r32["removed"], r32["erased"], "a jitter beyond the clip")
    # a translation applied before the removal: the removed points sit at 0 (turned by the later stages) instead of at t
    early = r32["out"].copy()
    only_removed = ref["removed"] & ~ref["erased"]
    assert only_removed.sum() > 0
    early[only_removed] = 0
    rejected(early, r32["removed"], r32["erased"], "a translation applied before the removal")


def test_removed_points_move_with_the_translation_and_enter_the_box():
    pts, off, ids = gpu_inputs()
    P = R.Params(seed=3, stages=R.REMOVE_POINTS | R.TRANSLATE | R.BLOCK)
    r = R.augment(pts, off, ids, P, np.float32)
    d = r["scans"][0]
    t = d["trans"].astype(np.float32)
    rm = r["removed"][:5000] & ~r["erased"][:5000]
    assert rm.sum() > 0 and (r["out"][:5000][rm] == t).all()


def test_records_layout():
    pts, off, ids = gpu_inputs()
    P = _block_seed(R.MODE2 | R.SET1)
    r = R.augment(pts, off, ids, P, np.float32)
    ri, rd = R.records(r, P)
    assert ri.shape == (7, 8) and rd.shape == (7, 32) and ri[:, 0].tolist() == [5000, 0, 1, 256, 257, 4096, 12_345]
    assert ri[1, 1] == 0 and ri[1, 2] == 0 and ri[0, 2] == 1 and (ri[:, 5] == ids).all()

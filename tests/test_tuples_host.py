"""CPU tests of the training-tuple path (egonn_amd/tuples.py, csrc/tuples.hip): the new C entries are declared and exported
and refuse bad arguments before any launch, the Python surface refuses them before it asks for a device, the pickles round
trip (the reference's class path included), `BatchSampler` keeps the contract of datasets/samplers.py:47-137, and every
numpy restatement of a kernel rule (tests/tuples_data.py) reproduces the fixture written from the reference's own functions
(tests/golden/make_golden_tuples.py).  Nothing here needs a GPU."""
import ctypes as C
import os
import pickle
import pickletools
import re

import numpy as np
import pytest

from tests import tuples_data as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["egonn_radius_count", "egonn_radius_fill", "egonn_pair_masks", "egonn_relative_poses", "egonn_gather_clouds"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from egonn_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def fx():
    return D.load_fixture()


# ----------------------------------------------------------------------------- the C ABI
def test_symbols_declared_and_exported(lib):
    from egonn_amd import _lib
    header = open(os.path.join(REPO, "include", "egonn_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    src = open(os.path.join(REPO, "egonn_amd", "csrc", "tuples.hip")).read()
    assert "#pragma clang fp contract(off)" in src
    assert not re.search(r"atomicAdd|atomicMax|atomicMin|atomicExch|atomicCAS", src), "integer atomicOr on status words only"


def _refused(lib, rc, needle):
    assert rc == 1, rc                              # EGONN_STATUS_INVALID: returned before any device work
    assert needle in lib.egonn_last_error().decode(), lib.egonn_last_error()


def test_c_entries_refuse_bad_arguments_before_any_launch(lib):
    """every refusal below is decided on the host from the scalar arguments: the pointers are never dereferenced (they are
    small fake addresses), and no GPU is present when this runs"""
    p, q = C.c_void_p(64), C.c_void_p(128)
    r = lambda *v: (C.c_double * len(v))(*v)        # noqa: E731
    big = (1 << 24) + 1
    _refused(lib, lib.egonn_radius_count(p, big, p, 5, r(1.0), 1, 0, p, None), "2^24")
    _refused(lib, lib.egonn_radius_count(p, 5, p, big, r(1.0), 1, 0, p, None), "2^24")
    _refused(lib, lib.egonn_radius_count(p, 5, p, 5, r(-1.0), 1, 0, p, None), "radii")
    _refused(lib, lib.egonn_radius_count(p, 5, p, 5, r(float("nan")), 1, 0, p, None), "radii")
    _refused(lib, lib.egonn_radius_count(p, 5, p, 5, r(float("inf")), 1, 0, p, None), "radii")
    _refused(lib, lib.egonn_radius_count(p, 5, p, 5, r(1.0, 2.0, 3.0, 4.0, 5.0), 5, 0, p, None), "radii")
    _refused(lib, lib.egonn_radius_count(p, 5, p, 5, r(1.0), 0, 0, p, None), "radii")
    _refused(lib, lib.egonn_radius_count(p, 5, p, 5, r(1.0), 1, 2, p, None), "exclude_self_mask")
    _refused(lib, lib.egonn_radius_count(p, 5, q, 5, r(1.0), 1, 1, p, None), "same array")
    _refused(lib, lib.egonn_radius_count(p, 5, p, 6, r(1.0), 1, 1, p, None), "same array")
    _refused(lib, lib.egonn_radius_count(None, 5, p, 5, r(1.0), 1, 0, p, None), "null")
    _refused(lib, lib.egonn_radius_fill(p, 5, q, 5, 1.0, 1, p, p, 10, p, None), "same array")
    _refused(lib, lib.egonn_radius_fill(p, 5, p, 5, -0.5, 0, p, p, 10, p, None), "radius")
    _refused(lib, lib.egonn_radius_fill(p, 5, p, 5, 1.0, 0, p, p, -1, p, None), "capacity")
    _refused(lib, lib.egonn_radius_fill(p, 5, p, 5, 1.0, 0, p, p, 10, None, None), "null")
    _refused(lib, lib.egonn_pair_masks(p, 0, p, p, 1, p, p, 1, 4, p, p, p, None), "batch size")
    _refused(lib, lib.egonn_pair_masks(p, 4097, p, p, 1, p, p, 1, 4, p, p, p, None), "batch size")
    _refused(lib, lib.egonn_pair_masks(p, 4, p, None, 1, p, p, 1, 4, p, p, p, None), "null")
    _refused(lib, lib.egonn_relative_poses(p, -1, p, p, 4, 1, p, p, None), "bad shape")
    _refused(lib, lib.egonn_relative_poses(p, 4, None, p, 4, 1, p, p, None), "null")
    _refused(lib, lib.egonn_gather_clouds(p, 10, p, 2, p, 0, p, 10, p, p, None), "n_pick")
    _refused(lib, lib.egonn_gather_clouds(p, 10, p, 2, p, 4097, p, 10, p, p, None), "n_pick")
    _refused(lib, lib.egonn_gather_clouds(p, 10, p, 2, p, 2, p, -1, p, p, None), "capacity")
    _refused(lib, lib.egonn_gather_clouds(p, 10, p, 2, p, 2, p, 10, p, None, None), "null")


def test_python_refuses_bad_arguments_before_asking_for_a_device(lib):
    """each ValueError below is raised although no HIP device is visible: the shape and value checks come first (a call that
    passes them fails later with the RuntimeError of _lib.require_gpu)"""
    import torch
    from egonn_amd import tuples as T
    xy = np.zeros((5, 2))
    with pytest.raises(ValueError, match=r"\(n, 2\)"):
        T.radius_neighbors(np.zeros((5, 3)), None, 1.0)
    with pytest.raises(ValueError, match=r"\(n, 2\)"):
        T.radius_neighbors(xy, np.zeros(5), 1.0)
    for bad in (-1.0, float("nan"), float("inf"), [1.0] * 5, []):
        with pytest.raises(ValueError, match="radi"):
            T.radius_neighbors(xy, None, bad)
    with pytest.raises(ValueError, match="exclude_self"):
        T.radius_neighbors(xy, xy.copy(), 1.0, exclude_self=True)
    with pytest.raises(ValueError, match="exclude_self"):
        T.radius_neighbors(xy, None, [1.0, 2.0], exclude_self=[True])
    with pytest.raises(ValueError, match=r"\(n, 2\)"):
        T.count_within(xy, np.zeros((4, 3)), 1.0)
    with pytest.raises(ValueError, match=r"\(n, 4, 4\)"):
        T.relative_poses(np.zeros((3, 3, 4)), [0], [1])
    with pytest.raises(ValueError, match="equally long"):
        T.relative_poses(np.zeros((3, 4, 4)), [0, 1], [1])
    with pytest.raises(ValueError, match="voxel_size"):
        T.CloudBank(voxel_size=0.0)
    with pytest.raises(ValueError, match="crop"):
        T.CloudBank(crop=(0, 1, 2))
    with pytest.raises(ValueError, match=r"\(n, 3 \| 4\)"):
        T.CloudBank().add([np.zeros((4, 5), np.float32)])
    with pytest.raises(ValueError, match="picks"):
        T.CloudBank().gather([])
    with pytest.raises(ValueError, match=r"\(n, 4, 4\)"):
        T.generate_training_tuples(np.zeros((3, 4)), lambda i: None)
    with pytest.raises(ValueError, match="pairs_per_call"):
        T.generate_training_tuples(np.tile(np.eye(4), (3, 1, 1)), lambda i: None, pairs_per_call=0)
    with pytest.raises(ValueError, match="CloudBank or a callable"):
        T.generate_training_tuples(np.tile(np.eye(4), (3, 1, 1)), [1, 2, 3])
    with pytest.raises(ValueError, match="one entry per pose"):
        T.generate_training_tuples(np.tile(np.eye(4), (3, 1, 1)), lambda i: None, timestamps=[1])
    tuples = _toy_tuples()
    with pytest.raises(ValueError, match="consecutive"):
        T.TupleIndex({1: tuples[1], 5: tuples[5]})
    unsorted = {0: T.TrainingTuple(0, 0, "", np.array([1, 0]), np.array([0]), np.eye(4))}
    with pytest.raises(ValueError, match="sorted"):
        T.TupleIndex(unsorted)
    with pytest.raises(ValueError, match="batch size"):
        T.TupleIndex(tuples).masks(np.zeros(0, np.int32))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device"):
            T.radius_neighbors(xy, None, 1.0)


# ----------------------------------------------------------------------------- pickles
def _toy_tuples(n=24, pos_r=1.5, non_r=4.0):
    """positions on a line 1 m apart, elements 7 and 23 moved away (no positives); tables by the restated rule"""
    from egonn_amd.tuples import TrainingTuple
    xy = np.stack([np.arange(n, dtype=np.float64), np.zeros(n)], axis=1)
    for k, y in ((7, 100.0), (23, -100.0)):
        if k < n:
            xy[k, 1] = y
    po, pi = D.radius_rows(xy, xy, pos_r, exclude_self=True)
    no, ni = D.radius_rows(xy, xy, non_r)
    out = {}
    for i in range(n):
        pose = np.eye(4)
        pose[:2, 3] = xy[i]
        p = pi[po[i]: po[i + 1]]
        out[i] = TrainingTuple(i, 1000 + i, f"scan/{i}.bin", p, ni[no[i]: no[i + 1]], pose,
                               {int(j): np.eye(4) * (1 + 0.01 * j) for j in p})
    return out


def _same_tuple(a, b):
    assert (a.id, a.timestamp, a.rel_scan_filepath) == (b.id, b.timestamp, b.rel_scan_filepath)
    assert np.array_equal(a.positives, b.positives) and np.array_equal(a.non_negatives, b.non_negatives)
    assert np.array_equal(a.pose, b.pose) and set(a.positives_poses) == set(b.positives_poses)
    for k in a.positives_poses:
        assert np.array_equal(a.positives_poses[k], b.positives_poses[k])


def test_training_tuple_pickles_round_trip(tmp_path):
    from egonn_amd import tuples as T
    tuples = _toy_tuples()
    path = str(tmp_path / "train.pickle")
    T.save_training_tuples(path, tuples)
    back = T.load_training_tuples(path)
    assert set(back) == set(tuples)
    for k in tuples:
        assert type(back[k]) is T.TrainingTuple
        _same_tuple(tuples[k], back[k])
    with open(str(tmp_path / "junk.pickle"), "wb") as f:
        pickle.dump([1, 2, 3], f)
    with pytest.raises(ValueError, match="training tuples"):
        T.load_training_tuples(str(tmp_path / "junk.pickle"))


def test_reads_a_pickle_that_names_the_reference_class(tmp_path):
    """a hand-made pickle whose GLOBAL is datasets.base_datasets.TrainingTuple, as the reference's generator writes it: our
    pickle with the module path rewritten in the opcode stream (no reference module exists in this process)"""
    from egonn_amd import tuples as T
    tuples = _toy_tuples(6)
    ours = pickle.dumps(tuples, protocol=2)                        # protocol 2: GLOBAL 'module name\n' in clear text
    assert b"cegonn_amd.tuples\nTrainingTuple\n" in ours
    theirs = ours.replace(b"cegonn_amd.tuples\nTrainingTuple\n", b"cdatasets.base_datasets\nTrainingTuple\n")
    names = [arg for op, arg, _ in pickletools.genops(theirs) if op.name == "GLOBAL"]
    assert "datasets.base_datasets TrainingTuple" in names and not any("egonn_amd" in n for n in names)
    path = str(tmp_path / "reference.pickle")
    with open(path, "wb") as f:
        f.write(theirs)
    with pytest.raises(Exception):
        pickle.loads(theirs)                                        # plain pickle needs the reference's module (or finds another `datasets`)
    back = T.load_training_tuples(path)
    for k in tuples:
        assert type(back[k]) is T.TrainingTuple
        _same_tuple(tuples[k], back[k])


def test_evaluation_set_uses_the_plain_tuple_layout(tmp_path):
    from egonn_amd import tuples as T
    q = [T.EvaluationTuple(10 + i, f"q/{i}.bin", np.array([1.0 * i, 2.0]), np.eye(4) * i) for i in range(3)]
    m = [T.EvaluationTuple(20 + i, f"m/{i}.bin", np.array([0.5 * i, -2.0])) for i in range(4)]
    path = str(tmp_path / "eval.pickle")
    T.EvaluationSet(q, m).save(path)
    with open(path, "rb") as f:
        raw = pickle.load(f)                                        # no class of ours inside: lists of plain tuples
    assert isinstance(raw, list) and len(raw) == 2 and all(type(e) is tuple and len(e) == 4 for part in raw for e in part)
    assert raw[0][1][0] == 11 and raw[0][1][1] == "q/1.bin" and raw[1][2][3] is None
    s = T.EvaluationSet()
    s.load(path)
    assert [e.timestamp for e in s.query_set] == [10, 11, 12] and [e.rel_scan_filepath for e in s.map_set] == [f"m/{i}.bin" for i in range(4)]
    assert np.array_equal(s.get_query_positions(), np.array([[0, 2.0], [1, 2], [2, 2]]))
    assert np.array_equal(s.get_map_positions()[:, 0], [0, 0.5, 1.0, 1.5]) and s.map_set[0].pose is None
    assert np.array_equal(s.query_set[2].pose, np.eye(4) * 2)
    with pytest.raises(AssertionError):
        T.EvaluationTuple(0, "", np.zeros(3))


# ----------------------------------------------------------------------------- sampler
def test_batch_sampler_invariants():
    from egonn_amd.tuples import BatchSampler
    tuples = _toy_tuples()
    s = BatchSampler(tuples, batch_size=8, seed=3)
    batches = list(s)
    assert batches and len(s) == len(batches)
    firsts = []
    for k, b in enumerate(batches):
        assert len(b) >= 4 and len(b) % 2 == 0
        assert len(b) == 8 or k == len(batches) - 1, "every batch but the last is full"
        for g in range(len(b) // 2):
            a, p = b[2 * g], b[2 * g + 1]
            assert p in tuples[a].positives and a in tuples[p].positives, (a, p)
            firsts.append(a)
    assert len(firsts) == len(set(firsts)), "an element is drawn as a first element at most once per epoch"
    assert 7 not in firsts and 23 not in firsts and not any(7 in b or 23 in b for b in batches), "no positives: skipped"
    assert list(BatchSampler(tuples, batch_size=8, seed=3)) == batches, "same seed, same batches"
    assert list(BatchSampler(tuples, batch_size=8, seed=4)) != batches
    assert list(s) != batches, "regenerated per __iter__: the second epoch draws anew"
    assert [len(b) for b in BatchSampler(tuples, batch_size=8, seed=3, max_batches=1)] == [8]
    assert BatchSampler(tuples, batch_size=2).batch_size == 4, "a batch needs two groups"
    # fewer than two groups left: nothing is flushed
    pair = {0: tuples[0], 1: tuples[1]}
    assert list(BatchSampler(pair, batch_size=4)) == []


def test_batch_sampler_expansion_arithmetic():
    from egonn_amd.tuples import BatchSampler
    tuples = _toy_tuples()
    s = BatchSampler(tuples, batch_size=6, batch_size_limit=20, batch_expansion_rate=1.4)
    sizes = []
    for _ in range(6):
        s.expand_batch()
        sizes.append(s.batch_size)
    assert sizes == [8, 11, 15, 20, 20, 20]                       # int(6 * 1.4) = 8, int(8 * 1.4) = 11, int(11 * 1.4) = 15, min(21, 20)
    none = BatchSampler(tuples, batch_size=6)
    none.expand_batch()
    assert none.batch_size == 6
    with pytest.raises(ValueError):
        BatchSampler(tuples, batch_size=6, batch_size_limit=20, batch_expansion_rate=1.0)
    with pytest.raises(ValueError):
        BatchSampler(tuples, batch_size=30, batch_size_limit=20, batch_expansion_rate=1.4)


# ----------------------------------------------------------------------------- the restatements reproduce the fixture
def _radius_cases():
    for rows in D.TRAJECTORY_ROWS:
        for r in D.TRAJECTORY_RADII:
            yield f"traj{rows}_xy", f"traj{rows}_r{int(r)}", r, False
    yield "lattice_xy", "lattice_r5", D.LATTICE_RADIUS, False
    yield "stationary_xy", "stationary_r1", D.STATIONARY_RADIUS, False
    yield "stationary_xy", "stationary_r1_noself", D.STATIONARY_RADIUS, True


def test_radius_rule_reproduces_every_reference_row(fx):
    for xy_key, key, r, excl in _radius_cases():
        off, idx = D.fixture_rows(fx, key)
        my_off, my_idx = D.radius_rows(fx[xy_key], fx[xy_key], r, excl)
        assert np.array_equal(off, my_off) and np.array_equal(idx, my_idx), key
        assert all((np.diff(row) > 0).all() for row in D.rows_of(off, idx)), key
    assert int(fx["lattice_boundary_pairs"]) == 1136
    assert (np.diff(fx["stationary_r1_noself_off"]) == 39).all()
    # the inputs are what the builders make (the fixture is reproducible from tests/tuples_data.py)
    assert np.array_equal(fx["traj257_xy"], D.trajectory(257, 1)) and np.array_equal(fx["lattice_xy"], D.lattice())


def test_filter_rule_reproduces_the_reference(fx):
    map32 = fx["filter_map_xy"].astype(np.float32).astype(np.float64)
    off, idx = D.fixture_rows(fx, "filter")
    my_off, my_idx = D.radius_rows(fx["filter_query_xy"], map32, D.FILTER_RADIUS)
    assert np.array_equal(off, my_off) and np.array_equal(idx, my_idx)
    kept = fx["filter_kept"]
    assert np.array_equal(np.diff(off) > 0, kept) and 0 < kept.sum() < len(kept)
    assert int(fx["filter_rows_changed_by_float32"]) > 0, "the case must tell a float32 map from a float64 one"


def test_mask_rule_reproduces_the_reference(fx):
    tables = [fx[k] for k in ("mask_pos_off", "mask_pos_idx", "mask_non_off", "mask_non_idx")]
    assert tables[0][11] == tables[0][10] and tables[0][80] == tables[0][79]
    for B in D.MASK_BATCHES:
        labels = fx[f"mask{B}_labels"]
        assert np.array_equal(labels, D.mask_labels(B)) and len(set(labels.tolist())) < B and 79 in labels
        pos, neg = D.pair_masks(labels, *tables)
        assert np.array_equal(pos, fx[f"mask{B}_pos"]) and np.array_equal(neg, fx[f"mask{B}_neg"]), B
    pos, neg = D.pair_masks(np.array([3, 80, -1, 4]), *tables)
    assert not pos[1].any() and not pos[:, 1].any() and not neg[2].any() and not neg[:, 2].any() and pos[0, 3]


def test_pose_rule_against_the_reference(fx):
    """d0 of the fixture is reproduced here; the UTM set shows why the difference comes first"""
    for kind in ("local", "utm"):
        poses, ia, ib = fx[f"poses_{kind}"], fx[f"poses_{kind}_ia"], fx[f"poses_{kind}_ib"]
        neg, st = D.relative_poses(poses, ia, ib, True)
        plain, _ = D.relative_poses(poses, ia, ib, False)
        assert not st.any()
        assert np.array_equal(neg[:, :3, :3], plain[:, :3, :3]) and np.array_equal(neg[:, :3, 3], -plain[:, :3, 3])
        assert np.abs(neg - fx[f"poses_{kind}_ref_neg"]).max() == float(fx[f"poses_{kind}_d0_neg"])
        assert np.abs(plain - fx[f"poses_{kind}_ref_plain"]).max() == float(fx[f"poses_{kind}_d0_plain"])
    assert 0 < float(fx["poses_local_d0_neg"]) < 1e-12
    truth, _ = D.relative_poses(fx["poses_utm"], fx["poses_utm_ia"], fx["poses_utm_ib"], True, dtype=np.longdouble)
    mine, _ = D.relative_poses(fx["poses_utm"], fx["poses_utm_ia"], fx["poses_utm_ib"], True)
    assert np.abs(mine - truth).max() <= np.abs(fx["poses_utm_ref_neg"] - truth).max()
    bad = np.tile(np.eye(4), (3, 1, 1))
    bad[1, 3, 3] = 1.0 + 1e-12
    bad[2, :3, :3] = [[1, 2, 3], [2, 4, 6], [0, 0, 1]]
    out, st = D.relative_poses(bad, [0, 0, 0, 5], [1, 2, 0, 0], True)
    assert st.tolist() == [1, 2, 0, 4] and all(np.array_equal(o, np.eye(4)) for o in out)


def test_gather_rule():
    bank = np.arange(30, dtype=np.float64).reshape(10, 3)
    off = np.array([0, 4, 4, 9, 10])
    pts, o = D.gather(bank, off, [2, 1, 0, 2])
    assert o.tolist() == [0, 5, 5, 9, 14] and np.array_equal(pts[:5], bank[4:9]) and np.array_equal(pts[5:9], bank[:4])
    assert D.gather(bank, off, [0, 4])[1].tolist() == [0, 0, 0] and D.gather(bank, off, [0, 2], capacity=8)[1].tolist() == [0, 0, 0]


def test_planted_sequence_is_what_the_end_to_end_test_assumes():
    raws, planted, gps = D.planted_sequence()
    assert len(raws) == 6 and all(r.shape == (6017, 4) and r.dtype == np.float32 for r in raws)
    assert all(len(D.zero_filtered(r)) == 6000 for r in raws)
    steps = np.linalg.norm(np.diff(planted[:, :3, 3], axis=0), axis=1)
    assert np.allclose(steps, 1.0, atol=0.02)
    assert np.linalg.norm(gps[:, :3, 3] - planted[:, :3, 3], axis=1).max() <= 0.3
    yaw = lambda m: np.arctan2(m[:, 1, 0], m[:, 0, 0])             # noqa: E731
    assert np.abs(yaw(gps) - yaw(planted)).max() <= 0.02 + 1e-12
    off, _ = D.radius_rows(gps[:, :2, 3], gps[:, :2, 3], 2.0, exclude_self=True)
    assert (np.diff(off) >= 1).all(), "every scan has a positive at pos_threshold = 2"

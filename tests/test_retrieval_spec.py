"""Retrieval matching on the CPU: known answers of the rule (tests/util_retrieval.py), the host half of the
product against it, and match_retrieval with the device steps replaced by their specifications."""
import ctypes
import logging
import os
import socket
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import util_retrieval as ur
from oracle import matcher_oracle as mo
from test_dist_cpu import _dump_db, _oracle_match_fn, _same_db, _stand_in_verify_fn

N_TRAJ, K_TRAJ = 24, 4


def _spec(block, counts, k):
    q, valid = ur.global_descriptors(ur.pool_sums(block, counts), counts)
    idx, score = ur.neighbours(q, valid, k)
    return q, valid, idx, score


def _images(rows, n_max=4):
    """One descriptor row per image, repeated: image i's mean descriptor is rows[i]; an all-None row is an empty image."""
    D = max(len(r) for r in rows if r is not None)
    block = np.zeros((len(rows), n_max, D), np.uint8)
    counts = np.zeros(len(rows), np.int32)
    for i, r in enumerate(rows):
        if r is not None:
            block[i, :] = np.asarray(r, np.uint8)
            counts[i] = n_max
    return block, counts


# ---- known answers of the rule ---------------------------------------------------------------------------------------------
A, B, C = [200, 10, 10, 10, 50, 0, 0, 90], [10, 200, 10, 10, 0, 50, 90, 0], [10, 10, 200, 120, 0, 0, 50, 50]


def test_duplicate_images_tie_and_the_lower_index_wins():
    block, counts = _images([A, B, A, C, A])
    q, valid, idx, score = _spec(block, counts, 2)
    assert valid.tolist() == [1] * 5 and np.array_equal(q[0], q[2]) and np.array_equal(q[0], q[4])
    assert idx[1, 0] == 0 or score[1, 0] > score[1, 1]            # image 1 sees 0, 2, 4 alike: the lowest comes first
    s1 = (q[1].astype(np.int64) * q[[0, 2, 4]]).sum(axis=1)
    assert s1[0] == s1[1] == s1[2]
    order1 = ur.neighbours(q, valid, 4)[0][1].tolist()
    assert [j for j in order1 if j in (0, 2, 4)] == [0, 2, 4]
    assert idx[0].tolist() == [2, 4] and idx[2].tolist() == [0, 4] and idx[4].tolist() == [0, 2]
    assert score[0, 0] == score[0, 1] == int((q[0].astype(np.int64) ** 2).sum())


def test_an_empty_image_neither_gets_nor_becomes_a_neighbour():
    block, counts = _images([A, None, B, C])
    q, valid, idx, score = _spec(block, counts, 3)
    assert valid.tolist() == [1, 0, 1, 1] and not q[1].any()
    assert (idx[1] == -1).all() and (score[1] == ur.INT32_MIN).all()
    assert 1 not in idx
    for i in (0, 2, 3):                                               # two candidates for k = 3: a -1 tail
        assert sorted(idx[i, :2].tolist()) == sorted({0, 2, 3} - {i}) and idx[i, 2] == -1 and score[i, 2] == ur.INT32_MIN
    assert ur.pairs_of(idx).tolist() == [[0, 2], [0, 3], [2, 3]]


def test_identical_images_give_zero_descriptors_and_the_lowest_indices():
    block, counts = _images([A] * 6)                                  # the Dummy extractor's case
    q, valid, idx, score = _spec(block, counts, 3)
    assert not q.any() and valid.all()
    assert idx.tolist() == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 1, 2], [0, 1, 2]]
    assert (score == 0).all()


def test_all_neighbours_give_the_exhaustive_list():
    block, counts = ur.trajectory(seed=3, n=9, w=32, stride=8, D=16)
    for k in (8, 11):
        idx = _spec(block, counts, k)[2]
        assert np.array_equal(ur.pairs_of(idx), mo.exhaustive_pairs(9))
        assert (idx[:, :8] >= 0).all() and (idx[:, 8:] == -1).all()


def test_quantised_descriptors_keep_their_shape_and_padding():
    block, counts = ur.trajectory(seed=5, n=6, w=40, stride=10, D=100)
    q, valid = ur.global_descriptors(ur.pool_sums(block, counts), counts)
    assert q.shape == (6, 128) and q.dtype == np.int8 and not q[:, 100:].any()
    norms = np.sqrt((q.astype(np.float64) ** 2).sum(axis=1))
    assert np.allclose(norms, 127 * np.sqrt(100.0) / 4, rtol=0.01)   # rows of nearly equal norm: the dot product ranks like the cosine


# ---- the trajectory: full recall of the near pairs -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def traj():
    block, counts = ur.trajectory()
    q, valid, idx, score = _spec(block, counts, K_TRAJ)
    return block, counts, idx, ur.pairs_of(idx)


@pytest.mark.parametrize("D", [128, 384])
def test_every_pair_at_most_two_images_apart_is_selected(D, traj):
    if D == 128:
        pairs = traj[3]
    else:
        block, counts = ur.trajectory(D=D)
        pairs = ur.pairs_of(_spec(block, counts, K_TRAJ)[2])
    near = {(i, j) for i in range(N_TRAJ) for j in range(i + 1, N_TRAJ) if j - i <= 2}
    got = {tuple(p) for p in pairs.tolist()}
    assert len(near) == 45 and near <= got                             # recall 45 of 45 ...
    assert len(got) <= 60 < N_TRAJ * (N_TRAJ - 1) // 2                 # ... out of about 51 pairs, not 276


# ---- the host half of the product ------------------------------------------------------------------------------------------------
def test_product_host_steps_equal_the_rule(traj):
    from vit_colmap_amd.matching import global_descriptors, retrieval_pairs

    block, counts, idx, pairs = traj
    counts0 = counts.copy()
    counts0[[3, 17]] = 0
    for c in (counts, counts0):
        sums = ur.pool_sums(block, c)
        q0, v0 = ur.global_descriptors(sums, c)
        q1, v1 = global_descriptors(sums, c)
        assert q1.dtype == np.int8 and v1.dtype == np.int32 and np.array_equal(q0, q1) and np.array_equal(v0, v1)
    block100, counts100 = ur.trajectory(seed=5, n=6, w=40, stride=10, D=100)
    sums = ur.pool_sums(block100, counts100)
    assert np.array_equal(global_descriptors(sums, counts100)[0], ur.global_descriptors(sums, counts100)[0])
    q, v = global_descriptors(np.zeros((3, 8), np.int32), np.zeros(3, np.int32))     # no image has descriptors
    assert q.shape == (3, 32) and not q.any() and not v.any()
    got = retrieval_pairs(idx)
    assert got.dtype == np.int32 and np.array_equal(got, pairs)
    assert retrieval_pairs(np.full((5, 3), -1)).shape == (0, 2)
    assert retrieval_pairs(np.array([[1, 2], [0, -1], [0, 1]])).tolist() == [[0, 1], [0, 2], [1, 2]]
    ex = mo.exhaustive_pairs(N_TRAJ).tolist()                                          # a sub-sequence of the exhaustive list
    pos = [ex.index(p) for p in got.tolist()]
    assert pos == sorted(pos)


def test_product_global_descriptors_known_answers():
    """Worked by hand, so the product's host step does not rest on the specification's copy of the same lines."""
    from vit_colmap_amd.matching import global_descriptors

    def q_of(m_rows, counts, D):
        sums = np.zeros((len(m_rows), D), np.int32)
        for i, (row, c) in enumerate(zip(m_rows, counts)):
            sums[i, : len(row)] = np.asarray(row) * max(c, 1)           # sums = mean row x count
        return global_descriptors(sums, np.asarray(counts, np.int32))

    # D = 4, S = 127 * 2 / 4 = 63.5.  Means (4, 0, 0, 0) and 0: centre (2, 0, 0, 0), g = +-(1, 0, 0, 0), g S = +-63.5,
    # and half goes to even: +-64.  The columns are padded to 32.
    q, valid = q_of([[4], [0]], [3, 5], 4)
    assert q.shape == (2, 32) and q.dtype == np.int8 and valid.tolist() == [1, 1]
    assert q[0].tolist() == [64] + [0] * 31 and q[1].tolist() == [-64] + [0] * 31
    # D = 16, S = 127.  Means (6, 8, 0, ...) and 0: centre (3, 4), g = +-(0.6, 0.8), g S = +-(76.2, 101.6) -> +-(76, 102).
    # The empty image between them (its sums are never looked at) stays out of the centre and gets a zero row.
    sums = np.zeros((3, 16), np.int32)
    sums[0, :2], sums[1, :] = [12, 16], 999
    q, valid = global_descriptors(sums, np.array([2, 0, 7], np.int32))
    assert valid.tolist() == [1, 0, 1] and not q[1].any()
    assert q[0].tolist() == [76, 102] + [0] * 30 and q[2].tolist() == [-76, -102] + [0] * 30
    # D = 64, S = 254: a unit axis vector would be 254 and is clipped to 127.
    q, _ = q_of([[10], [0]], [1, 1], 64)
    assert q[0, 0] == 127 and q[1, 0] == -127 and not q[:, 1:].any()
    # one image alone is its own centre: g = 0, norm 0, q = 0
    q, valid = q_of([[9, 1]], [4], 4)
    assert valid.tolist() == [1] and not q.any()


def test_listed_pairs_are_dealt_round_robin():
    from vit_colmap_amd import dist as vd

    pairs = mo.exhaustive_pairs(7)[::2]
    parts = [vd.listed_pairs_for_rank(pairs, r, 3) for r in range(3)]
    assert all(p.dtype == np.int32 for p in parts) and max(map(len, parts)) - min(map(len, parts)) <= 1
    for r in range(3):
        assert np.array_equal(parts[r], pairs[r::3])
    assert vd.listed_pairs_for_rank(np.zeros((0, 2), np.int32), 1, 2).shape == (0, 2)


# ---- match_retrieval with the device steps replaced by their specifications ------------------------------------------------------
SEAMS = dict(neighbour_fn=ur.neighbour_fn, match_fn=_oracle_match_fn, verify_fn=_stand_in_verify_fn, device="cpu")


def _wide_options():
    """The trajectory's rows are signed normals with the negatives clipped by the quantiser, so a row and its noisy copy
    are about 1.05 rad apart: beyond the default max_distance of 0.7, under which no pair of them would match."""
    from vit_colmap_amd.utils.config import MatchingConfig

    return MatchingConfig(max_distance=1.25).to_matching_options()


def _pair_rows(path):
    from vit_colmap_amd.database import ColmapDatabase

    with ColmapDatabase.open_database(str(path)) as h:
        ids = [im.image_id for im in h.read_all_images()]
        m = {(i, j) for i in ids for j in ids if i < j and h.read_matches(i, j) is not None}
        g = {(i, j) for i in ids for j in ids if i < j and h.read_two_view_geometry(i, j) is not None}
    return m, g


@pytest.fixture(scope="module")
def traj_db(tmp_path_factory, traj):
    from vit_colmap_amd.matching import match_retrieval

    block, counts = traj[0][:, :96], np.minimum(traj[1], 96)          # 96 rows per image keep the numpy matcher quick
    path = tmp_path_factory.mktemp("retrieval") / "single.db"
    ur.make_feature_db(path, block, counts)
    stats = match_retrieval(database_path=str(path), matching_options=_wide_options(), num_neighbors=K_TRAJ, **SEAMS)
    return block, counts, path, stats


def test_rows_exist_for_exactly_the_selected_pairs(traj_db):
    block, counts, path, stats = traj_db
    pairs = ur.pairs_of(ur.neighbour_fn(block, counts, K_TRAJ))
    want = {(int(a) + 1, int(b) + 1) for a, b in pairs}                # image ids start at 1
    m, g = _pair_rows(path)
    assert m == want and g == want
    assert stats["pairs"] == len(pairs) < stats["candidate_pairs"] == 276
    assert stats["num_neighbors"] == K_TRAJ and stats["retrieval_s"] > 0 and stats["images"] == N_TRAJ and stats["ranks"] == 1
    assert stats["matches"] > 100 and stats["verified_pairs"] > 10


def test_with_every_image_a_neighbour_the_database_is_the_exhaustive_one(tmp_path):
    from vit_colmap_amd.matching import match_exhaustive, match_retrieval

    block, counts = ur.trajectory(seed=11, n=7, w=48, stride=12, D=64)
    counts[2] = 0                                                       # an image without features: exhaustive writes its empty rows
    for name in ("ex.db", "re.db", "re_few.db"):
        ur.make_feature_db(tmp_path / name, block, counts)
    seams = {k: v for k, v in SEAMS.items() if k != "neighbour_fn"}
    s0 = match_exhaustive(database_path=str(tmp_path / "ex.db"), matching_options=_wide_options(), **seams)
    # every VALID image is a neighbour of every other; the pairs of the empty image are the only ones left out
    s1 = match_retrieval(database_path=str(tmp_path / "re.db"), matching_options=_wide_options(), num_neighbors=6, **SEAMS)
    ex, re_ = _dump_db(tmp_path / "ex.db"), _dump_db(tmp_path / "re.db")
    assert s0["pairs"] == 21 and s1["pairs"] == 15 and s1["candidate_pairs"] == 21
    for key in ex:
        if isinstance(key, tuple) and key[0] in ("m", "tvg"):
            if 3 in key[1:]:                                            # image id 3 = index 2
                assert re_.get(key) is None and (key[0] == "tvg" or len(ex[key]) == 0)
            else:
                assert np.array_equal(ex[key], re_[key]), key
    assert s1["matches"] == s0["matches"] > 50 and s1["verified_pairs"] == s0["verified_pairs"] > 3


def test_with_every_image_valid_and_a_neighbour_the_tables_are_equal_row_for_row(tmp_path):
    from vit_colmap_amd.matching import match_exhaustive, match_retrieval

    block, counts = ur.trajectory(seed=12, n=6, w=48, stride=12, D=64)
    for name in ("ex.db", "re.db", "re64.db"):
        ur.make_feature_db(tmp_path / name, block, counts)
    seams = {k: v for k, v in SEAMS.items() if k != "neighbour_fn"}
    s0 = match_exhaustive(database_path=str(tmp_path / "ex.db"), matching_options=_wide_options(), **seams)
    s1 = match_retrieval(database_path=str(tmp_path / "re.db"), matching_options=_wide_options(), num_neighbors=5, **SEAMS)
    s2 = match_retrieval(database_path=str(tmp_path / "re64.db"), matching_options=_wide_options(), num_neighbors=64, **SEAMS)
    _same_db(_dump_db(tmp_path / "ex.db"), _dump_db(tmp_path / "re.db"))
    _same_db(_dump_db(tmp_path / "ex.db"), _dump_db(tmp_path / "re64.db"))
    for k in ("images", "pairs", "matches", "verified_pairs", "ranks", "guided_pairs", "pose_pairs"):
        assert s0[k] == s1[k] == s2[k], k
    assert set(s1) == set(s0) | {"num_neighbors", "candidate_pairs", "retrieval_s"} and s0["matches"] > 50


def test_guided_matching_passes_through(tmp_path):
    import test_guided_spec as tg
    from vit_colmap_amd.matching import match_exhaustive, match_retrieval

    tg.make_twin_db(tmp_path / "ex.db")
    tg.make_twin_db(tmp_path / "re.db")
    seams = dict(match_fn=tg._match_fn, verify_fn=tg._verify_fn, guided_fn=tg._guided_fn, device="cpu")
    s0 = match_exhaustive(database_path=str(tmp_path / "ex.db"), matching_options=tg._options(True), **seams)
    s1 = match_retrieval(database_path=str(tmp_path / "re.db"), matching_options=tg._options(True), num_neighbors=3,
                         neighbour_fn=ur.neighbour_fn, **seams)
    assert s1["guided_pairs"] == s0["guided_pairs"] == 3 and s1["pairs"] == 6
    ex, re_ = tg.dump_db(tmp_path / "ex.db"), tg.dump_db(tmp_path / "re.db")
    assert ex.keys() == re_.keys()
    for k in ex:
        assert np.array_equal(ex[k], re_[k]), k


def test_relative_pose_passes_through(tmp_path):
    import test_pose_spec as tp
    from vit_colmap_amd.matching import match_retrieval

    tp.make_pose_db(tmp_path / "re.db")
    calls = []
    # two neighbours per image: the three views of the first scene and each of the two twin pairs find each other
    s = match_retrieval(database_path=str(tmp_path / "re.db"), matching_options=tp._options(True), num_neighbors=2,
                        neighbour_fn=ur.neighbour_fn, match_fn=tp._match_fn, verify_fn=tp.pose_verify_fn(calls), device="cpu")
    rows = {k: g for k, g in tp.read_rows(tmp_path / "re.db").items() if g is not None}
    assert calls == [(True, True)] and len(rows) == s["pairs"] < 21
    for pair, config in tp.PAIRS.items():
        if pair in rows:
            assert rows[pair]["config"] == config and abs(np.linalg.norm(rows[pair]["qvec"]) - 1) < 1e-12
    assert {(4, 5), (6, 7)} <= set(rows) and set(tp.PAIRS) & set(rows)
    assert s["pose_pairs"] == s["verified_pairs"] >= 3 and s["planar_pairs"] >= 1 and s["panoramic_pairs"] >= 1


def test_small_and_empty_databases(tmp_path):
    from vit_colmap_amd.matching import match_retrieval

    block, counts = ur.trajectory(seed=2, n=3, w=16, stride=4, D=16)
    ur.make_feature_db(tmp_path / "one.db", block[:1], counts[:1])
    s = match_retrieval(database_path=str(tmp_path / "one.db"), **SEAMS)
    assert s["pairs"] == 0 and s["candidate_pairs"] == 0 and s["num_neighbors"] == 20 and s["retrieval_s"] == 0.0
    ur.make_feature_db(tmp_path / "none.db", block, np.zeros(3, np.int32))         # three images, no descriptors at all
    s = match_retrieval(database_path=str(tmp_path / "none.db"), **SEAMS)
    assert s["pairs"] == 0 and s["candidate_pairs"] == 3 and _pair_rows(tmp_path / "none.db") == (set(), set())
    ur.make_feature_db(tmp_path / "two.db", block[:2], counts[:2])                  # k is cut to n - 1
    s = match_retrieval(database_path=str(tmp_path / "two.db"), num_neighbors=20, **SEAMS)
    assert s["pairs"] == 1 and _pair_rows(tmp_path / "two.db")[0] == {(1, 2)}


# ---- configuration, command line, dispatch, errors -------------------------------------------------------------------------------
def test_config_defaults_and_command_line(monkeypatch, tmp_path):
    from vit_colmap_amd import _lib
    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import MatchingConfig

    assert MatchingConfig().matcher_type == "exhaustive" and MatchingConfig().num_neighbors == 20
    assert _lib.VC_MAX_NEIGHBOURS == 64
    seen = []
    monkeypatch.setattr(rp.Pipeline, "run", lambda self, *a, **k: seen.append((self.config.matching.matcher_type,
                                                                               self.config.matching.num_neighbors)))
    base = ["prog", "--images", str(tmp_path), "--output", str(tmp_path), "--db", str(tmp_path / "x.db")]
    for extra in ([], ["--matcher", "retrieval"], ["--matcher", "retrieval", "--num-neighbors", "7"], ["--matcher", "exhaustive"]):
        monkeypatch.setattr(sys, "argv", base + extra)
        rp.main()
    assert seen == [("exhaustive", 20), ("retrieval", 20), ("retrieval", 7), ("exhaustive", 20)]
    monkeypatch.setattr(sys, "argv", base + ["--matcher", "vocab_tree"])
    with pytest.raises(SystemExit):
        rp.main()


def _pipeline(tmp_path, **matching):
    from vit_colmap_amd.pipeline.run_pipeline import Pipeline
    from vit_colmap_amd.utils import image_io
    from vit_colmap_amd.utils.config import Config
    from test_host_logic import checkerboard

    (tmp_path / "images").mkdir(exist_ok=True)
    for k in range(3):
        image_io.imwrite(tmp_path / "images" / f"img_{k}.png", np.roll(checkerboard(), (13 * k, 7 * k), (1, 0)))
    cfg = Config()
    cfg.extractor.extractor_type = "dummy"
    cfg.do_reconstruction = False
    for k, v in matching.items():
        setattr(cfg.matching, k, v)
    return Pipeline(cfg)


def test_pipeline_dispatches_on_the_matcher_type(tmp_path, monkeypatch):
    import vit_colmap_amd.matching as vm

    calls = []
    monkeypatch.setattr(vm, "match_exhaustive", lambda **kw: calls.append(("exhaustive", kw)) or {})
    monkeypatch.setattr(vm, "match_retrieval", lambda **kw: calls.append(("retrieval", kw)) or {})
    args = (tmp_path / "images", tmp_path / "out", tmp_path / "a.db")
    _pipeline(tmp_path).run(*args)
    assert [c[0] for c in calls] == ["exhaustive"] and "num_neighbors" not in calls[0][1]
    _pipeline(tmp_path, matcher_type="retrieval", num_neighbors=9).run(tmp_path / "images", tmp_path / "out", tmp_path / "b.db")
    assert [c[0] for c in calls] == ["exhaustive", "retrieval"] and calls[1][1]["num_neighbors"] == 9
    assert calls[1][1]["database_path"] == str(tmp_path / "b.db") and calls[1][1]["matching_options"] is not None
    with pytest.raises(ValueError, match="vocab_tree"):
        _pipeline(tmp_path, matcher_type="vocab_tree").run(tmp_path / "images", tmp_path / "out", tmp_path / "c.db")
    with pytest.raises(ValueError, match="num_neighbors"):
        _pipeline(tmp_path, matcher_type="retrieval", num_neighbors=0).run(tmp_path / "images", tmp_path / "out", tmp_path / "d.db")
    assert len(calls) == 2 and not (tmp_path / "c.db").exists() and not (tmp_path / "d.db").exists()


def test_num_neighbors_is_checked_and_clamped(tmp_path, caplog):
    from vit_colmap_amd.matching import match_retrieval

    block, counts = ur.trajectory(seed=2, n=4, w=16, stride=4, D=16)
    ur.make_feature_db(tmp_path / "a.db", block, counts)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="num_neighbors"):
            match_retrieval(database_path=str(tmp_path / "a.db"), num_neighbors=bad, **SEAMS)
    asked = []
    seams = dict(SEAMS, neighbour_fn=lambda b, c, k: asked.append(k) or ur.neighbour_fn(b, c, k))
    with caplog.at_level(logging.WARNING, logger="vit_colmap_amd.matching.retrieval"):
        s = match_retrieval(database_path=str(tmp_path / "a.db"), num_neighbors=500, **seams)
    assert s["num_neighbors"] == 64 and s["pairs"] == 6 and asked == [3]
    assert len([r for r in caplog.records if "clamped" in r.getMessage()]) == 1


def test_the_sharded_in_memory_pipeline_refuses_retrieval(tmp_path):
    from vit_colmap_amd.pipeline.distributed import run_sharded

    with pytest.raises(ValueError, match="match_retrieval"):
        run_sharded(tmp_path, tmp_path / "x.db", "PINHOLE", matcher_type="retrieval")
    assert not (tmp_path / "x.db").exists()


def test_without_a_gpu_the_device_steps_raise(monkeypatch, tmp_path):
    import torch

    from vit_colmap_amd import _lib
    from vit_colmap_amd.matching import match_retrieval, nearest_images, pool_descriptors

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.HipLibraryError):
        pool_descriptors(np.zeros((1, 1, 1), np.uint8), np.ones(1, np.int32))
    with pytest.raises(_lib.HipLibraryError):
        nearest_images(np.zeros((2, 32), np.int8), np.ones(2, np.int32), 1)
    with pytest.raises(_lib.HipLibraryError, match="match_retrieval"):
        match_retrieval(database_path=str(tmp_path / "x.db"), match_fn=_oracle_match_fn)


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------
def test_entry_points_validate_their_arguments_without_a_gpu():
    from vit_colmap_amd import _lib

    lib = _lib.load()
    fake = ctypes.c_void_p(4096)                                       # never dereferenced: every call below is refused first
    assert lib.vc_pool_descriptors_u8(None, None, 2, 16, 32, None, None) == _lib.VC_ERR_INVALID_ARG
    assert lib.vc_pool_descriptors_u8(fake, fake, 2, 0, 32, fake, None) == _lib.VC_ERR_INVALID_ARG
    assert lib.vc_pool_descriptors_u8(fake, fake, 2, _lib.VC_MAX_KEYPOINTS + 1, 32, fake, None) == _lib.VC_ERR_UNSUPPORTED
    assert lib.vc_pool_descriptors_u8(fake, fake, 2, 16, _lib.VC_MAX_DESC_DIM + 1, fake, None) == _lib.VC_ERR_UNSUPPORTED
    assert lib.vc_pool_descriptors_u8(None, None, 0, 16, 32, None, None) == _lib.VC_OK
    # workspace: one 8-byte key per (column range, row, neighbour); 16 column ranges at most, one from 512 row groups on
    assert lib.vc_retrieval_workspace_bytes(500, 256, 20) == 16 * 500 * 20 * 8
    assert lib.vc_retrieval_workspace_bytes(16384, 256, 20) == 4 * 16384 * 20 * 8
    assert lib.vc_retrieval_workspace_bytes(65536, 256, 64) == 65536 * 64 * 8
    assert lib.vc_retrieval_workspace_bytes(1, 32, 1) == 8
    for n, d, k in [(0, 32, 1), (10, 100, 4), (10, 2048, 4), (10, 32, 0), (10, 32, 65), ((1 << 20) + 1, 32, 4)]:
        assert lib.vc_retrieval_workspace_bytes(n, d, k) == 0
    ws = lib.vc_retrieval_workspace_bytes(100, 64, 8)
    assert lib.vc_retrieval_topk_i8(None, None, 100, 64, 8, None, None, None, ws, None) == _lib.VC_ERR_INVALID_ARG
    for missing in range(5):
        p = [fake] * 5
        p[missing] = None
        assert lib.vc_retrieval_topk_i8(p[0], p[1], 100, 64, 8, p[2], p[3], p[4], ws, None) == _lib.VC_ERR_INVALID_ARG
    assert lib.vc_retrieval_topk_i8(fake, fake, 100, 64, 8, fake, fake, fake, ws - 1, None) == _lib.VC_ERR_WORKSPACE
    assert lib.vc_retrieval_topk_i8(fake, fake, 100, 64, 0, fake, fake, fake, ws, None) == _lib.VC_ERR_INVALID_ARG
    assert lib.vc_retrieval_topk_i8(fake, fake, 100, 100, 8, fake, fake, fake, ws, None) == _lib.VC_ERR_INVALID_ARG   # not padded
    assert lib.vc_retrieval_topk_i8(ctypes.c_void_p(4100), fake, 100, 64, 8, fake, fake, fake, ws, None) == _lib.VC_ERR_INVALID_ARG
    assert lib.vc_retrieval_topk_i8(fake, fake, 100, 64, 65, fake, fake, fake, 1 << 30, None) == _lib.VC_ERR_UNSUPPORTED
    assert lib.vc_retrieval_topk_i8(fake, fake, 100, 2048, 8, fake, fake, fake, 1 << 30, None) == _lib.VC_ERR_UNSUPPORTED
    assert lib.vc_retrieval_topk_i8(fake, fake, (1 << 20) + 1, 64, 8, fake, fake, fake, 1 << 40, None) == _lib.VC_ERR_UNSUPPORTED
    assert lib.vc_retrieval_topk_i8(None, None, 0, 64, 8, None, None, None, 0, None) == _lib.VC_OK


# ---- two ranks ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, db_path, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from vit_colmap_amd.matching import match_retrieval

        calls = []
        seams = dict(SEAMS, neighbour_fn=lambda b, c, k: calls.append(rank) or ur.neighbour_fn(b, c, k))
        s = match_retrieval(database_path=db_path, matching_options=_wide_options(), num_neighbors=K_TRAJ, distributed=True,
                            **seams)
        ok = s["ranks"] == 2 and s["num_neighbors"] == K_TRAJ and s["candidate_pairs"] == 276 and 45 <= s["pairs"] < 276
        ok = ok and calls == ([0] if rank == 0 else [])                # rank 0 alone chooses the pairs
        try:                                                            # rank 0's failure in the selection reaches rank 1
            match_retrieval(database_path=db_path, num_neighbors=K_TRAJ, distributed=True,
                            **dict(SEAMS, neighbour_fn=lambda b, c, k: 1 / 0))
            ok = False
        except ZeroDivisionError:
            ok = ok and rank == 0
        except RuntimeError as e:
            ok = ok and rank == 1 and "rank 0 failed" in str(e)
        q.put((bool(ok), s["pairs"], s["matches"]))
    finally:
        dist.destroy_process_group()


def test_two_ranks_write_the_single_process_database(tmp_path, traj_db):
    block, counts, single_path, single_stats = traj_db
    ur.make_feature_db(tmp_path / "dist.db", block, counts)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path / "dist.db"), q)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(r[0] for r in results)
    assert all(r[1:] == (single_stats["pairs"], single_stats["matches"]) for r in results)
    _same_db(_dump_db(single_path), _dump_db(tmp_path / "dist.db"))

"""Retrieval matching on the GPU: vc_pool_descriptors_u8 and vc_retrieval_topk_i8 bit for bit against the
numpy rule (tests/util_retrieval.py), and match_retrieval end to end."""
import numpy as np
import pytest
import torch

import util_retrieval as ur
from util_data import quantize

pytestmark = pytest.mark.gpu


# ---- pooling ---------------------------------------------------------------------------------------------------------------------
def _counts(n, n_max, rs):
    """0, 1, n_max and a partial fill, as far as n goes; random fills behind them."""
    base = [n_max, 0, 1, max(n_max * 2 // 3, 1)]
    return np.array((base + list(rs.randint(0, n_max + 1, max(n - 4, 0))))[:n], np.int32)


# the issue's shapes; (4, 40, 301): a row longer than the workgroup and no multiple of 4; (70, 64, 48): three 16-byte chunks per row, so some threads of a workgroup idle
@pytest.mark.parametrize("n,n_max,D", [(1, 1, 1), (3, 17, 100), (5, 300, 128), (2, 2048, 1024), (4, 40, 301), (70, 64, 48)])
def test_pooling_is_exact(n, n_max, D):
    from vit_colmap_amd.matching import pool_descriptors

    rs = np.random.RandomState(n * 1000 + D)
    block = rs.randint(0, 256, (n, n_max, D)).astype(np.uint8)           # rows past the count hold data too: they must not be read
    for counts in (_counts(n, n_max, rs), np.full(n, n_max, np.int32), np.zeros(n, np.int32)):
        got = pool_descriptors(block, counts)
        assert got.dtype == np.int32 and got.shape == (n, D)
        assert np.array_equal(got, ur.pool_sums(block, counts)), counts


def test_pooling_reaches_the_largest_sum():
    from vit_colmap_amd.matching import pool_descriptors

    block = np.full((2, 2048, 1024), 255, np.uint8)
    got = pool_descriptors(block, np.array([2048, 1999], np.int32))
    assert (got[0] == 255 * 2048).all() and (got[1] == 255 * 1999).all()


# blocks taller than one kernel block (VC_MAX_KEYPOINTS = 2048 rows; SIFT's default asks for 8192, the trainable model for
# 20 480): pooled in row sub-blocks.  One row over, two full sub-blocks, and two sub-blocks and a part.
@pytest.mark.parametrize("n,n_max,D", [(3, 2049, 16), (4, 4096, 8), (5, 5000, 36)])
def test_pooling_of_tall_blocks_is_exact(n, n_max, D):
    from vit_colmap_amd.matching import pool_descriptors

    rs = np.random.RandomState(n_max)
    block = rs.randint(0, 256, (n, n_max, D)).astype(np.uint8)
    edges = np.array([n_max, 2048, 2049, 0, 2047], np.int32)[:n]      # counts at, and either side of, the sub-block edge
    for counts in (edges, _counts(n, n_max, rs), np.full(n, n_max, np.int32)):
        assert np.array_equal(pool_descriptors(block, counts), ur.pool_sums(block, counts)), counts
    assert np.array_equal(pool_descriptors(torch.from_numpy(block).cuda(), torch.from_numpy(edges).cuda()),
                          ur.pool_sums(block, edges))                  # a block that is on the device already


def _tall_trajectory(n=8, k=2):
    """Every image: 2048 rows that all images share, then its rows of a short trajectory.  What tells the images apart
    lies past row 2048 alone."""
    traj, traj_counts = ur.trajectory(seed=7, n=n, w=256, stride=64, D=128)
    common = quantize(np.random.RandomState(1).standard_normal((2048, 128)))
    block = np.concatenate([np.broadcast_to(common, (n, 2048, 128)), traj], axis=1)
    counts = (2048 + traj_counts).astype(np.int32)
    neigh = ur.neighbour_fn(block, counts, k)
    assert not np.array_equal(neigh, ur.neighbour_fn(block[:, :2048], np.minimum(counts, 2048), k))   # the tail decides
    return np.ascontiguousarray(block), counts, neigh


def test_neighbours_of_tall_blocks_equal_the_rule(tmp_path):
    from test_retrieval_spec import _pair_rows, _wide_options
    from vit_colmap_amd.matching import match_retrieval
    from vit_colmap_amd.matching.retrieval import hip_neighbours

    block, counts, neigh = _tall_trajectory()
    assert block.shape[1] == 2304
    assert np.array_equal(hip_neighbours(block, counts, 2), neigh)
    pairs = ur.pairs_of(neigh)
    ur.make_feature_db(tmp_path / "tall.db", block, counts)
    s = match_retrieval(database_path=str(tmp_path / "tall.db"), matching_options=_wide_options(), num_neighbors=2)
    assert s["pairs"] == len(pairs) < s["candidate_pairs"] == 28 and s["matches"] > 0
    want = {(int(a) + 1, int(b) + 1) for a, b in pairs}
    assert _pair_rows(tmp_path / "tall.db") == (want, want)


# ---- nearest images ----------------------------------------------------------------------------------------------------------------
def _random_q(seed, n, D, invalid_every=0):
    rs = np.random.RandomState(seed)
    q = np.zeros((n, (D + 31) // 32 * 32), np.int8)
    q[:, :D] = rs.randint(-127, 128, (n, D))
    valid = np.ones(n, np.int32)
    if invalid_every:
        valid[rs.permutation(n)[: n // invalid_every]] = 0
    return q, valid


def _check(q, valid, k):
    from vit_colmap_amd.matching import nearest_images

    idx, score = nearest_images(q, valid, k, return_scores=True)
    ref_idx, ref_score = ur.neighbours(q, valid, k)
    assert idx.dtype == np.int32 and score.dtype == np.int32 and idx.shape == (len(q), k)
    assert np.array_equal(idx, ref_idx)
    assert np.array_equal(score, ref_score)
    return idx, score


@pytest.mark.parametrize("n,D,k", [(1, 32, 1), (2, 32, 1), (2, 100, 4), (33, 32, 4), (33, 256, 64), (33, 1024, 1), (257, 100, 4),
                                   (257, 1024, 64), (257, 32, 1), (1000, 256, 4), (1000, 32, 64), (1000, 1024, 1), (1000, 100, 64)])
def test_neighbours_of_random_rows_are_exact(n, D, k):
    q, valid = _random_q(n * 7 + D + k, n, D, invalid_every=0 if n < 33 else 9)
    idx, _ = _check(q, valid, k)
    if k >= n - 1 and n > 1:
        assert (idx[valid == 1, : int(valid.sum()) - 1] >= 0).all()      # every other valid image, then the -1 tail
        assert (idx[:, int(valid.sum()) - 1:] == -1).all()
    assert (idx[valid == 0] == -1).all()


def test_ties_across_column_tiles_go_to_the_lower_index():
    q, valid = _random_q(5, 257, 32)
    for i in range(0, 60):                                             # copies 64, 128 and 192 rows on: other tiles, other ranges
        q[i + 64] = q[i + 128] = q[i + 192] = q[i]
    valid[[70, 130]] = 0
    idx, score = _check(q, valid, 4)
    assert idx[3].tolist()[:3] == [67, 131, 195] and score[3, 0] == score[3, 1] == score[3, 2]
    _check(q, valid, 64)
    _check(q[:, :32].repeat(8, axis=1).copy(), valid, 4)               # the same ties at D = 256


def test_extreme_scores():
    rs = np.random.RandomState(11)
    q = (rs.randint(0, 2, (257, 1024)) * 254 - 127).astype(np.int8)    # every entry +-127
    q[100] = q[3]
    q[200] = -q[3]
    valid = np.ones(257, np.int32)
    idx, score = _check(q, valid, 64)
    assert idx[3, 0] == 100 and score[3, 0] == 127 * 127 * 1024
    idx, score = _check(q[[3, 200]].copy(), valid[:2], 1)
    assert score[0, 0] == -127 * 127 * 1024 and idx.tolist() == [[1], [0]]


def test_identical_and_all_invalid_images():
    q = np.zeros((40, 32), np.int8)
    idx, score = _check(q, np.ones(40, np.int32), 3)
    assert idx[0].tolist() == [1, 2, 3] and idx[39].tolist() == [0, 1, 2] and (score == 0).all()
    idx, score = _check(q, np.zeros(40, np.int32), 3)
    assert (idx == -1).all() and (score == ur.INT32_MIN).all()


def test_many_row_and_column_tiles():
    q, valid = _random_q(21, 4096, 128, invalid_every=50)
    _check(q, valid, 8)


def test_refusals_on_the_device():
    from vit_colmap_amd import _lib

    lib = _lib.load()
    n, d, k = 100, 64, 8
    q = torch.zeros((n, d), dtype=torch.int8, device="cuda")
    valid = torch.ones(n, dtype=torch.int32, device="cuda")
    idx = torch.full((n, k), 7, dtype=torch.int32, device="cuda")
    score = torch.full((n, k), 7, dtype=torch.int32, device="cuda")
    need = lib.vc_retrieval_workspace_bytes(n, d, k)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    p = _lib.ptr
    args = lambda **kw: [kw.get("q", p(q)), kw.get("valid", p(valid)), n, d, k, kw.get("idx", p(idx)), kw.get("score", p(score)),  # noqa: E731
                         kw.get("ws", p(ws)), kw.get("bytes", need), _lib.stream_ptr()]
    assert lib.vc_retrieval_topk_i8(*args(bytes=need - 1)) == _lib.VC_ERR_WORKSPACE
    for name in ("q", "valid", "idx", "score", "ws"):
        assert lib.vc_retrieval_topk_i8(*args(**{name: None})) == _lib.VC_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (idx == 7).all() and (score == 7).all()                    # a refusal launches nothing
    assert lib.vc_retrieval_topk_i8(*args()) == _lib.VC_OK
    torch.cuda.synchronize()
    assert idx[0].tolist() == list(range(1, 9)) and (score == 0).all()
    desc = torch.zeros((2, 4, 8), dtype=torch.uint8, device="cuda")
    assert lib.vc_pool_descriptors_u8(p(desc), None, 2, 4, 8, p(idx), _lib.stream_ptr()) == _lib.VC_ERR_INVALID_ARG


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_match_retrieval_on_the_device_equals_the_run_on_the_specifications(tmp_path):
    from test_dist_cpu import _dump_db, _oracle_match_fn, _same_db
    from test_retrieval_spec import K_TRAJ, _pair_rows, _wide_options
    from vit_colmap_amd.matching import match_retrieval
    from vit_colmap_amd.matching.retrieval import hip_neighbours

    block, counts = ur.trajectory()
    neigh = ur.neighbour_fn(block, counts, K_TRAJ)
    assert np.array_equal(hip_neighbours(block, counts, K_TRAJ), neigh)
    pairs = ur.pairs_of(neigh)
    near = {(i, j) for i in range(24) for j in range(i + 1, 24) if j - i <= 2}
    assert near <= {tuple(p) for p in pairs.tolist()}                   # (asserted on the CPU too: test_retrieval_spec.py)
    for name in ("device.db", "spec.db"):
        ur.make_feature_db(tmp_path / name, block, counts)
    s0 = match_retrieval(database_path=str(tmp_path / "device.db"), matching_options=_wide_options(), num_neighbors=K_TRAJ)
    s1 = match_retrieval(database_path=str(tmp_path / "spec.db"), matching_options=_wide_options(), num_neighbors=K_TRAJ,
                         neighbour_fn=ur.neighbour_fn, match_fn=_oracle_match_fn)
    assert s0["pairs"] == s1["pairs"] == len(pairs) and s0["matches"] == s1["matches"] > 1000
    assert s0["verified_pairs"] == s1["verified_pairs"] and s0["retrieval_s"] > 0 and s0["candidate_pairs"] == 276
    want = {(int(a) + 1, int(b) + 1) for a, b in pairs}
    assert _pair_rows(tmp_path / "device.db") == (want, want)
    _same_db(_dump_db(tmp_path / "device.db"), _dump_db(tmp_path / "spec.db"))   # matches byte for byte, two-view rows equal

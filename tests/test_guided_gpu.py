"""GPU parity of guided matching: vc_match_pairs_guided_u8 against the numpy specification of
tests/util_guided.py — bit-equal, no tolerance — then against the unguided matcher where the model admits every
candidate, and end to end behind verify_pairs and match_exhaustive."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from oracle import matcher_oracle as mo
from oracle import two_view_oracle as tv
from util_guided import admissible, guided_match_pair, plain_inliers, twin_scene

pytestmark = pytest.mark.gpu

SENTINEL = -77777   # out_counts is pre-filled with it: a count the kernel never wrote cannot pass for a result
KIND_CODE = {"F": 0, "H": 1, None: -1}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_guided(desc, counts, kps, pairs, models, kinds, max_error=4.0, **kw):
    """desc uint8 (n, n_max, D), counts, kps float32 (n, n_max, 2), pairs (P, 2), models (P, 9), kinds list -> P lists."""
    from vit_colmap_amd.matching import match_pairs_guided, prepare_descriptors

    n_images, n_max, d = desc.shape
    prepared = prepare_descriptors(dev(desc), dev(counts))
    out_counts = torch.full((len(pairs),), SENTINEL, dtype=torch.int32, device="cuda")
    kind = np.array([KIND_CODE[k] for k in kinds], np.int32)
    m, c = match_pairs_guided(prepared, dev(counts), n_images, n_max, d, dev(kps.astype(np.float32)), dev(np.asarray(pairs, np.int32)),
                              dev(np.asarray(models, np.float32).reshape(-1, 9)), dev(kind), max_error, out_counts=out_counts, **kw)
    torch.cuda.synchronize()
    m, c = m.cpu().numpy().view(np.uint32), c.cpu().numpy()
    assert not np.any(c == SENTINEL), f"counts never written for pairs {np.nonzero(c == SENTINEL)[0][:10]}"
    assert np.all((c >= 0) & (c <= n_max))
    return [m[p, : c[p]] for p in range(len(pairs))]


def spec_lists(desc, counts, kps, pairs, models, kinds, max_error=4.0, **kw):
    out = []
    for (a, b), m9, k in zip(pairs, models, kinds):
        if k is None:
            out.append(np.zeros((0, 2), np.uint32))
        else:
            out.append(guided_match_pair(desc[a, : counts[a]], desc[b, : counts[b]], kps[a, : counts[a]], kps[b, : counts[b]], k, m9,
                                         max_error, **kw))
    return out


def assert_guided_equal(desc, counts, kps, pairs, models, kinds, max_error=4.0, **kw):
    got = run_guided(desc, counts, kps, pairs, models, kinds, max_error, **kw)
    ref = spec_lists(desc, counts, kps, pairs, models, kinds, max_error, **kw)
    for p, (g, r) in enumerate(zip(got, ref)):
        assert np.array_equal(g, r), f"pair {p} {tuple(pairs[p])} kind {kinds[p]}: {len(g)} matches against {len(r)}"
    return got


def blocks(images, n_max=None):
    """[(kp (N, 2), desc (N, D))] -> padded desc block, counts, keypoint block (padding rows hold a keypoint that must not
    matter: the image centre)."""
    counts = np.array([len(d) for _, d in images], np.int32)
    n_max = n_max or max(int(counts.max()), 1)
    D = images[0][1].shape[1]
    desc = np.zeros((len(images), n_max, D), np.uint8)
    kps = np.full((len(images), n_max, 2), 320.0, np.float32)
    for k, (kp, d) in enumerate(images):
        desc[k, : len(d)] = d
        kps[k, : len(d)] = kp[:, :2]
    return desc, counts, kps


def scene_models(seed, n, n_unique, planar, D=128):
    kp1, kp2, d1, d2, is_twin = twin_scene(seed, n, n_unique, planar, D)
    _, f9, _ = plain_inliers(kp1, kp2, d1, d2, "F")
    _, h9, _ = plain_inliers(kp1, kp2, d1, d2, "H")
    assert f9 is not None and h9 is not None
    return kp1, kp2, d1, d2, is_twin, f9, h9


@pytest.mark.parametrize("D", [64, 128, 256, 384, 768, 1024])
def test_bit_equal_for_every_descriptor_length(D):
    kp1, kp2, d1, d2, is_twin, f9, h9 = scene_models(41, 300, 140, True, D)
    desc, counts, kps = blocks([(kp1, d1), (kp2, d2)])
    pairs = np.array([[0, 1]] * 4, np.int32)
    got = assert_guided_equal(desc, counts, kps, pairs, [f9, h9, f9, h9], ["F", "H", "H", "F"])
    assert len(got[0]) > 250 and len(got[1]) > 250          # the look-alikes are back under either model
    assert sum(1 for i, j in got[1] if i == j and is_twin[i]) >= 0.9 * is_twin.sum()


@pytest.mark.parametrize("kind", ["F", "H"])
def test_ragged_and_empty_blocks(kind):
    kp1, kp2, d1, d2, _, f9, h9 = scene_models(42 if kind == "F" else 44, 512, 200 if kind == "F" else 100, kind == "H")
    images = [(kp1[:0], d1[:0]), (kp1[:1], d1[:1]), (kp1[:300], d1[:300]), (kp2, d2)]
    desc, counts, kps = blocks(images)
    assert counts.tolist() == [0, 1, 300, 512]
    pairs = mo.exhaustive_pairs(4)
    m9 = f9 if kind == "F" else h9
    got = assert_guided_equal(desc, counts, kps, pairs, [m9] * len(pairs), [kind] * len(pairs))
    assert [len(g) for g in got[:3]] == [0, 0, 0] and len(got[5]) > 250       # 300 rows against 512
    assert_guided_equal(desc, counts, kps, pairs, [m9] * len(pairs), [kind] * len(pairs), cross_check=False)


@pytest.mark.parametrize("kind,planar", [("F", False), ("H", True)])
def test_two_full_blocks_of_2048(kind, planar):
    kp1, kp2, d1, d2, is_twin, f9, h9 = scene_models(46, 2048, 900, planar)
    desc, counts, kps = blocks([(kp1, d1), (kp2, d2)])
    got = assert_guided_equal(desc, counts, kps, np.array([[0, 1]], np.int32), [f9 if kind == "F" else h9], [kind])
    assert len(got[0]) > 900


def test_skipped_pairs_nan_models_thresholds_and_error_bounds():
    kp1, kp2, d1, d2, _, f9, h9 = scene_models(40, 300, 140, False)
    desc, counts, kps = blocks([(kp1, d1), (kp2, d2)], n_max=320)
    nan9 = np.full(9, np.nan, np.float32)
    models = [f9, nan9, h9, nan9, f9, h9]
    kinds = ["F", "F", "H", "H", None, None]
    pairs = np.array([[0, 1]] * len(kinds), np.int32)
    got = assert_guided_equal(desc, counts, kps, pairs, models, kinds)
    assert len(got[0]) > 250 and len(got[1]) == 0 and all(len(g) == 0 for g in got[3:])
    for max_error in (0.0, 1.0, 4.0):
        for cross_check in (True, False):
            assert_guided_equal(desc, counts, kps, pairs, models, kinds, max_error, cross_check=cross_check)
    assert_guided_equal(desc, counts, kps, pairs, models, kinds, max_ratio=1.0, max_distance=1.5, cross_check=False)
    assert_guided_equal(desc, counts, kps, pairs, models, kinds, max_ratio=0.95, max_distance=1.2)
    assert_guided_equal(desc, counts, kps, pairs, models, kinds, max_ratio=0.6, max_distance=0.3)


def test_one_launch_of_many_pairs_of_mixed_kinds():
    images, models = [], {}
    for s, (seed, n, n_unique, planar) in enumerate([(40, 300, 140, False), (41, 300, 140, True), (43, 200, 60, False),
                                                      (44, 512, 100, True)]):
        kp1, kp2, d1, d2, _, f9, h9 = scene_models(seed, n, n_unique, planar)
        images += [(kp1, d1), (kp2, d2)]
        models[s] = (f9, h9)
    desc, counts, kps = blocks(images)
    pairs = mo.exhaustive_pairs(len(images))
    rs = np.random.RandomState(3)
    ms, kinds = [], []
    for p, (a, b) in enumerate(pairs):
        f9, h9 = models[a // 2]                              # the model of image a's scene, also where b shows another scene
        kind = ["F", "H", "F", None, "H"][p % 5]
        m9 = h9 if kind == "H" else f9
        if p % 11 == 7:
            m9 = np.full(9, np.nan, np.float32)
        if p % 13 == 5:
            m9 = rs.standard_normal(9).astype(np.float32)     # an arbitrary matrix
        ms.append(m9)
        kinds.append(kind)
    got = assert_guided_equal(desc, counts, kps, pairs, ms, kinds)
    assert sum(len(g) > 100 for g in got) >= 2


def test_agrees_with_the_unguided_matcher_where_every_candidate_is_admissible():
    from vit_colmap_amd.matching import match_pairs, prepare_descriptors

    kp1, kp2, d1, d2, _, f9, h9 = scene_models(40, 300, 140, False)
    desc, counts, kps = blocks([(kp1, d1), (kp2, d2), (kp1[:77], d2[:77])])
    pairs = mo.exhaustive_pairs(3)
    max_error = 1.0e6
    for kind, m9 in (("F", f9), ("H", h9)):
        for a, b in pairs:                                   # the premise, from the specification itself
            assert admissible(kps[a, : counts[a]], kps[b, : counts[b]], kind, m9, max_error).all()
        got = run_guided(desc, counts, kps, pairs, [m9] * 3, [kind] * 3, max_error)
        prepared = prepare_descriptors(dev(desc), dev(counts))
        m, c = match_pairs(prepared, dev(counts), 3, desc.shape[1], desc.shape[2], dev(pairs))
        torch.cuda.synchronize()
        m, c = m.cpu().numpy().view(np.uint32), c.cpu().numpy()
        for p in range(3):
            assert np.array_equal(got[p], m[p, : c[p]]), (kind, p)
            assert np.array_equal(got[p], mo.match_pair(desc[pairs[p][0], : counts[pairs[p][0]]], desc[pairs[p][1], : counts[pairs[p][1]]]))


def test_verify_pairs_then_guided_equals_the_spec_fed_the_gpus_model():
    from vit_colmap_amd.matching.exhaustive import hip_guided_blocks
    from vit_colmap_amd.matching.two_view import verify_pairs

    images, kp_by_index, pair_images, pids, lists, twins = [], {}, [], [], [], []
    for s, (seed, n, n_unique, planar) in enumerate([(40, 300, 140, False), (41, 300, 140, True), (43, 200, 60, False)]):
        kp1, kp2, d1, d2, is_twin = twin_scene(seed, n, n_unique, planar)
        images += [(kp1, d1), (kp2, d2)]
        kp_by_index[2 * s], kp_by_index[2 * s + 1] = kp1, kp2
        pair_images.append((2 * s, 2 * s + 1))
        pids.append((2 * s + 1) * 2147483647 + 2 * s + 2)
        lists.append(mo.match_pair(d1, d2))
        twins.append(is_twin)
    res = verify_pairs(kp_by_index, pair_images, pids, lists)
    assert all(r["config"] != tv.CONFIG_DEGENERATE and r["model"] in ("F", "H") and r["model9"].shape == (9,) for r in res)
    assert all(r["model9"].dtype == np.float32 for r in res)
    desc, counts, kps = blocks(images)
    pairs = np.array(pair_images, np.int32)
    got = hip_guided_blocks(desc, counts, kps, pairs, np.stack([r["model9"] for r in res]), [r["model"] for r in res], tv.MAX_ERROR)
    for p, (a, b) in enumerate(pair_images):
        r = res[p]
        ref = guided_match_pair(images[a][1], images[b][1], images[a][0], images[b][0], r["model"], r["model9"], tv.MAX_ERROR)
        assert np.array_equal(got[p], ref), p
        assert set(map(tuple, r["inlier_matches"])) <= set(map(tuple, got[p])), p     # guided ⊇ the verifier's inliers
        assert sum(1 for i, j in got[p] if i == j and twins[p][i]) >= 0.9 * twins[p].sum(), p


@lru_cache(maxsize=None)
def three_pairs():
    """Three scenes of at most 300 keypoints, D = 128, as one block of six images: pair p is images (2p, 2p + 1) under the
    specification's own F, H, F -> images, (desc, counts, kps), pairs, models, kinds."""
    images, models = [], []
    for kind, (seed, n, n_unique, planar) in zip("FHF", [(40, 300, 140, False), (41, 300, 140, True), (43, 200, 60, False)]):
        kp1, kp2, d1, d2, _, f9, h9 = scene_models(seed, n, n_unique, planar)
        images += [(kp1, d1), (kp2, d2)]
        models.append(f9 if kind == "F" else h9)
    return images, blocks(images), np.array([[0, 1], [2, 3], [4, 5]], np.int32), np.stack(models), list("FHF")


def test_hip_guided_blocks_in_two_launches_equals_one_launch_and_the_spec():
    """pair_chunk = 2: three pairs in two launches, the second of a single pair."""
    from vit_colmap_amd.matching.exhaustive import hip_guided_blocks

    images, (desc, counts, kps), pairs, models, kinds = three_pairs()
    two = hip_guided_blocks(desc, counts, kps, pairs, models, kinds, tv.MAX_ERROR, pair_chunk=2)
    one = hip_guided_blocks(desc, counts, kps, pairs, models, kinds, tv.MAX_ERROR, pair_chunk=16384)
    assert len(two) == len(one) == 3
    for p, (a, b) in enumerate(pairs):
        ref = guided_match_pair(images[a][1], images[b][1], images[a][0], images[b][0], kinds[p], models[p], tv.MAX_ERROR)
        assert len(ref) > 150 and two[p].dtype == np.uint32
        assert np.array_equal(two[p], one[p]) and np.array_equal(two[p], ref), p


def test_hip_match_blocks_takes_device_tensors_and_host_arrays_alike():
    """The upload and unpack paths that the unguided and the guided function share, in two launches."""
    from vit_colmap_amd.matching.exhaustive import hip_match_blocks

    images, (desc, counts, _), pairs, _, _ = three_pairs()
    from_device = hip_match_blocks(dev(desc), dev(counts), pairs, pair_chunk=2)
    from_host = hip_match_blocks(desc, counts, pairs, pair_chunk=2)
    assert len(from_device) == len(from_host) == 3
    for p, (a, b) in enumerate(pairs):
        ref = mo.match_pair(images[a][1], images[b][1])
        assert len(ref) > 50 and from_device[p].dtype == np.uint32
        assert np.array_equal(from_device[p], from_host[p]) and np.array_equal(from_device[p], ref), p


def test_match_exhaustive_with_and_without_the_flag(tmp_path):
    """Across the two runs: the same `matches` rows and `config`, guided ⊇ unguided inliers.  F and H are compared inside the
    guided run, with what its own verification returned: the verifier's float64 solves accumulate with atomics, so two
    runs on the same database agree on them only to rounding (and on the pure image shift of pair (1, 3), whose F the
    f33 = 1 parametrisation cannot hold, not even that)."""
    from test_guided_spec import dump_db, make_twin_db
    from vit_colmap_amd.matching import match_exhaustive
    from vit_colmap_amd.matching.two_view import verify_pairs
    from vit_colmap_amd.utils.config import MatchingConfig

    is_twin = make_twin_db(tmp_path / "plain.db")
    make_twin_db(tmp_path / "guided.db")
    verified = {}

    def recording_verify(kps, pair_images, pair_ids, lists):
        res = verify_pairs(kps, pair_images, pair_ids, lists)
        for (a, b), r in zip(pair_images, res):                                    # image index -> image id: + 1
            verified[(a + 1, b + 1)] = dict(inliers=r["inlier_matches"].copy(), config=r["config"],
                                            geo=np.concatenate([[float(r["config"])], np.asarray(r["F"]).reshape(-1),
                                                                np.asarray(r["H"]).reshape(-1)]))
        return res

    s0 = match_exhaustive(database_path=str(tmp_path / "plain.db"))
    s1 = match_exhaustive(database_path=str(tmp_path / "guided.db"), verify_fn=recording_verify,
                          matching_options=MatchingConfig(guided_matching=True).to_matching_options())
    assert s0["guided_pairs"] == 0 and s1["guided_pairs"] == s1["verified_pairs"] == s0["verified_pairs"] == 3
    plain, guided = dump_db(tmp_path / "plain.db"), dump_db(tmp_path / "guided.db")
    assert plain.keys() == guided.keys() and len(verified) == 6
    for k in plain:
        got = set(map(tuple, guided[k])) if k[0] == "inl" else None
        if k[0] == "m":
            assert np.array_equal(plain[k], guided[k]), k                          # the matches table is untouched
        elif k[0] == "geo":
            assert plain[k][0] == guided[k][0], k                                  # the same config in both runs
            assert np.array_equal(guided[k], verified[k[1:]]["geo"]), k            # config, F, H: as the verification left them
        else:
            assert set(map(tuple, plain[k])) <= got, k                             # guided ⊇ unguided inliers, every pair
            assert set(map(tuple, verified[k[1:]]["inliers"])) <= got, k           # ... and ⊇ its own run's inliers, exactly
            if verified[k[1:]]["config"] == tv.CONFIG_DEGENERATE:
                assert len(got) == 0, k
    g12 = guided[("inl", 1, 2)]
    assert len(g12) > len(plain[("inl", 1, 2)])
    assert sum(1 for i, j in g12 if i == j and is_twin[i]) >= 0.9 * is_twin.sum()

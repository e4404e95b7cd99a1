"""Guided matching on the CPU: the numpy specification's own properties on scenes with look-alike
descriptors, the option's way from the configuration objects and the command line into match_exhaustive, the host
plumbing with oracle seams (one process and two gloo ranks), and the argument checks of the C entry point."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import matcher_oracle as mo
from oracle import two_view_oracle as tv
from util_guided import guided_match_pair, plain_inliers, twin_descriptors, twin_scene

F_SCENES = [(40, 300, 140, False), (41, 300, 140, True), (42, 512, 200, False), (43, 200, 60, False)]
H_SCENES = [(41, 300, 140, True), (44, 512, 100, True)]


def _check_properties(seed, n, n_unique, planar, kind):
    kp1, kp2, d1, d2, is_twin = twin_scene(seed, n, n_unique, planar)
    raw, m9, inliers = plain_inliers(kp1, kp2, d1, d2, kind)
    assert m9 is not None and len(inliers) >= tv.MIN_NUM_INLIERS
    assert not is_twin[raw[:, 0]].any()                       # the ratio test discards every row that has a look-alike
    g = guided_match_pair(d1, d2, kp1, kp2, kind, m9)
    got = set(map(tuple, g))
    assert set(map(tuple, inliers)) <= got                    # guided ⊇ inliers
    recovered = sum(1 for i, j in got if i == j and is_twin[i])
    wrong = sum(1 for i, j in got if i != j)
    print(f"seed {seed} {kind}: raw {len(raw)} inliers {len(inliers)} guided {len(g)} twins {recovered}/{int(is_twin.sum())} "
          f"wrong {wrong}")
    assert recovered >= 0.9 * is_twin.sum()
    assert wrong == 0
    assert np.array_equal(g[:, 0], np.sort(g[:, 0])) and g.dtype == np.uint32
    return kp1, kp2, d1, d2, m9


@pytest.mark.parametrize("seed,n,n_unique,planar", F_SCENES)
def test_spec_properties_under_the_estimated_f(seed, n, n_unique, planar):
    _check_properties(seed, n, n_unique, planar, "F")


@pytest.mark.parametrize("seed,n,n_unique,planar", H_SCENES)
def test_spec_properties_under_an_h_passed_directly(seed, n, n_unique, planar):
    kp1, kp2, d1, d2, h9 = _check_properties(seed, n, n_unique, planar, "H")
    # wide thresholds, one-way: the homography alone decides, and it leaves every row its true partner
    g = guided_match_pair(d1, d2, kp1, kp2, "H", h9, max_ratio=1.0, max_distance=1.5, cross_check=False)
    assert np.array_equal(g[:, 0], np.arange(n))


@pytest.mark.parametrize("kind", ["F", "H"])
def test_nan_model_admits_nothing(kind):
    kp1, kp2, d1, d2, _ = twin_scene(40, 300, 140)
    assert len(guided_match_pair(d1, d2, kp1, kp2, kind, np.full(9, np.nan, np.float32))) == 0
    assert len(guided_match_pair(d1[:0], d2, kp1[:0], kp2, kind, np.eye(3, dtype=np.float32).reshape(9))) == 0


# ---- the option --------------------------------------------------------------------------------------------------------
def test_option_defaults_off_and_travels_through_the_option_objects():
    from vit_colmap_amd.matching.exhaustive import _guided_option
    from vit_colmap_amd.utils.config import FeatureMatchingOptions, MatchingConfig, SiftMatchingOptions

    assert MatchingConfig().guided_matching is False
    assert SiftMatchingOptions().guided_matching is False and FeatureMatchingOptions().guided_matching is False
    assert not _guided_option(None, None) and not _guided_option(MatchingConfig().to_matching_options(), None)
    on = MatchingConfig(guided_matching=True)
    assert on.to_matching_options().guided_matching and on.to_matching_options().sift.guided_matching
    assert on._to_sift_options_legacy().guided_matching
    assert _guided_option(on.to_matching_options(), None) and _guided_option(None, on._to_sift_options_legacy())
    assert _guided_option(FeatureMatchingOptions(guided_matching=True), None)                    # 3.13: the outer object
    assert _guided_option(FeatureMatchingOptions(sift=SiftMatchingOptions(guided_matching=True)), None)   # 3.12: .sift


def test_match_settings_parses_every_option_shape_once():
    from vit_colmap_amd.matching.exhaustive import MatchSettings
    from vit_colmap_amd.utils.config import FeatureMatchingOptions, MatchingConfig, SiftMatchingOptions

    d = MatchingConfig()
    assert MatchSettings.from_options(None, None) == MatchSettings(float(d.max_ratio), float(d.max_distance), bool(d.cross_check),
                                                                   False, False)                       # None: the defaults
    on = MatchingConfig(max_ratio=0.9, max_distance=0.6, cross_check=False, guided_matching=True, compute_relative_pose=True)
    want = MatchSettings(0.9, 0.6, False, True, True)
    assert MatchSettings.from_options(on.to_matching_options(), None) == want                         # the outer object
    assert MatchSettings.from_options(None, on._to_sift_options_legacy()) == want                      # SIFT options alone
    sift = SiftMatchingOptions(max_ratio=0.9, max_distance=0.6, cross_check=False)
    outer = FeatureMatchingOptions(sift=sift, guided_matching=True)                                   # 3.13: flags on the outer object
    assert MatchSettings.from_options(outer, None) == MatchSettings(0.9, 0.6, False, True, False)
    inner = FeatureMatchingOptions(sift=SiftMatchingOptions(max_ratio=0.9, max_distance=0.6, cross_check=False,
                                                            guided_matching=True, compute_relative_pose=True))
    assert MatchSettings.from_options(inner, None) == want                                            # 3.12: flags on .sift
    for opts in ((on.to_matching_options(), None), (None, on._to_sift_options_legacy()), (inner, None)):
        assert MatchSettings.from_options(*opts, verify=False) == MatchSettings(0.9, 0.6, False, False, False)
    with pytest.raises(Exception):
        want.guided = False                                                                           # frozen


def test_command_line_flag_reaches_the_matching_options(monkeypatch, tmp_path):
    from vit_colmap_amd.pipeline import run_pipeline as rp

    seen = []
    monkeypatch.setattr(rp.Pipeline, "run", lambda self, *a, **k: seen.append(self.config.matching.to_matching_options()))
    base = ["prog", "--images", str(tmp_path), "--output", str(tmp_path), "--db", str(tmp_path / "x.db")]
    monkeypatch.setattr(sys, "argv", base)
    rp.main()
    monkeypatch.setattr(sys, "argv", base + ["--guided-matching"])
    rp.main()
    assert [o.guided_matching for o in seen] == [False, True] and seen[1].sift.guided_matching


# ---- match_exhaustive with oracle seams ------------------------------------------------------------------------------------
def _match_fn(block, counts, pairs, max_ratio, max_distance, cross_check):
    block, counts = np.asarray(block), np.asarray(counts)
    return [mo.match_pair(block[a, : counts[a]], block[b, : counts[b]], max_ratio, max_distance, cross_check) for a, b in pairs]


def _verify_fn(kps, pair_images, pair_ids, lists):
    """oracle/two_view_oracle.verify_pair plus the model whose mask produced the inliers (what matching/two_view.py adds)."""
    out = []
    for (a, b), pid, m in zip(pair_images, pair_ids, lists):
        r = tv.verify_pair(kps[a], kps[b], m, pid)
        if r["config"] != tv.CONFIG_DEGENERATE:
            m = np.asarray(m, np.uint32).reshape(-1, 2)
            pts = np.concatenate([kps[a][m[:, 0], :2], kps[b][m[:, 1], :2]], axis=1).astype(np.float32)
            use_h = r["config"] == tv.CONFIG_PLANAR_OR_PANORAMIC and r["n_h"] > r["n_f"]
            r["model"] = "H" if use_h else "F"
            r["model9"], mask = tv.estimate_model(r["model"], pts, int(pid) & 0xFFFFFFFF, tv.NUM_HYP_H if use_h else tv.NUM_HYP_F)
            assert np.array_equal(m[mask], r["inlier_matches"])
        out.append(r)
    return out


def _guided_fn(block, counts, kp_xy, pairs, models, kinds, max_error, max_ratio, max_distance, cross_check):
    block, counts, kp_xy = np.asarray(block), np.asarray(counts), np.asarray(kp_xy)
    return [guided_match_pair(block[a, : counts[a]], block[b, : counts[b]], kp_xy[a, : counts[a]], kp_xy[b, : counts[b]], k, m9,
                              max_error, max_ratio, max_distance, cross_check)
            for (a, b), m9, k in zip(pairs, models, kinds)]


def make_twin_db(path, n=160, n_unique=70, junk_rows=40):
    """Three views of one twin scene (view 3: view 1 shifted by 3 px) and a fourth image with unrelated descriptors."""
    from vit_colmap_amd.database import ColmapDatabase

    rs = np.random.RandomState(5)
    kp1, kp2, _, _ = tv.synthetic_two_view(45, n, 0.0, False)
    descs = twin_descriptors(rs, n, n_unique, 128, 3)
    db = ColmapDatabase(str(path))
    cam = db.add_pinhole_camera(640, 480, 600, 600, 320, 240)
    for k, (kp, d) in enumerate(zip((kp1, kp2, kp1 + np.float32(3.0)), descs)):
        i = db.add_image(f"v{k}.png", cam)
        db.add_keypoints(i, kp)
        db.add_descriptors(i, d)
    i = db.add_image("junk.png", cam)
    db.add_keypoints(i, (rs.rand(junk_rows, 2) * 400).astype(np.float32))
    db.add_descriptors(i, twin_descriptors(rs, junk_rows, junk_rows, 128, 1)[0])
    db.db.close()
    return np.arange(n) >= n_unique


def dump_db(path):
    from vit_colmap_amd.database import ColmapDatabase

    out = {}
    with ColmapDatabase.open_database(str(path)) as h:
        ids = [im.image_id for im in h.read_all_images()]
        for i in ids:
            for j in ids:
                if i < j:
                    out[("m", i, j)] = h.read_matches(i, j)
                    g = h.read_two_view_geometry(i, j)
                    out[("inl", i, j)] = g["inlier_matches"]
                    out[("geo", i, j)] = np.concatenate([[float(g["config"])], np.asarray(g["F"]).reshape(-1),
                                                         np.asarray(g["H"]).reshape(-1)])
    return out


def _options(guided):
    from vit_colmap_amd.utils.config import MatchingConfig

    return MatchingConfig(guided_matching=guided).to_matching_options()


def test_match_exhaustive_replaces_the_inlier_matches_of_verified_pairs(tmp_path):
    from vit_colmap_amd.matching import match_exhaustive

    is_twin = make_twin_db(tmp_path / "plain.db")
    make_twin_db(tmp_path / "guided.db")
    seams = dict(match_fn=_match_fn, verify_fn=_verify_fn, device="cpu")
    s0 = match_exhaustive(database_path=str(tmp_path / "plain.db"), matching_options=_options(False), **seams)
    s1 = match_exhaustive(database_path=str(tmp_path / "guided.db"), matching_options=_options(True), guided_fn=_guided_fn, **seams)
    assert s0["guided_pairs"] == 0 and s1["guided_pairs"] == s1["verified_pairs"] == s0["verified_pairs"] == 3
    plain, guided = dump_db(tmp_path / "plain.db"), dump_db(tmp_path / "guided.db")
    assert plain.keys() == guided.keys()
    for k in plain:
        if k[0] in ("m", "geo"):                                   # matches, config, F and H stay as they are
            assert np.array_equal(plain[k], guided[k]), k
    for (i, j) in [(1, 2), (1, 3), (2, 3)]:
        a, b = set(map(tuple, plain[("inl", i, j)])), set(map(tuple, guided[("inl", i, j)]))
        assert a <= b and len(b) > len(a), (i, j)
        assert all(x == y for x, y in b)
    assert sum(1 for x, _ in map(tuple, guided[("inl", 1, 2)]) if is_twin[x]) >= 0.9 * is_twin.sum()
    for j in (1, 2, 3):                                            # degenerate pairs keep their empty rows
        assert len(guided[("inl", j, 4)]) == 0 and guided[("geo", j, 4)][0] == tv.CONFIG_DEGENERATE


def test_guided_matching_refuses_blocks_the_kernel_cannot_hold_before_matching(tmp_path):
    from vit_colmap_amd import _lib
    from vit_colmap_amd.database import ColmapDatabase
    from vit_colmap_amd.matching import match_exhaustive

    n = _lib.VC_MAX_KEYPOINTS + 1
    db = ColmapDatabase(str(tmp_path / "big.db"))
    cam = db.add_pinhole_camera(640, 480, 600, 600, 320, 240)
    for k in range(2):
        i = db.add_image(f"b{k}.png", cam)
        db.add_keypoints(i, np.zeros((n, 2), np.float32))
        db.add_descriptors(i, np.zeros((n, 32), np.uint8))
    db.db.close()
    calls = []

    def match_fn(*a):
        calls.append(a)
        return _match_fn(*a)

    with pytest.raises(_lib.HipLibraryError, match="VC_MAX_KEYPOINTS"):
        match_exhaustive(database_path=str(tmp_path / "big.db"), matching_options=_options(True), match_fn=match_fn,
                         verify_fn=_verify_fn, guided_fn=_guided_fn, device="cpu")
    assert not calls


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
        from vit_colmap_amd.matching import match_exhaustive

        s = match_exhaustive(database_path=db_path, matching_options=_options(True), distributed=True, match_fn=_match_fn,
                             verify_fn=_verify_fn, guided_fn=_guided_fn, device="cpu")
        q.put(s["ranks"] == 2 and s["guided_pairs"] == 3)
    finally:
        dist.destroy_process_group()


def test_two_ranks_write_the_single_process_database(tmp_path):
    from vit_colmap_amd.matching import match_exhaustive

    make_twin_db(tmp_path / "single.db")
    make_twin_db(tmp_path / "dist.db")
    match_exhaustive(database_path=str(tmp_path / "single.db"), matching_options=_options(True), match_fn=_match_fn,
                     verify_fn=_verify_fn, guided_fn=_guided_fn, device="cpu")
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
    assert all(results)
    single, sharded = dump_db(tmp_path / "single.db"), dump_db(tmp_path / "dist.db")
    assert single.keys() == sharded.keys()
    for k in single:
        assert np.array_equal(single[k], sharded[k]), k
    assert len(single[("inl", 1, 2)]) > 100


# ---- pipeline.distributed.run_sharded against extract + match_exhaustive: one feature set through both bodies ---------------
SIZES = [(48, 64), (56, 64), (64, 64), (72, 64)]                   # the image's height names its features


def _twin_features(path):
    """The four images of make_twin_db -> {image height: (keypoints, descriptors)}."""
    from vit_colmap_amd.database import ColmapDatabase

    make_twin_db(path)
    with ColmapDatabase.open_database(str(path)) as h:
        ids = [im.image_id for im in h.read_all_images()]
        return {hw[0]: (np.asarray(h.read_keypoints(i), np.float32)[:, :2], h.read_descriptors(i)) for hw, i in zip(SIZES, ids)}


def _verify_with_cameras(kps, pair_images, pair_ids, lists, cameras=None):
    """_verify_fn behind the keyword that a focal-length prior on every camera adds to the seam."""
    assert cameras is not None and len(cameras[0]) == len(cameras[1]) == len(kps) and all(cameras[1])
    return _verify_fn(kps, pair_images, pair_ids, lists)


def _sharded_worker(rank, world, port, tmp, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pathlib import Path

        from vit_colmap_amd.pipeline.distributed import run_sharded

        feats = _twin_features(Path(tmp) / f"features_{rank}.db")
        seen = []

        def match_fn(block, counts, pairs, *a):
            seen.append(type(block) is np.ndarray and type(counts) is np.ndarray)     # a stand-in gets host arrays
            return _match_fn(block, counts, pairs, *a)

        def guided_fn(block, counts, *a):
            seen.append(type(block) is np.ndarray and type(counts) is np.ndarray)
            return _guided_fn(block, counts, *a)

        st = run_sharded(Path(tmp) / "images", Path(tmp) / "sharded.db", "PINHOLE", device="cpu", batch_size=3,
                         feature_fn=lambda imgs: [feats[im.shape[0]] for im in imgs], matching_options=_options(True),
                         match_fn=match_fn, verify_fn=_verify_with_cameras, guided_fn=guided_fn, prior_focal_length=True)
        q.put((len(seen) == 2 and all(seen), st))
    finally:
        dist.destroy_process_group()


def test_two_sharded_ranks_write_the_database_of_extract_and_match_exhaustive(tmp_path):
    from vit_colmap_amd.features.dummy_extractor import DummyExtractor
    from vit_colmap_amd.matching import match_exhaustive
    from vit_colmap_amd.utils import image_io

    (tmp_path / "images").mkdir()
    for k, (h, w) in enumerate(SIZES):
        image_io.imwrite(tmp_path / "images" / f"v{k}.png", np.full((h, w, 3), 40 * k, np.uint8))
    feats = _twin_features(tmp_path / "features.db")

    class TwinExtractor(DummyExtractor):
        prior_focal_length = True

        def features_for(self, height, width):
            return feats[height]

    TwinExtractor().extract(tmp_path / "images", tmp_path / "single.db", "PINHOLE")
    s = match_exhaustive(database_path=str(tmp_path / "single.db"), matching_options=_options(True), match_fn=_match_fn,
                         verify_fn=_verify_with_cameras, guided_fn=_guided_fn, device="cpu")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    single, sharded = dump_db(tmp_path / "single.db"), dump_db(tmp_path / "sharded.db")
    assert single.keys() == sharded.keys() and len(single) == 18
    for k in single:
        assert np.array_equal(single[k], sharded[k]), k
    assert len(single[("inl", 1, 2)]) > 100 and s["guided_pairs"] == s["verified_pairs"] == 3 and s["pairs"] == 6
    for ok, st in results:                                          # rank 0's totals on every rank, and match_exhaustive's
        assert ok and st["ranks"] == 2
        assert {k: st[k] for k in ("pairs", "matches", "verified_pairs", "guided_pairs")} == \
            {k: s[k] for k in ("pairs", "matches", "verified_pairs", "guided_pairs")}
        assert set(s) - {"total_s"} <= set(st)                      # run_sharded's stats carry match_exhaustive's keys


# ---- C ABI ---------------------------------------------------------------------------------------------------------------
def test_entry_point_validates_its_arguments_without_a_gpu():
    from vit_colmap_amd import _lib

    lib = _lib.load()
    assert "vc_match_pairs_guided_u8" in _lib.SIGNATURES
    null = (None, None, 1, 512, 384, None, None, 1, None, None, 4.0, 0.8, 0.7, 1, None, None, None)
    assert lib.vc_match_pairs_guided_u8(*null) == -1
    import ctypes

    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    some = [p, p, 1, 512, 384, p, p, 0, p, p, 4.0, 0.8, 0.7, 1, p, p, None]
    assert lib.vc_match_pairs_guided_u8(*some) == 0                                   # no pairs: nothing to do
    for pos in (0, 1, 5, 6, 8, 9, 14, 15):                                           # every pointer is checked
        args = list(some)
        args[pos] = None
        assert lib.vc_match_pairs_guided_u8(*args) == -1, pos
    for pos, bad in ((2, 0), (3, -1), (4, 0), (7, -1), (10, -1.0), (10, float("nan"))):
        args = list(some)
        args[pos] = bad
        assert lib.vc_match_pairs_guided_u8(*args) == -1, (pos, bad)
    args = list(some)
    args[3], args[7] = _lib.VC_MAX_KEYPOINTS + 1, 1
    assert lib.vc_match_pairs_guided_u8(*args) == -2                                  # VC_ERR_UNSUPPORTED, as vc_match_pairs_u8

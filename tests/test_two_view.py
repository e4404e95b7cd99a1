"""Two-view geometric verification: the oracle's own behaviour on scenes with a known answer
(CPU), and the HIP scoring kernels + batched solver against the oracle (GPU).  Parity with COLMAP's estimator is
unpinned (absent third-party wheel): what is pinned here is the build's published specification."""
import numpy as np
import pytest

from oracle import two_view_oracle as tv


def test_sampler_is_deterministic_distinct_and_in_range():
    idx = tv.sample_indices(1234567, 64, 8, 37, tv.SALT_F)
    assert idx.shape == (64, 8) and idx.min() >= 0 and idx.max() < 37
    assert all(len(set(r)) == 8 for r in idx)
    assert np.array_equal(idx, tv.sample_indices(1234567, 64, 8, 37, tv.SALT_F))
    assert not np.array_equal(idx, tv.sample_indices(1234568, 64, 8, 37, tv.SALT_F))
    tiny = tv.sample_indices(5, 32, 8, 6, tv.SALT_F)          # fewer matches than a sample needs: every hypothesis void
    assert (tiny == -1).all()


@pytest.mark.parametrize("planar,expect", [(False, tv.CONFIG_UNCALIBRATED), (True, tv.CONFIG_PLANAR_OR_PANORAMIC)])
def test_oracle_recovers_the_geometry_of_a_synthetic_scene(planar, expect):
    kp1, kp2, m, is_in = tv.synthetic_two_view(3, 300, 0.3, planar)
    r = tv.verify_pair(kp1, kp2, m, pair_id=2147483647 + 2)
    got, true = set(map(tuple, r["inlier_matches"])), set(map(tuple, m[is_in]))
    assert r["config"] == expect
    assert len(got & true) >= 0.97 * len(true) and len(got - true) <= 0.05 * len(true)
    F = r["F"]
    assert abs(np.linalg.det(F)) < 1e-9 and abs(np.linalg.norm(F) - 1) < 1e-9            # rank 2, unit norm
    x1 = np.c_[kp1[m[is_in][:, 0]], np.ones(is_in.sum())]
    x2 = np.c_[kp2[m[is_in][:, 1]], np.ones(is_in.sum())]
    if not planar:
        l2 = x1 @ F.T                                                                         # epipolar lines in image 2
        dist = np.abs(np.einsum("ni,ni->n", x2, l2)) / np.hypot(l2[:, 0], l2[:, 1])
        assert np.median(dist) < 1.0                                                          # pixels (noise sigma 0.5)


def test_oracle_degenerate_cases():
    kp1, kp2, m, _ = tv.synthetic_two_view(4, 300, 0.3)
    assert tv.verify_pair(kp1, kp2, m[:10], 7)["config"] == tv.CONFIG_DEGENERATE              # too few matches
    rs = np.random.RandomState(0)
    junk = np.stack([rs.permutation(300)[:120], rs.permutation(300)[:120]], axis=1).astype(np.uint32)
    r = tv.verify_pair(kp1, kp2, junk, 7)                                                    # no consistent geometry
    assert r["config"] == tv.CONFIG_DEGENERATE and len(r["inlier_matches"]) == 0
    assert tv.verify_pair(kp1, kp2, np.zeros((0, 2), np.uint32), 7)["config"] == tv.CONFIG_DEGENERATE


def test_database_row_round_trip_and_metrics(tmp_path):
    from vit_colmap_amd.database import ColmapDatabase
    from vit_colmap_amd.utils.export import MetricsExporter, export_metrics, extract_all_metrics

    db = ColmapDatabase(str(tmp_path / "t.db"))
    cam = db.add_pinhole_camera(640, 480, 600, 600, 320, 240)
    for k in range(3):
        i = db.add_image(f"i{k}.png", cam)
        db.add_keypoints(i, np.zeros((50, 2), np.float32))
        db.add_descriptors(i, np.zeros((50, 128), np.uint8))
    m = np.arange(40, dtype=np.uint32).reshape(20, 2)
    F = np.arange(9.0).reshape(3, 3)
    db.db.write_matches(1, 2, m)
    db.db.write_matches(1, 3, m[:5])
    db.db.write_two_view_geometry(1, 2, m[:16], tv.CONFIG_UNCALIBRATED, F=F, H=np.eye(3))
    db.db.write_two_view_geometry(3, 1, m[:0], tv.CONFIG_DEGENERATE)
    g = db.db.read_two_view_geometry(1, 2)
    assert g["config"] == 3 and np.array_equal(g["inlier_matches"], m[:16]) and np.array_equal(g["F"], F)
    g2 = db.db.read_two_view_geometry(2, 1)                                                  # swapped view of the same row
    assert np.array_equal(g2["inlier_matches"], m[:16][:, ::-1]) and np.array_equal(g2["F"], F.T)
    assert db.db.num_verified_image_pairs() == 1 and db.db.num_inlier_matches() == 16
    db.db.close()
    res = extract_all_metrics(tmp_path / "t.db", "DTU", "scan1", "vit", {"camera_model": "PINHOLE"})
    assert res.matching.verified_pairs == 2 and res.matching.total_inlier_matches == 16
    assert res.matching.config_distribution == {"UNCALIBRATED": 1, "DEGENERATE": 1}
    assert abs(res.matching.inlier_ratio - 16 / 25) < 1e-12
    export_metrics(res, tmp_path / "results")
    export_metrics(res, tmp_path / "results")                                                # second run appends a CSV row
    back = MetricsExporter.load_json(tmp_path / "results" / "DTU" / "scan1" / "vit.json")
    assert back.matching.total_inlier_matches == 16 and back.features.total_keypoints == 150
    rows = (tmp_path / "results" / "DTU" / "summary.csv").read_text().strip().splitlines()
    assert len(rows) == 3 and rows[0].startswith("dataset,scene,extractor_type,timestamp,total_images")
    assert rows[0].split(",")[-1] == "avg_reprojection_error" and rows[1].split(",")[:3] == ["DTU", "scan1", "vit"]


@pytest.mark.parametrize("model", ["F", "H"])
def test_a_non_finite_or_zero_denominator_has_no_inliers(model):
    """The scoring rule over a power-of-two scale sweep of a valid model: wherever no intermediate overflows or underflows
    (float64 conditions of util_two_view.sweep_conditions) the decision is the unscaled one, wherever the bound t2 * den
    overflows or the denominator is 0 there is no inlier, and the all-zero matrix has none."""
    import util_two_view as u

    pts, m9 = u.best_hypothesis(model)
    base = tv.inliers_f32(model, m9, pts)
    assert 100 < base.sum() < len(pts)
    all_safe = all_dead = 0
    for k, scaled in zip(u.SCALE_EXPONENTS, u.scale_sweep(m9)):
        safe, dead = u.sweep_conditions(model, m9, k, pts)
        got = tv.inliers_f32(model, scaled, pts)
        assert not (safe & dead).any()
        assert np.array_equal(got[safe], base[safe]), k
        assert not got[dead].any(), k
        all_safe += safe.all()
        all_dead += dead.all()
    assert all_safe >= 20 and all_dead >= 10              # the sweep reaches both regimes on every match
    assert u.sweep_conditions(model, m9, 0, pts)[0].all()
    assert tv.inliers_f32(model, np.zeros(9, np.float32), pts).sum() == 0
    assert tv.inliers_f32(model, np.float32(2.0 ** 72) * m9, pts).sum() == 0       # finite entries, every bound overflows


@pytest.mark.parametrize("model", ["F", "H"])
def test_threshold_set_separates_a_contracted_evaluation_from_the_oracle(model):
    """The condition of the GPU threshold test: on the boundary correspondences an evaluation with fused multiply-adds
    disagrees with the oracle on at least 1 % of the points, so a library built without -ffp-contract=off cannot pass."""
    import util_two_view as u

    m9, pts = u.threshold_set(model)
    assert 4000 <= len(pts) <= 4096 and np.isfinite(pts).all()
    res = u.residual64(model, m9, pts)
    assert np.abs(res / tv.MAX_ERROR - 1).max() < 1e-4         # 2e-5 relative in the radius, float32 rounding of the point
    ref = tv.inliers_f32(model, m9, pts)
    assert 0.3 < ref.mean() < 0.7                              # both sides of the boundary
    assert (u.contracted_inliers(model, m9, pts) != ref).mean() >= 0.01
    # away from the boundary the two evaluations agree: the set, not the emulation, is what separates them
    far, _ = u.scene_hypotheses(model, 51, 1000, model == "H", 64)
    assert (u.contracted_inliers(model, m9, far) != tv.inliers_f32(model, m9, far)).sum() == 0


SAMPLER_SEEDS = [0, 1, 2 ** 31, 2 ** 32 - 1, 1234567, (3 * 2147483647 + 17) % 2 ** 32]      # the last: pair_id_of(3, 17) mod 2^32
SAMPLER_COUNTS = [1, 3, 4, 5, 7, 8, 9, 15, 16, 33, 300, 65536, 2 ** 20 + 3, 2 ** 31 - 1]
SAMPLER_MODELS = [(8, "F"), (4, "H"), (5, "E"), (3, "P")]


def sampler_parity(device):
    """_common._sample_indices against the oracle's sampler, element for element, on `device`."""
    import torch

    from vit_colmap_amd.matching import _common

    assert (3 * 2147483647 + 17) == __import__("vit_colmap_amd.database.colmap_db", fromlist=["pair_id_of"]).pair_id_of(3, 17)
    seeds = [s for s in SAMPLER_SEEDS for _ in SAMPLER_COUNTS]
    counts = [m for _ in SAMPLER_SEEDS for m in SAMPLER_COUNTS]
    for S, name in SAMPLER_MODELS:
        salt = _common.SALT[name]
        got = _common._sample_indices(torch.tensor(seeds, dtype=torch.int64, device=device),
                                      torch.tensor(counts, dtype=torch.int64, device=device), 130, S, salt).cpu().numpy()
        assert got.shape == (len(seeds), 130, S) and got.dtype == np.int64
        for row, (seed, m) in enumerate(zip(seeds, counts)):
            want = tv.sample_indices(seed, 130, S, m, salt)
            assert np.array_equal(got[row], want), (name, seed, m)
            if m < S:
                assert (want == -1).all()
        if S in (8, 4):
            assert salt == {8: tv.SALT_F, 4: tv.SALT_H}[S]
        assert (got[counts.index(300)] >= 0).all()             # not a comparison of voids
        empty = _common._sample_indices(torch.tensor(SAMPLER_SEEDS, dtype=torch.int64, device=device),
                                        torch.zeros(len(SAMPLER_SEEDS), dtype=torch.int64, device=device), 130, S, salt)
        assert empty.shape == (len(SAMPLER_SEEDS), 130, S) and bool((empty == -1).all())


def test_torch_sampler_equals_the_oracle_sampler_on_the_cpu():
    sampler_parity("cpu")


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_scoring_kernels_bit_exact_against_oracle_scoring():
    import torch

    from vit_colmap_amd.matching import two_view as g

    rs = np.random.RandomState(1)
    pts_l, offs, hyps = [], [0], {"F": [], "H": []}
    for p, (n, planar) in enumerate([(300, False), (77, True), (15, False), (1000, False)]):
        kp1, kp2, m, _ = tv.synthetic_two_view(10 + p, n, 0.3, planar)
        pts = np.concatenate([kp1[m[:, 0]], kp2[m[:, 1]]], axis=1).astype(np.float32)
        pts_l.append(pts)
        offs.append(offs[-1] + n)
        for model, k in (("F", 40), ("H", 24)):
            h, _ = tv.hypotheses(model, pts, 99 + p, k)
            h[3] = np.nan                                        # a void hypothesis scores zero
            h[5] = rs.standard_normal(9).astype(np.float32)      # an arbitrary matrix
            hyps[model].append(h)
    pts = torch.from_numpy(np.concatenate(pts_l)).cuda()
    offsets = torch.tensor(offs, dtype=torch.int32, device="cuda")
    for model in ("F", "H"):
        hyp = torch.from_numpy(np.stack(hyps[model])).cuda().contiguous()
        counts = g._score(pts, offsets, hyp, model, tv.MAX_ERROR).cpu().numpy()
        for p in range(4):
            ref = [int(tv.inliers_f32(model, h, pts_l[p]).sum()) for h in hyps[model][p]]
            assert np.array_equal(counts[p], ref), (model, p)
        mask = g._mask(pts, offsets, hyp[:, 0].contiguous(), model, tv.MAX_ERROR).cpu().numpy()
        for p in range(4):
            assert np.array_equal(mask[offs[p]:offs[p + 1]], tv.inliers_f32(model, hyps[model][p][0], pts_l[p]))


@pytest.mark.gpu
def test_verify_pairs_against_oracle_on_synthetic_scenes():
    from vit_colmap_amd.matching.two_view import verify_pairs

    scenes = [tv.synthetic_two_view(20 + i, n, o, pl) for i, (n, o, pl) in enumerate(
        [(300, 0.3, False), (200, 0.5, False), (300, 0.2, True), (60, 0.3, False), (12, 0.0, False), (400, 0.9, False)])]
    kps, pairs, pids, lists = {}, [], [], []
    for i, (kp1, kp2, m, _) in enumerate(scenes):
        kps[2 * i], kps[2 * i + 1] = kp1, kp2
        pairs.append((2 * i, 2 * i + 1))
        pids.append((2 * i + 1) * 2147483647 + 2 * i + 2)
        lists.append(m)
    res = verify_pairs(kps, pairs, pids, lists)
    for i, (kp1, kp2, m, is_in) in enumerate(scenes):
        o = tv.verify_pair(kp1, kp2, m, pids[i])
        r = res[i]
        assert r["config"] == o["config"], (i, r["config"], o["config"], r["n_f"], o["n_f"], r["n_h"], o["n_h"])
        # identical sampler and arithmetic; the 8x8 solves differ in the last bits between LAPACK and the GPU solver,
        # which may move a borderline match across the threshold
        assert abs(r["n_f"] - o["n_f"]) <= max(2, 0.02 * o["n_f"]) and abs(r["n_h"] - o["n_h"]) <= max(2, 0.02 * o["n_h"])
        got, ref = set(map(tuple, r["inlier_matches"])), set(map(tuple, o["inlier_matches"]))
        assert len(got ^ ref) <= max(2, 0.03 * len(ref))
        if o["config"] != tv.CONFIG_DEGENERATE:
            true = set(map(tuple, m[is_in]))
            assert len(got & true) >= 0.95 * len(true)
            assert abs(np.linalg.det(r["F"])) < 1e-9


@pytest.mark.gpu
def test_match_exhaustive_writes_two_view_geometries(tmp_path):
    """Descriptors that encode the 3-D point identity: matching finds the true correspondences, verification
    keeps them, and the reference's metrics SQL reads non-empty inlier statistics."""
    from vit_colmap_amd.database import ColmapDatabase
    from vit_colmap_amd.matching import match_exhaustive
    from vit_colmap_amd.utils.metrics import MetricsExtractor

    rs = np.random.RandomState(0)
    n = 250
    base = np.abs(rs.standard_normal((n, 128))).astype(np.float32)
    kp1, kp2, _, _ = tv.synthetic_two_view(30, n, 0.0, False)
    kp3 = kp1 + np.float32(3.0)                                          # a pure image shift of view 1: planar-looking
    db = ColmapDatabase(str(tmp_path / "g.db"))
    cam = db.add_pinhole_camera(640, 480, 600, 600, 320, 240)
    for k, kp in enumerate((kp1, kp2, kp3)):
        d = np.abs(base + 0.05 * rs.standard_normal(base.shape).astype(np.float32))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        i = db.add_image(f"v{k}.png", cam)
        db.add_keypoints(i, kp)
        db.add_descriptors(i, np.clip(d * 512, 0, 255).astype(np.uint8))
    db.db.close()
    stats = match_exhaustive(database_path=str(tmp_path / "g.db"))
    assert stats["pairs"] == 3 and stats["verified_pairs"] == 3
    with ColmapDatabase.open_database(str(tmp_path / "g.db")) as h:
        g12, g13 = h.read_two_view_geometry(1, 2), h.read_two_view_geometry(1, 3)
        assert g12["config"] == tv.CONFIG_UNCALIBRATED and len(g12["inlier_matches"]) > 200
        assert g13["config"] == tv.CONFIG_PLANAR_OR_PANORAMIC
        assert np.array_equal(g12["inlier_matches"][:, 0], g12["inlier_matches"][:, 1])   # true correspondences
    mm = MetricsExtractor(tmp_path / "g.db").extract_matching_metrics()
    assert mm.verified_pairs == 3 and mm.inlier_ratio > 0.9 and mm.config_distribution.get("UNCALIBRATED", 0) >= 1

"""The hybrid extractor on the device: SIFT as a detector, the three device detectors under ViT descriptors, the batched
path against the per-image one, and `extractor_type="hybrid"` through the pipeline in one process and in two ranks."""
import os
import socket

import numpy as np
import pytest

import util_detect as ud

pytestmark = pytest.mark.gpu

DETECTORS = ["sift", "fast", "gftt"]


def _check_u8(got, ref):
    """The bound of tests/test_hybrid.py, taken from that file: at most 1 LSB on under 0.5 % of the entries."""
    from test_hybrid import _check_u8 as check

    check(got, ref)


def _images(n, w=640, h=480):
    return [ud.noisy_checkerboard(k, w, h, amp=20 if k % 2 else 40) for k in range(n)]


# ---- SIFT as a detector ------------------------------------------------------------------------------------------------
def test_sift_detector_equals_the_extractors_positions_and_runs_no_descriptor_kernel(monkeypatch):
    import torch

    from vit_colmap_amd import _lib
    from vit_colmap_amd.features import sift_extractor as se

    imgs = _images(2) + [ud.rectangles()]
    batch = torch.from_numpy(np.stack(imgs)).cuda()
    full = se.extract_device(batch, se.SiftOptions(max_num_features=20000, upright=True))
    totals = full["count"].cpu().numpy()
    assert totals.min() > 20 and totals.max() < 20000, totals
    cases = {"truncates": int(totals.min()) // 2, "mixed": int(np.sort(totals)[1]), "keeps all": int(totals.max()) + 7}
    refs = {name: se.extract_device(batch, se.SiftOptions(max_num_features=n, upright=True)) for name, n in cases.items()}
    assert (refs["truncates"]["count"].cpu().numpy() == cases["truncates"]).all()        # every image is cut inside an octave
    assert np.array_equal(refs["keeps all"]["count"].cpu().numpy(), totals)

    lib = _lib.load()

    def boom(*a):
        raise AssertionError("the orientation / descriptor kernels must not run for detection")

    monkeypatch.setattr(lib, "vc_sift_describe", boom)
    monkeypatch.setattr(lib, "vc_sift_orient", boom)
    for name, n in cases.items():
        xy, count = se.detect_device(batch, n)
        want = refs[name]
        assert xy.shape == (3, n, 2) and xy.dtype == torch.float32
        assert torch.equal(count, want["count"]), name
        assert torch.equal(xy.view(torch.int32), want["keypoints"][..., :2].contiguous().view(torch.int32)), name   # to the bit


# ---- the extractor -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def extractors():
    """One ViT-S hybrid extractor per detector, built with the default arguments but the model (no cv2 here)."""
    from vit_colmap_amd.features.hybrid_extractor import HybridViTExtractor

    return {d: HybridViTExtractor(model_name="dinov2_vits14", descriptor_dim=128, detector_type=d) for d in DETECTORS}


def _detector_points(detector, img, n=2048):
    if detector == "fast":
        return ud.fast_detect(ud.grey_u8(img), 10, n)[0]
    if detector == "gftt":
        return ud.gftt_detect(ud.grey_u8(img), n)[0]
    import torch

    from vit_colmap_amd.features import sift_extractor as se

    r = se.extract_device(torch.from_numpy(img[None]).cuda(), se.SiftOptions(max_num_features=n, upright=True))
    return r["keypoints"][0, : int(r["count"][0]), :2].cpu().numpy()


@pytest.mark.parametrize("detector", DETECTORS)
def test_extractor_detects_and_describes_without_opencv(extractors, detector):
    ex = extractors[detector]
    assert ex.detector_backend == "hip" and ex.batch_size > 1
    img = ud.noisy_checkerboard(1, amp=20)
    kp, desc = ex._run_inference(img)
    want = _detector_points(detector, img)
    assert kp.dtype == np.float32 and np.array_equal(kp, want) and len(kp) > 100        # the detector's own points
    assert desc.dtype == np.uint8 and desc.shape == (len(kp), 128)
    assert tuple(ex.descriptor_projection.shape) == (384, 128)
    _check_u8(desc, ex.describe_batch([img], [kp])[0])                                  # descriptors at exactly these points


def _batch_and_singles(model_name, dim, detector):
    from vit_colmap_amd.features.hybrid_extractor import HybridViTExtractor

    proj = np.random.RandomState(5).randn(dim, 128).astype(np.float32) / np.sqrt(dim)
    ex = HybridViTExtractor(model_name=model_name, descriptor_dim=128, detector_type=detector, projection=proj)
    imgs = _images(4) + [ud.rectangles()]
    imgs.insert(2, np.full((480, 640, 3), 128, np.uint8))                 # nothing to detect in slot 2
    batch = ex._run_batch(imgs)                                            # 6 images, one call
    assert len(batch) == 6
    singles = [ex._run_inference(img) for img in imgs]
    for i, (kp, desc) in enumerate(singles):
        assert np.array_equal(batch[i][0], kp), i                          # the detectors are functions of the image alone
        assert batch[i][0].shape == (len(kp), 2) and batch[i][1].shape == (len(kp), 128) == desc.shape
    assert batch[2][0].shape == (0, 2) and batch[2][1].shape == (0, 128) and batch[2][1].dtype == np.uint8
    assert all(len(batch[i][0]) > 10 for i in (0, 1, 3, 4, 5))
    return ex, imgs, batch, singles


@pytest.mark.parametrize("detector", DETECTORS)
def test_batch_equals_image_by_image_and_an_empty_image_disturbs_nothing(detector):
    """The class's default backbone (ViT-B/14, the one the pipeline builds): every GEMM epilogue and the attention are
    functions of the row / the image alone, so a batch equals its images run one by one, descriptors included."""
    ex, imgs, batch, singles = _batch_and_singles("dinov2_vitb14", 768, detector)
    for i, (kp, desc) in enumerate(singles):
        assert np.array_equal(batch[i][1], desc), i
    five = ex._run_batch(imgs[:2] + imgs[3:])                              # 5 images equal 5 calls, without the empty one
    for got, i in zip(five, (0, 1, 3, 4, 5)):
        assert np.array_equal(got[0], singles[i][0]) and np.array_equal(got[1], singles[i][1])


@pytest.mark.parametrize("detector", DETECTORS)
def test_batch_on_vits_keeps_the_points_and_the_first_images_descriptors(detector, capsys):
    """ViT-S runs the fused MLP of csrc/gemm.hip, whose 32-row tiles span image boundaries (1531 rows per image) and
    choose the table or the float GELU per wave (vit/dinov2.py, "batch shards"): the tokens of an image depend in the
    last bf16 bit on where its rows fall in the tiles, so only the first image of a batch is aligned as it is alone.
    Asserted: the points of every image and the descriptors of the first one, exactly.  The other images' descriptors
    are compared and the figures printed, not bounded here: that is the backbone's property, pinned in
    tests/test_vit_gpu.py.  Measured on an MI355X (6 frames of 640x480, 128-D): images 1, 3, 4, 5 differ from their
    single-image run in 0.29 % - 15.0 % of the uint8 entries, by at most 11."""
    ex, imgs, batch, singles = _batch_and_singles("dinov2_vits14", 384, detector)
    assert np.array_equal(batch[0][1], singles[0][1])
    with capsys.disabled():
        for i in (1, 3, 4, 5):
            diff = np.abs(batch[i][1].astype(int) - singles[i][1].astype(int))
            print(f"\n[vits batch vs alone] {detector} image {i}: max |diff| {diff.max()} LSB, "
                  f"{(diff != 0).mean():.4%} of entries differ", end="")


# ---- the pipeline ------------------------------------------------------------------------------------------------------
def _write_images(d, n=6):
    from vit_colmap_amd.utils import image_io

    d.mkdir()
    for k, img in enumerate(_images(n)):
        image_io.imwrite(d / f"img_{k}.png", img)


def _run_pipeline(tmp, db_name, detector):
    from vit_colmap_amd.pipeline.run_pipeline import Pipeline
    from vit_colmap_amd.utils.config import Config

    cfg = Config()
    cfg.extractor.extractor_type, cfg.extractor.detector_type = "hybrid", detector
    cfg.do_reconstruction = False
    pipe = Pipeline(cfg)
    pipe.run(tmp / "images", tmp / "out", tmp / db_name, dataset="synthetic", scene="boards", results_dir=tmp / "results")
    return pipe


@pytest.mark.parametrize("detector", DETECTORS)
def test_pipeline_selects_the_hybrid_extractor(tmp_path, detector):
    from vit_colmap_amd.database import ColmapDatabase

    _write_images(tmp_path / "images")
    _run_pipeline(tmp_path, "h.db", detector)
    with ColmapDatabase.open_database(str(tmp_path / "h.db")) as h:
        assert h.num_images() == 6
        for i in range(1, 7):
            kp, d = h.read_keypoints(i), h.read_descriptors(i)
            assert kp.shape[1] == 2 and 100 < len(kp) <= 2048 and d.shape == (len(kp), 256) and d.dtype == np.uint8
        assert h.num_matched_image_pairs() == 15
    assert (tmp_path / "results" / "synthetic" / "boards" / "hybrid.json").exists()     # the metrics carry the extractor's name


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_worker(rank, world, port, tmp, q):
    import torch
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pathlib import Path

        torch.cuda.set_device(0)
        pipe = _run_pipeline(Path(tmp), "two_ranks.db", "sift")
        st = pipe.last_stats
        q.put(bool(st["images"] == 6 and st["pairs"] == 15 and st["ranks"] == 2))
    finally:
        dist.destroy_process_group()


def test_two_ranks_write_the_single_process_database(tmp_path):
    """Both ranks project with the matrix rank 0 fits from the first file (`sync_projection`), which is the matrix a
    single process fits: the two databases are equal, descriptors included."""
    import torch.multiprocessing as mp

    from test_dist_cpu import _dump_db, _same_db

    _write_images(tmp_path / "images")
    _run_pipeline(tmp_path, "single.db", "sift")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]   # 2 processes on the GPU
    for p in procs:
        p.start()
    results = [q.get(timeout=400) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(results)
    single, two = _dump_db(tmp_path / "single.db"), _dump_db(tmp_path / "two_ranks.db")
    assert single[("d", 1)].shape[1] == 256 and single["pairs"] == 15
    _same_db(single, two)

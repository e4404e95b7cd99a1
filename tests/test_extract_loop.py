"""The files -> database loop of every extractor's `extract()` and of `run_sharded`, on the host: the device calls are
replaced by deterministic fakes, so the loop's policy (file order, unreadable files, batches of equal-size images, a failing
image, an image without keypoints, camera rows) is pinned without a GPU."""
import sqlite3

import numpy as np
import pytest

from vit_colmap_amd import _lib
from vit_colmap_amd.database import colmap_db
from vit_colmap_amd.utils import image_io

A, B = (30, 40), (20, 28)                       # (height, width) of the two image sizes
SIZES = {0: A, 1: A, 2: A, 3: B, 5: A, 6: A, 7: A}
UNREADABLE, FAILING, EMPTY = 4, 6, 7
BATCH = 2


def image_dir(tmp_path):
    """im00 .. im07: sizes A A A B, an unreadable file, A A A; image k is filled with the value k."""
    d = tmp_path / "images"
    d.mkdir()
    for k, (h, w) in SIZES.items():
        img = np.full((h, w, 3), k, np.uint8)
        img[0, 0] = (k, 100 + k, 200 + k)
        image_io.imwrite(d / f"im{k:02d}.png", img)
    (d / f"im{UNREADABLE:02d}.png").write_bytes(b"not an image")
    return d


def rows(k, kdim, dim):
    """The fake features of image k (none for EMPTY)."""
    n = 0 if k == EMPTY else k + 1
    kp = (np.arange(n * kdim, dtype=np.float32).reshape(n, kdim) + 0.25 * k).astype(np.float32)
    desc = ((np.arange(n * dim) * 7 + k) % 256).astype(np.uint8).reshape(n, dim)
    return kp, desc


class Fake:
    """Host stand-in for an extractor's device calls; `calls` records what it was given, in order."""

    def __init__(self, kdim, dim, fail=FAILING):
        self.kdim, self.dim, self.fail, self.calls = kdim, dim, fail, []

    def results(self, images):
        ks = [int(im[0, 0, 0]) for im in images]
        if self.fail in ks:
            raise ValueError(f"fake failure on image {self.fail}")
        return [rows(k, self.kdim, self.dim) for k in ks]

    def run_batch(self, images):
        self.calls.append(("run", [int(im[0, 0, 0]) for im in images]))
        return self.results(images)

    def run_inference(self, image):
        self.calls.append(("inference", [int(image[0, 0, 0])]))
        return self.results([image])[0]


def dump(path):
    con = sqlite3.connect(str(path))
    try:
        out = {t: con.execute(f"SELECT * FROM {t} ORDER BY 1").fetchall() for t in ("cameras", "images")}
        for t in ("keypoints", "descriptors"):
            out[t] = con.execute(f"SELECT image_id, rows, cols, data FROM {t} ORDER BY image_id").fetchall()
    finally:
        con.close()
    return out


def camera_row(camera_id, model, hw, params):
    return (camera_id, colmap_db.CAMERA_MODEL_IDS[model], hw[1], hw[0], np.asarray(params, np.float64).tobytes(), 0)


def expected_features(kdim, dim, fail=FAILING):
    """keypoint and descriptor rows: image ids follow the readable files; the failing and the empty image have none."""
    kps, descs = [], []
    for image_id, k in enumerate(sorted(SIZES), start=1):
        if k in (fail, EMPTY):
            continue
        kp, desc = rows(k, kdim, dim)
        kps.append((image_id, len(kp), kdim, kp.tobytes()))
        descs.append((image_id, len(desc), dim, desc.tobytes()))
    return kps, descs


def one_camera(model, params):
    return [camera_row(1, model, A, params)], [(i, f"im{k:02d}.png", 1) for i, k in enumerate(sorted(SIZES), start=1)]


def per_image_cameras(model):
    from vit_colmap_amd.features.sift_extractor import camera_params_for

    cams, imgs = [], []
    for i, k in enumerate(sorted(SIZES), start=1):
        h, w = SIZES[k]
        cams.append(camera_row(i, model, SIZES[k], camera_params_for(model, w, h)))
        imgs.append((i, f"im{k:02d}.png", i))
    return cams, imgs


# the batches of equal-size images (at most BATCH) the device sees; [5, 6] fails and is re-run image by image
BATCHES = [[0, 1], [2], [3], [5, 6], [5], [6], [7]]


def make(kind, monkeypatch, fake_kwargs=None):
    """-> (extractor whose device calls are fakes, the fake, camera model, camera params passed, expected database)."""
    if kind.startswith("vit"):
        from vit_colmap_amd.features.vit_extractor import ViTExtractor

        fake = Fake(2, 64, **(fake_kwargs or {}))
        ex = ViTExtractor.__new__(ViTExtractor)
        ex.model_name, ex.num_keypoints, ex.batch_size = "dinov2_vits14", 64, BATCH
        ex.timings = {"decode_s": 0.0, "gpu_s": 0.0, "db_s": 0.0, "images": 0}
        fail_at = kind.split("-")[1]

        def launch(images):
            fake.calls.append(("launch", [int(im[0, 0, 0]) for im in images]))
            if fail_at == "launch":
                return fake.results(images)
            return images

        def finish(handle):
            if fail_at == "launch":
                return handle
            fake.calls.append(("finish", [int(im[0, 0, 0]) for im in handle]))
            return fake.results(handle)

        ex._launch_batch, ex._finish_batch, ex._run_batch = launch, finish, fake.run_batch
        cams, imgs = one_camera("SIMPLE_PINHOLE", [40, 20, 15])
        return ex, fake, "SIMPLE_PINHOLE", None, (cams, imgs) + expected_features(2, 64, **(fake_kwargs or {}))
    if kind == "trainable":
        from vit_colmap_amd.features.trainable_vit_extractor import TrainableViTExtractor

        fake = Fake(6, 128, **(fake_kwargs or {}))
        ex = TrainableViTExtractor.__new__(TrainableViTExtractor)
        ex.model_name, ex.num_keypoints, ex.score_threshold, ex.nms_radius, ex.batch_size = "dinov2_vits14", 64, 0.0, 4, BATCH
        ex._run_batch = fake.run_batch
        cams, imgs = one_camera("SIMPLE_RADIAL", [40, 20, 15, 0.0])
        return ex, fake, "SIMPLE_RADIAL", None, (cams, imgs) + expected_features(6, 128, **(fake_kwargs or {}))
    if kind == "sift":
        from vit_colmap_amd.features.sift_extractor import SiftExtractor

        fake = Fake(6, 128, **(fake_kwargs or {}))
        ex = SiftExtractor.__new__(SiftExtractor)
        ex.batch_size = BATCH
        ex._run_batch = fake.run_batch
        monkeypatch.setattr(ex, "_require_gpu", lambda: None, raising=False)
        # camera_params is ignored: one camera per image, f = 1.2 max(w, h)
        return (ex, fake, "SIMPLE_PINHOLE", [1.0, 2.0, 3.0],
                per_image_cameras("SIMPLE_PINHOLE") + expected_features(6, 128, **(fake_kwargs or {})))
    assert kind == "hybrid"
    from vit_colmap_amd.features.hybrid_extractor import HybridViTExtractor

    fake = Fake(2, 128, **(fake_kwargs or {}))
    ex = HybridViTExtractor.__new__(HybridViTExtractor)
    ex._run_inference = fake.run_inference
    cams, imgs = one_camera("PINHOLE", [500.0, 510.0, 21.0, 14.0])
    return ex, fake, "PINHOLE", [500.0, 510.0, 21.0, 14.0], (cams, imgs) + expected_features(2, 128, **(fake_kwargs or {}))


def expected_calls(kind):
    if kind == "vit-launch":           # the failing launch is re-run at once, before the next batch is launched
        return [("launch", [0, 1]), ("launch", [2]), ("launch", [3]), ("launch", [5, 6]), ("run", [5]), ("run", [6]),
                ("launch", [7])]
    if kind == "vit-finish":           # batch k - 1 is waited for after batch k was launched
        return [("launch", [0, 1]), ("launch", [2]), ("finish", [0, 1]), ("launch", [3]), ("finish", [2]),
                ("launch", [5, 6]), ("finish", [3]), ("launch", [7]), ("finish", [5, 6]), ("run", [5]), ("run", [6]),
                ("finish", [7])]
    if kind == "hybrid":               # one image at a time
        return [("inference", [k]) for k in sorted(SIZES)]
    return [("run", b) for b in BATCHES]


KINDS = ["vit-launch", "vit-finish", "trainable", "sift", "hybrid"]


@pytest.mark.parametrize("kind", KINDS)
def test_extract_writes_the_database_of_the_file_loop(kind, tmp_path, monkeypatch, capsys):
    d = image_dir(tmp_path)
    ex, fake, model, params, (cams, imgs, kps, descs) = make(kind, monkeypatch)
    ex.extract(d, tmp_path / "db.db", model, params)
    got = dump(tmp_path / "db.db")
    assert got["cameras"] == cams
    assert got["images"] == imgs
    assert got["keypoints"] == kps
    assert got["descriptors"] == descs
    assert fake.calls == expected_calls(kind)
    out = capsys.readouterr().out
    assert f"Error during feature extraction of im{FAILING:02d}.png" in out
    assert f"im{UNREADABLE:02d}.png" in out
    if kind.startswith("vit"):
        assert ex.timings["images"] == len(SIZES) and ex.timings["decode_s"] > 0


@pytest.mark.parametrize("kind", KINDS)
def test_extract_error_conventions(kind, tmp_path, monkeypatch):
    ex, _, model, params, _ = make(kind, monkeypatch)
    empty = tmp_path / "none"
    empty.mkdir()
    with pytest.raises(ValueError, match="No images found"):
        ex.extract(empty, tmp_path / "a.db", model, params)
    (empty / "broken.png").write_bytes(b"not an image")
    image_io.imwrite(empty / "c.png", np.zeros((8, 8, 3), np.uint8))
    with pytest.raises(ValueError, match="Failed to read first image"):
        ex.extract(empty, tmp_path / "b.db", model, params)
    with pytest.raises(ValueError, match="Unsupported camera model"):
        ex.extract(image_dir(tmp_path), tmp_path / "c.db", "FISHEYE")


@pytest.mark.parametrize("kind", KINDS)
def test_unsupported_camera_model_is_rejected_before_the_database_exists(kind, tmp_path, monkeypatch):
    ex, _, _, _, _ = make(kind, monkeypatch)
    with pytest.raises(ValueError, match="Unsupported camera model"):
        ex.extract(image_dir(tmp_path), tmp_path / "db.db", "FISHEYE")
    assert not (tmp_path / "db.db").exists()


@pytest.mark.parametrize("kind", KINDS)
def test_extract_closes_its_database_and_reports_the_traceback(kind, tmp_path, monkeypatch, capsys):
    opened = []
    real_open = colmap_db.SqliteColmapDatabase.open

    def open_(self, path):
        opened.append(self)
        return real_open(self, path)

    monkeypatch.setattr(colmap_db.SqliteColmapDatabase, "open", open_)
    ex, _, model, params, _ = make(kind, monkeypatch)
    ex.extract(image_dir(tmp_path), tmp_path / "db.db", model, params)
    assert len(opened) == 1 and opened[0]._conn is None
    err = capsys.readouterr().err
    assert "Traceback" in err and f"fake failure on image {FAILING}" in err


@pytest.mark.parametrize("kind", KINDS)
def test_library_errors_propagate_from_the_per_image_retry(kind, tmp_path, monkeypatch):
    """A missing library or device is never a per-image problem: a HipLibraryError from the re-run of a failing batch
    ends the extraction."""
    ex, fake, model, params, _ = make(kind, monkeypatch)
    results = fake.results

    def results_then_library_error(images):
        if len(images) == 1 and int(images[0][0, 0, 0]) == FAILING:
            raise _lib.HipLibraryError("no device")
        return results(images)

    fake.results = results_then_library_error
    with pytest.raises(_lib.HipLibraryError):
        ex.extract(image_dir(tmp_path), tmp_path / "db.db", model, params)


def test_sharded_one_rank_writes_the_database_of_extract(tmp_path, monkeypatch):
    """run_sharded on one rank with the SIFT extractor's camera policy writes what SiftExtractor.extract writes,
    cameras included."""
    from vit_colmap_amd.pipeline.distributed import run_sharded

    d = image_dir(tmp_path)
    ex, fake, model, params, expected = make("sift", monkeypatch, dict(fail=None))
    ex.extract(d, tmp_path / "a.db", model, params)
    run_sharded(d, tmp_path / "b.db", model, params, feature_fn=fake.run_batch, do_matching=False, device="cpu",
                batch_size=BATCH, camera_params_for=ex.camera_params_for, camera_per_image=ex.camera_per_image)
    a, b = dump(tmp_path / "a.db"), dump(tmp_path / "b.db")
    assert a == b
    assert (a["cameras"], a["images"], a["keypoints"], a["descriptors"]) == expected

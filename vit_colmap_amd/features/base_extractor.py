"""Extractor plugin API — identical contract to reference vit_colmap/features/base_extractor.py:6-16 — and the one
files -> database loop behind every extractor's `extract()` (`extract_to_database`), whose pieces `run_sharded` shares."""
import os
import time
import traceback
from abc import ABC, abstractmethod
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import Optional

import numpy as np

from .. import _lib
from ..database.colmap_db import Camera, ColmapDatabase
from ..utils import image_io


class BaseExtractor(ABC):
    prior_focal_length = False     # True: the camera rows this extractor writes carry `has_prior_focal_length`

    @abstractmethod
    def extract(
        self,
        image_dir: Path,
        db_path: Path,
        camera_model: str,
        camera_params: Optional[list[float]] = None,
    ) -> None:
        """Process images in `image_dir` and write features into the COLMAP database at `db_path`."""
        raise NotImplementedError


IMAGE_EXTENSIONS = {".jpg", ".jpeg", ".png", ".bmp", ".tiff", ".tif"}  # vit_extractor.py:684


def list_images(image_dir: Path, extensions=IMAGE_EXTENSIONS):
    """Sorted image files of a directory (vit_extractor.py:684-687, dummy_extractor.py:39-43)."""
    return sorted(f for f in Path(image_dir).iterdir() if f.suffix.lower() in extensions)


def default_camera_params(camera_model: str, width: int, height: int) -> list:
    """f = max(w, h), principal point at the centre (vit_extractor.py:706-716)."""
    f = max(width, height)
    if camera_model == "SIMPLE_PINHOLE":
        return [f, width / 2.0, height / 2.0]
    if camera_model == "PINHOLE":
        return [f, f, width / 2.0, height / 2.0]
    raise ValueError(f"Unsupported camera model: {camera_model}")


def camera_policy(camera_model, camera_params, first_hw, params_for=default_camera_params, per_image=False,
                  prior_focal_length=False):
    """-> camera_of(height, width): the Camera of an image.  One camera for all images (the same object), of the first
    image's size, with `camera_params` or else `params_for(camera_model, w, h)`; with `per_image`, one camera per image
    from `params_for` and `camera_params` ignored (COLMAP's ImageReader with CameraMode.AUTO).  ValueError for a model
    `params_for` does not support, raised here, before any database is opened.  `prior_focal_length` marks every camera
    row as carrying trusted intrinsics (`has_prior_focal_length`: the calibrated branch of verification)."""
    h0, w0 = (int(x) for x in first_hw)
    prior = bool(prior_focal_length)
    if per_image:
        params_for(camera_model, w0, h0)
        return lambda h, w: Camera(model=camera_model, width=w, height=h, params=params_for(camera_model, w, h),
                                   has_prior_focal_length=prior)
    camera = Camera(model=camera_model, width=w0, height=h0,
                    params=camera_params if camera_params is not None else params_for(camera_model, w0, h0),
                    has_prior_focal_length=prior)
    return lambda h, w: camera


def add_image_row(db, name, camera):
    """The image row of a readable file, behind its camera's row (written the first time the camera is used)."""
    if camera.camera_id is None:
        camera.camera_id = db.db.write_camera(camera)
    return db.add_image(name, camera_id=camera.camera_id)


def image_batches(files, batch_size, first=None, timings=None):
    """Consecutive equal-size batches of at most `batch_size` readable images of `files`, in file order, as lists of
    (index in files, path, BGR uint8 array).  A thread pool decodes up to 2 * batch_size files ahead (Pillow and OpenCV
    release the GIL); an unreadable file is reported and left out.  `first`: files[0], already decoded; the decode time
    of the others is added to timings["decode_s"]."""
    def decode(path):
        t0 = time.perf_counter()
        img = image_io.imread(path)
        return img, time.perf_counter() - t0

    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 2)
    pool = ThreadPoolExecutor(max(1, min(16, cores - 1)))
    start = 0 if first is None else 1
    ahead = deque(pool.submit(decode, f) for f in files[start:start + 2 * batch_size])
    nxt = start + len(ahead)
    batch = []
    try:
        for idx, path in enumerate(files):
            if idx < start:
                img = first
            else:
                img, dt = ahead.popleft().result()
                if timings is not None:
                    timings["decode_s"] += dt
                if nxt < len(files):
                    ahead.append(pool.submit(decode, files[nxt]))
                    nxt += 1
            if img is None:
                print(f"[{idx + 1}/{len(files)}] {path.name}: ⚠ failed to read image, skipping")
                continue
            if batch and (batch[0][2].shape != img.shape or len(batch) >= batch_size):
                yield batch
                batch = []
            batch.append((idx, path, img))
        if batch:
            yield batch
    finally:
        pool.shutdown(wait=False, cancel_futures=True)


def host_rows(count, keypoints, descriptors):
    """Padded batch result tensors (count (B,), keypoints (B, K, k), descriptors (B, K, D)), on the device or the host
    -> per image (keypoints (N_i, k) float32, descriptors (N_i, D) uint8)."""
    count, keypoints, descriptors = (t.cpu().numpy() for t in (count, keypoints, descriptors))
    return [(keypoints[i, :n].astype(np.float32), descriptors[i, :n].copy()) for i, n in enumerate(count)]


def _one_by_one(run_batch, items, error):
    """Results of a batch that raised `error`, re-run image by image (a batch of one image is not run again); a failing
    image gets None and is reported with its traceback."""
    results = []
    for _, name, img in items:
        try:
            if len(items) == 1:
                raise error
            results.append(run_batch([img])[0])
        except _lib.HipLibraryError:
            raise
        except Exception as e:  # noqa: BLE001
            print(f"  ✗ Error during feature extraction of {name}: {e}")
            traceback.print_exception(e)
            results.append(None)
    return results


def extract_to_database(extractor, image_dir, db_path, camera_model, camera_params=None):
    """The side effects of the plugin API's `extract` (reference vit_extractor.py:655-768), for every extractor:
      * the sorted image files of `image_dir` (`extractor.image_extensions` if set); ValueError for none, for an unreadable
        first file and for an unsupported camera model, before the database file is created;
      * camera rows by the extractor's `camera_params_for` / `camera_per_image` (`camera_policy`);
      * one image row per readable file, in file order, before inference; none for an unreadable file;
      * batches of equal-size images, at most `extractor.batch_size`, through `extractor._launch_batch` (returns at once)
        and `_finish_batch` (waits): the rows of batch k - 1 are written while batch k runs.  Without that pair,
        `_run_batch` is the launch and its results are the finish;
      * a failing batch (anything but a HipLibraryError: a missing library or device is never a per-image problem) is
        re-run image by image through the synchronous `_run_batch` (`_launch_batch`'s staging buffers may belong to the
        batch in flight); a failing image keeps its row and gets no features;
      * no keypoint / descriptor rows for an image without keypoints; a commit at the end; the database is closed.
    Host seconds spent decoding, launching / waiting and writing, and the image count, are added to
    `extractor.timings` if it has that dict."""
    timings = getattr(extractor, "timings", None) or {"decode_s": 0.0, "gpu_s": 0.0, "db_s": 0.0, "images": 0}
    launch, finish = getattr(extractor, "_launch_batch", None), getattr(extractor, "_finish_batch", None)
    if launch is None:
        launch, finish = extractor._run_batch, (lambda results: results)
    files = list_images(image_dir, getattr(extractor, "image_extensions", IMAGE_EXTENSIONS))
    if not files:
        raise ValueError(f"No images found in {image_dir}")
    print(f"Found {len(files)} images")
    first = image_io.imread(files[0])
    if first is None:
        raise ValueError(f"Failed to read first image: {files[0]}")
    camera_of = camera_policy(camera_model, camera_params, first.shape[:2], extractor.camera_params_for,
                              extractor.camera_per_image, getattr(extractor, "prior_focal_length", False))

    def write_rows(items, results):
        t0 = time.perf_counter()
        for (image_id, name, _), r in zip(items, results):
            if r is None:
                continue
            keypoints, descriptors = r
            print(f"  {name}: {len(keypoints)} keypoints, descriptors {descriptors.shape}")
            if len(keypoints) == 0:
                print("  ⚠ Warning: No keypoints extracted")
                continue
            db.add_keypoints(image_id, keypoints)
            db.add_descriptors(image_id, descriptors)
        timings["db_s"] += time.perf_counter() - t0
        timings["images"] += len(items)

    def settle(items, handle, error):
        """Wait for a launched batch, or take the error its launch raised, and write its rows."""
        t0 = time.perf_counter()
        try:
            if error is not None:
                raise error
            results = finish(handle)
        except _lib.HipLibraryError:
            raise
        except Exception as e:  # noqa: BLE001
            results = _one_by_one(extractor._run_batch, items, e)
        timings["gpu_s"] += time.perf_counter() - t0           # host time spent waiting for the GPU
        write_rows(items, results)

    db = ColmapDatabase(str(db_path))
    batches = image_batches(files, extractor.batch_size, first, timings)
    in_flight = None                                            # (items, handle, None) of the batch launched last
    try:
        for batch in batches:
            items = [(add_image_row(db, path.name, camera_of(*img.shape[:2])), path.name, img) for _, path, img in batch]
            t0 = time.perf_counter()
            try:
                handle, error = launch([img for _, _, img in items]), None
            except _lib.HipLibraryError:
                raise
            except Exception as e:  # noqa: BLE001
                handle, error = None, e
            timings["gpu_s"] += time.perf_counter() - t0
            if in_flight is not None:
                settle(*in_flight)                              # batch k - 1: its rows are written while batch k runs
                in_flight = None
            if error is None:
                in_flight = (items, handle, None)
            else:
                settle(items, None, error)                      # a failed launch is re-run at once, no batch in flight
        if in_flight is not None:
            settle(*in_flight)
        db.commit()
    finally:
        batches.close()
        db.db.close()

"""bench.py's rank handling (no GPU needed): a run that cannot have the ranks --gpus asks for must fail loudly,
never print a line with fewer GPUs."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True,
                          text=True, timeout=300)


def test_more_gpus_than_the_node_has_is_refused():
    import torch

    n = torch.cuda.device_count() + 1
    r = _run(["--gpus", str(max(n, 2)), "--steps", "1", "--warmup", "0"])
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert "refusing" in r.stderr and not r.stdout.strip()


def test_launcher_world_size_must_equal_gpus():
    r = _run(["--gpus", "2", "--steps", "1"], {"WORLD_SIZE": "4", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2 and "WORLD_SIZE=4" in r.stderr and not r.stdout.strip()
    r = _run(["--gpus", "8", "--steps", "1"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2 and not r.stdout.strip()


def test_gpu_leg_of_bench_does_not_import_the_oracle():
    """Only cpu_baseline() may touch oracle/ (it is the checker / baseline, never the product or its data)."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    head, _, tail = src.partition("def cpu_baseline(")
    body, _, rest = tail.partition("\ndef ")
    assert "oracle" not in head.split('"""', 2)[2] and "from oracle" not in rest and "import oracle" not in rest
    assert "from oracle" in body


def test_default_workloads_strong_scaling_on_the_200_image_set():
    """--gpus N > 1 measures north_star's experiment (the fixed 200-image set, strong scaling); one GPU
    keeps configs[1] (50 images); --weak keeps the old 50-per-GPU experiment; c5 is one GPU's share of configs[4]."""
    sys.path.insert(0, ROOT)
    import bench

    assert bench.plan_job("c2", 1) == (50, "strong")
    for n in (2, 4, 8):
        assert bench.plan_job("c2", n) == (200, "strong")
        assert bench.plan_job("c2", n, weak=True) == (50 * n, "weak")
    assert bench.plan_job("c2", 1, images_total=200) == (200, "strong")      # the N = 1 anchor of the scaling curve
    assert bench.plan_job("c5", 1) == (63, "strong") and bench.plan_job("c5", 8) == (504, "weak")
    import pytest

    with pytest.raises(ValueError):
        bench.plan_job("c2", 2, images_total=100, weak=True)
    with pytest.raises(ValueError):
        bench.plan_job("c2", 8, images_total=10)


def test_contradicting_flags_are_refused_before_any_gpu_call():
    r = _run(["--gpus", "1", "--weak", "--images-total", "100"])
    assert r.returncode == 2 and "exclude" in r.stderr and not r.stdout.strip()
    r = _run(["--gpus", "1", "--images-total", "1"])
    assert r.returncode == 2 and not r.stdout.strip()


def test_plain_run_is_lean_by_default(monkeypatch):
    """Everything beyond the headline runs behind --full; --dump-outputs is opt-in."""
    sys.path.insert(0, ROOT)
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse_args()
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse_args()
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_float_arrays_masked_and_within_64_mb(tmp_path):
    """--dump-outputs writes float32 / float64 .npy files; entries behind a count are fixed (0 / -1), so the files depend
    only on what was computed; an output larger than its share of 64 MB is a seeded sample of its rows."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import bench

    g = torch.Generator().manual_seed(0)
    for B, K, D, P in ((50, 512, 384, 1225), (200, 2048, 256, 19900)):
        res = {"keypoints": torch.rand(B, K, 2, generator=g),
               "desc_u8": torch.randint(0, 256, (B, K, D), dtype=torch.uint8, generator=g),
               "count": torch.randint(0, K + 1, (B,), dtype=torch.int32, generator=g)}
        m = torch.randint(0, K, (P, K, 2), dtype=torch.int32, generator=g)
        c = torch.randint(0, K + 1, (P,), dtype=torch.int32, generator=g)
        out = tmp_path / f"b{B}"
        bench.dump_outputs(str(out), res, B, m, c)
        files = {p.name: np.load(p) for p in out.iterdir()}
        assert sum(p.stat().st_size for p in out.iterdir()) <= 64e6
        assert all(a.dtype in (np.float32, np.float64) for a in files.values())
        assert np.array_equal(files["keypoint_counts.npy"], res["count"].numpy())
        assert np.array_equal(files["match_counts.npy"], c.numpy())
        rows = files["descriptors_rows.npy"].astype(np.int64) if "descriptors_rows.npy" in files else np.arange(B)
        d = files["descriptors.npy"]
        for i, b in enumerate(rows):
            n = int(res["count"][b])
            assert np.array_equal(d[i, :n], res["desc_u8"][b, :n].numpy()) and not d[i, n:].any()
        prow = files["matches_rows.npy"].astype(np.int64) if "matches_rows.npy" in files else np.arange(P)
        mm = files["matches.npy"]
        for i, p in enumerate(prow[:64]):
            n = int(c[p])
            assert np.array_equal(mm[i, :n], m[p, :n].numpy()) and (mm[i, n:] == -1).all()
    assert "matches_rows.npy" in files and len(files["matches_rows.npy"]) == len(files["matches.npy"])

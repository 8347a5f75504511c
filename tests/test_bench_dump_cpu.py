"""bench.py's --dump-outputs writer and the plain / --full split of its arguments (no GPU):
every array lands as float32 or float64 with integer words exact, the files stay within the
budget by a sample that is the same from call to call, and a plain run asks for none of the
extra readings."""
import os
import sys

import numpy as np
import torch

import bench


def _arrays(n):
    g = torch.Generator().manual_seed(3)
    return {"obs": torch.randint(-2**31, 2**31 - 1, (8 * n,), dtype=torch.int32, generator=g),
            "actions": torch.randint(0, 5, (n,), dtype=torch.int32, generator=g),
            "reward": torch.rand(n, dtype=torch.float64, generator=g),
            "done": (torch.rand(n, generator=g) < 0.1).to(torch.uint8),
            "online_params": torch.rand(1000, dtype=torch.float32, generator=g)}


def test_dump_within_budget_is_whole_and_exact(tmp_path):
    arrs = _arrays(4096)
    bench.dump_outputs(str(tmp_path), arrs, rank=0, world=1)
    assert sorted(os.listdir(tmp_path)) == sorted(k + ".npy" for k in arrs)
    for k, t in arrs.items():
        a = np.load(tmp_path / (k + ".npy"))
        assert a.dtype == (np.float64 if t.dtype in (torch.int32, torch.float64) else np.float32)
        assert a.shape == (t.numel(),) and np.array_equal(a, t.numpy().astype(a.dtype))
    assert np.array_equal(np.load(tmp_path / "obs.npy").astype(np.int64), arrs["obs"].numpy().astype(np.int64))


def test_dump_beyond_budget_is_a_fixed_sample(tmp_path, monkeypatch):
    arrs = _arrays(4096)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 64 << 10)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrs, rank=1, world=2)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(k + "_rank1.npy" for k in arrs)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) <= (64 << 10) // 2
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert np.array_equal(a, b)
        full = arrs[f[:-len("_rank1.npy")]].numpy().astype(a.dtype)
        assert a.size <= full.size and np.isin(a, full).all()
    assert np.load(tmp_path / "a" / "obs_rank1.npy").size < arrs["obs"].numel()  # cut to a sample
    assert np.load(tmp_path / "a" / "online_params_rank1.npy").size == 1000  # within its share: whole


def test_plain_run_asks_for_no_extra_reading(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert not a.full and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    assert (a.other_steps, a.env_steps, a.start_steps, a.total_reading, a.no_cpu) == (0, 0, 0, 0, True)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d" and not a.no_cpu
    assert a.other_steps > 0 and a.env_steps > 0 and a.start_steps > 0 and a.total_reading > 0

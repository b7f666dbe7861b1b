"""bench.py --dump-outputs and the plain / --full split.

CPU: the sampler behind the dumped arrays.  GPU: one plain run of the 228M step
on a small batch, in this process (about 6 s, nearly all of it building the
model): the files it writes, and that its line holds the headline fields and
none of the legs that take runs of their own."""
import json
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402


def test_dump_array_whole_when_small():
    t = torch.arange(24, dtype=torch.bfloat16).reshape(2, 3, 4)
    a = bench._dump_array(t, 24, 77)
    assert a.dtype == np.float32 and a.shape == (2, 3, 4)
    assert np.array_equal(a, np.arange(24, dtype=np.float32).reshape(2, 3, 4))


def test_dump_array_sample_is_fixed_and_leaves_the_global_rng():
    t = torch.arange(1000, dtype=torch.float32).reshape(10, 100)
    torch.manual_seed(5)
    want = torch.rand(3)
    torch.manual_seed(5)
    a = bench._dump_array(t, 64, 77)
    assert torch.equal(torch.rand(3), want)  # the dropout seeds come from the global generator
    b = bench._dump_array(t, 64, 77)
    assert a.dtype == np.float32 and a.shape == (64,)
    assert np.array_equal(a, b)
    assert np.all(np.diff(a) >= 0) and a.min() >= 0 and a.max() <= 999  # sorted positions of arange
    assert len(np.unique(a)) > 32
    assert not np.array_equal(a, bench._dump_array(t, 64, 78))


@pytest.mark.gpu
def test_plain_run_dumps_last_step(tmp_path, capsys, monkeypatch):
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    B, T = 2, 32
    d = tmp_path / "dump"
    bench.main(["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", str(B), "--seq", str(T),
                "--dump-outputs", str(d)])
    line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - B * T / (line["ms_per_step"] * 1e-3)) <= 1e-3 * line["value"]
    for leg in ("cpu_baseline", "parity", "feature_inclusive", "data_feed"):
        assert leg not in line
    assert line["roofline"]["traffic"] is None
    got = {f: np.load(d / f) for f in sorted(os.listdir(d))}
    assert sorted(got) == ["grad_norm.npy", "grads.npy", "loss.npy", "params.npy", "pred.npy"]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64e6
    assert got["pred.npy"].shape == (B, T, 61)
    assert got["loss.npy"].shape == (1,) and abs(got["loss.npy"][0] - line["final_loss"]) <= 1e-3
    assert got["grads.npy"].shape == got["params.npy"].shape == (bench.DUMP_ARENA_ELEMS,)
    # clipped at 2.0 from a norm the sampled gradients are part of
    assert got["grad_norm.npy"][0] > 0 and np.abs(got["grads.npy"]).max() > 0
    assert float(np.sqrt((got["grads.npy"].astype(np.float64) ** 2).sum())) <= got["grad_norm.npy"][0] * 1.5
    assert np.abs(got["pred.npy"]).max() > 0 and np.abs(got["params.npy"]).max() > 0

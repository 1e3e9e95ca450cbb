"""bench.py --dump-outputs DIR: what the last timed step computed, written as float32 .npy so that two builds can be compared output for
output.  CPU tier: the sampling rule (whole tensor when it fits, else seeded whole batch slices + seeded elements, under the budget).
GPU tier: a plain run at a small shape twice — same arrays both times, equal to the float64 oracle on the bench's own inputs, and the
plain line carries the headline only (the informational measurements are --full's)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_small_output_is_dumped_whole_in_float32(tmp_path):
    import bench
    out = torch.randn(2, 64, 16).to(torch.bfloat16)
    rec = bench.dump_outputs(str(tmp_path), out, 0, 1)
    got = np.load(tmp_path / "out.npy")
    assert rec["files"] == {"out": [2, 64, 16]} and got.dtype == np.float32
    assert np.array_equal(got, out.float().numpy())


def test_large_output_is_a_seeded_sample_under_the_budget(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1 << 20)
    out = torch.randn(16, 1024, 48)
    a = bench.dump_outputs(str(tmp_path / "a"), out, 0, 1)
    b = bench.dump_outputs(str(tmp_path / "b"), out, 0, 1)
    assert a["files"] == b["files"] and set(a["files"]) == {"out_batches", "out_elements"}
    total = 0
    for name in a["files"]:
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype == np.float32 and np.array_equal(x, y)
        total += x.nbytes
    assert total <= 1 << 20
    rng = np.random.default_rng(bench.DUMP_SEED)
    k = a["files"]["out_batches"][0]
    idx = np.sort(rng.choice(16, size=k, replace=False))
    assert np.array_equal(np.load(tmp_path / "a" / "out_batches.npy"), out[torch.from_numpy(idx)].numpy())
    m = a["files"]["out_elements"][0]
    eidx = np.sort(rng.integers(0, out.numel(), size=m, dtype=np.int64))
    assert np.array_equal(np.load(tmp_path / "a" / "out_elements.npy"), out.reshape(-1)[torch.from_numpy(eidx)].numpy())


def _bench(args, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0 and lines, p.stderr[-3000:]
    return json.loads(lines[-1])


@pytest.mark.gpu
def test_plain_run_dumps_its_last_step_reproducibly(tmp_path):
    from oracle.spectral_mix_oracle import assert_close, spectral_mix_numpy
    B, N, D, G = 4, 4096, 64, 4
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--prewarm", "4", "--shape", f"{B},{N},{D}", "--groups", str(G)]
    one = _bench(args + ["--dump-outputs", str(tmp_path / "a")])
    two = _bench(args + ["--dump-outputs", str(tmp_path / "b")])
    for line in (one, two):
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
        assert abs(line["ms_per_step"] - line["wall_s"] / 3 * 1e3) <= 1e-9 * line["ms_per_step"]
        assert not {"variants", "cpu_baseline", "cold_start"} & set(line), sorted(line)
        assert line["outputs_dumped"]["files"] == {"out": [B, N, D]}
    a, b = np.load(tmp_path / "a" / "out.npy"), np.load(tmp_path / "b" / "out.npy")
    assert a.dtype == np.float32 and np.array_equal(a, b)
    # the bench's inputs, drawn the same way on the same device
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    V = torch.randn(B, N, D, device=dev)
    gate = torch.randn(B, G, N // 2 + 1, dtype=torch.complex64, device=dev) * 0.3
    gate = gate * (torch.rand(B, G, N // 2 + 1, device=dev) >= 0.18)
    assert_close(a, spectral_mix_numpy(V.cpu().numpy(), gate.cpu().numpy(), None, N), what="bench dump")

"""`bench.py --dump-outputs DIR`: what the timed path computed in its last step, written as DIR/<name>.npy (float32 / float64,
at most 64 MB in all, a fixed seeded sample of anything larger), and the plain run's line (`--steps` timed steps, one window)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_writes_float_arrays_whole_when_they_fit(tmp_path):
    a = torch.arange(12, dtype=torch.float16).reshape(3, 4)
    b = torch.tensor([0.25], dtype=torch.float64)
    info = bench.dump_outputs(str(tmp_path), {"a": a, "b": b})
    ra, rb = np.load(tmp_path / "a.npy"), np.load(tmp_path / "b.npy")
    assert ra.dtype == np.float32 and ra.shape == (3, 4) and np.array_equal(ra, a.float().numpy())
    assert rb.dtype == np.float64 and rb.tolist() == [0.25]
    assert info["a"]["sampled"] is None and info["b"]["sampled"] is None


def test_dump_outputs_samples_large_arrays_under_the_limit_reproducibly(tmp_path):
    g = torch.Generator().manual_seed(3)
    big1, big2 = torch.randn(5000, generator=g), torch.randn(5000, generator=g)
    small = torch.randn(10, generator=g)
    limit = 10 * 4 + 2 * 1000 * 4
    info = bench.dump_outputs(str(tmp_path / "x"), {"p": big1, "g": big2, "s": small}, limit=limit)
    total = sum(os.path.getsize(tmp_path / "x" / f"{n}.npy") - 128 for n in ("p", "g", "s"))   # .npy header: 128 bytes
    assert total <= limit
    assert info["s"]["sampled"] is None and info["p"]["sampled"] == info["g"]["sampled"] == 1000
    p, q = np.load(tmp_path / "x" / "p.npy"), np.load(tmp_path / "x" / "g.npy")
    # the same sorted indices for arrays of one size: element i of both samples comes from the same position
    idx = torch.randperm(5000, generator=torch.Generator().manual_seed(0))[:1000].sort().values
    assert np.array_equal(p, big1[idx].numpy()) and np.array_equal(q, big2[idx].numpy())
    bench.dump_outputs(str(tmp_path / "y"), {"p": big1, "g": big2, "s": small}, limit=limit)
    for n in ("p", "g", "s"):
        assert np.array_equal(np.load(tmp_path / "x" / f"{n}.npy"), np.load(tmp_path / "y" / f"{n}.npy"))


def _bench(out, steps, warmup):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(out)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0, text[-3000:]
    lines = [l for l in text.splitlines() if l.startswith("{")]
    assert len(lines) == 1, text[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_steps_and_dumps_the_last_step(tmp_path):
    out = tmp_path / "dump"
    line = _bench(out, 2, 1)
    assert line["steps"] == 2 and line["timed_windows"]["n"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "images/s" and line["higher_is_better"] is True and line["dtype"] == "f16"
    assert line["full"] is False and line["roofline"] is None and line["cpu_baseline"] is None and line["ddim50"] is None
    names = {"pred", "loss", "params", "grads"}
    assert {f[:-4] for f in os.listdir(out)} == names
    total = 0
    for n in names:
        a = np.load(out / f"{n}.npy")
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(out / "pred.npy").shape == (4, 4, 64, 64)
    assert abs(float(np.load(out / "loss.npy")[0]) - line["loss"]) < 1e-4
    assert np.load(out / "params.npy").size == np.load(out / "grads.npy").size == 6047040
    # the dumped step starts from the state as set up: a run with a different trajectory before it computes the same outputs
    other = tmp_path / "dump_other"
    _bench(other, 4, 3)
    for n in names:
        a, b = np.load(out / f"{n}.npy").astype(np.float64), np.load(other / f"{n}.npy").astype(np.float64)
        scale = max(np.abs(b).max(), 1e-30)
        assert np.abs(a - b).max() <= 1e-5 * scale, (n, np.abs(a - b).max(), scale)

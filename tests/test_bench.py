"""bench.py's contract: a plain run measures only the timed steps, --full adds the rest, --dump-outputs writes the last timed step's
outputs as .npy files that two builds can compare element for element."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_sample_is_a_fixed_function_of_the_size():
    import bench
    big = torch.arange(3 * bench.DUMP_SAMPLE, dtype=torch.int32)
    a, b = bench._dump_array(big), bench._dump_array(big.clone())
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_SAMPLE,) and np.array_equal(a, b)
    assert np.all(np.diff(a) >= 0) and a[-1] < 3 * bench.DUMP_SAMPLE         # sorted indices, drawn from the whole tensor
    small = torch.linspace(0, 1, 1000, dtype=torch.float64).view(10, 100)
    s = bench._dump_array(small)
    assert s.dtype == np.float64 and np.array_equal(s, small.reshape(-1).numpy())


def test_bench_refuses_zero_steps_before_touching_the_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300,
                       cwd=ROOT)
    assert r.returncode == 2 and "--steps" in r.stderr, r.stderr[-2000:]


@pytest.mark.gpu
def test_plain_bench_run_times_only_its_steps_and_dumps_outputs(tmp_path):
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["step_ms"]["n"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "img/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["roofline"] is None and d["cpu_baseline"] is None and "schedule" not in d and "encoder_1x1" not in d
    files = {p.stem: np.load(p) for p in out.glob("*.npy")}
    assert {"logits", "params", "grads", "bn_buffers", "loss_per_class", "intersection", "union"} <= set(files)
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert files["logits"].shape == (3 * 256 * 384,) and np.isfinite(files["logits"]).all()
    assert abs(float(files["loss_per_class"].sum()) - d["final_loss_sum"]) <= 1e-6 * abs(d["final_loss_sum"])


@pytest.mark.gpu
def test_dumped_outputs_agree_between_runs_up_to_rounding(tmp_path):
    """Two runs with the same arguments: the dumped step starts from the seeded state, so what it computed agrees up to the
    order of the fp32 weight-gradient atomics (the forward, loss and metric counts are bit-reproducible)."""
    dumps = []
    for run in ("a", "b"):
        out = tmp_path / run
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                            "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        dumps.append({p.stem: np.load(p).astype(np.float64) for p in out.glob("*.npy")})
    a, b = dumps
    assert set(a) == set(b) and len(a) >= 9
    for name in a:
        x, y = a[name], b[name]
        fin = np.isfinite(y)
        assert np.array_equal(np.isfinite(x), fin), name
        d = float(np.abs(x[fin] - y[fin]).max()) if fin.any() else 0.0
        scale = float(np.abs(y[fin]).max()) if fin.any() else 0.0
        assert d <= 1e-5 * scale, (name, d, scale)
    for name in ("logits", "loss_per_class", "intersection", "union"):
        assert np.array_equal(a[name], b[name], equal_nan=True), name

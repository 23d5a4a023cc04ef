"""bench.py --gpus 1 as every change's measurement runs it: a plain run times its K steps and nothing else, `--dump-outputs DIR`
writes what those steps computed, and two runs with the same arguments write the same arrays.  `--full` still adds what a plain
run leaves out (here: the extra windows and the triad; the CPU baseline and the reference on the GPU are left out for time)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NY, NZ = 192, 160, 96


def bench(*extra, timeout=600):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--nx", str(NX), "--ny", str(NY), "--nz", str(NZ)]
    out = subprocess.run(cmd + [str(a) for a in extra], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, (out.stdout[-2000:], out.stderr[-3000:])
    return json.loads(lines[0])


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_a_plain_run_times_its_steps_and_dumps_what_they_computed(built_library, tmp_path, precision):
    steps, warmup = 12, 3
    r = bench("--steps", steps, "--warmup", warmup, "--precision", precision, "--dump-outputs", tmp_path / "a")
    assert r["steps"] == steps and r["warmup"] == warmup and r["dtype"] == precision and r["ms_per_step"] > 0
    assert r["unit"] == "Gnode-updates/s" and r["higher_is_better"] is True
    assert r["value"] == pytest.approx(NX * NY * NZ / (r["ms_per_step"] * 1e-3) / 1e9, rel=1e-2)
    # nothing but the timed steps: no extra windows, triad, side meshes, reference or CPU baseline
    assert "windows" not in r and r["roofline"]["triad_gbs"] is None and r["cpu_baseline"] is None and "reference_on_gpu" not in r
    assert "also_256cubed_gnode_per_s" not in r["config"] and "also_small_meshes" not in r["config"]
    a = tmp_path / "a"
    names = sorted(os.listdir(a))
    assert names == ["current.npy", "previous.npy", "receiver.npy"]
    assert sum(os.path.getsize(a / n) for n in names) <= 64 << 20
    rec = np.load(a / "receiver.npy")
    assert rec.shape == (steps, 1) and rec.dtype == np.float64 and np.all(np.isfinite(rec))
    dtype = np.float64 if precision == "f64" else np.float32
    for n in ("current", "previous"):
        f = np.load(a / (n + ".npy"))
        assert f.shape == (3 * NX * NY,) and f.dtype == dtype and np.all(np.isfinite(f))
        assert np.abs(f).max() > 0          # the planes through and next to the source, 15 steps after the impulse
    r2 = bench("--steps", steps, "--warmup", warmup, "--precision", precision, "--dump-outputs", tmp_path / "b")
    assert r2["steps"] == steps
    for n in names:
        assert np.load(a / n).tobytes() == np.load(tmp_path / "b" / n).tobytes(), n


def test_full_still_adds_what_a_plain_run_leaves_out(built_library):
    r = bench("--steps", 12, "--warmup", 3, "--full", "--no-cpu-baseline", "--no-reference-on-gpu")
    assert r["steps"] == 12 and r["ms_per_step"] > 0 and r["value"] > 0
    assert r["windows"]["steps_each"] >= 12 and len(r["windows"]["gnode_per_s"]) == 3
    assert r["roofline"]["triad_gbs"] > 0 and r["cpu_baseline"] is None

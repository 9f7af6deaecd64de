"""bench.py --dump-outputs: what the last timed step computed, written as float32 .npy files within 64 MB.
CPU: the writer's sampling and size bound.  GPU: one plain bench.py run (no --full), whose dumped losses are those of its last
timed step and whose line carries the headline figures and none of the measurements that --full adds."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_writes_small_arrays_whole_and_large_ones_as_the_same_seeded_sample(tmp_path):
    n = 3 * bench.DUMP_MAX_ELEMENTS + 7
    outputs = {"big": torch.arange(n, dtype=torch.float64).reshape(n, 1), "radii": torch.arange(10, dtype=torch.int32).reshape(2, 5)}
    info = bench.dump_outputs(outputs, str(tmp_path / "a"))
    bench.dump_outputs(outputs, str(tmp_path / "b"))
    big, radii = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "a" / "radii.npy")
    assert radii.dtype == np.float32 and radii.shape == (2, 5) and (radii == np.arange(10).reshape(2, 5)).all()
    assert big.dtype == np.float32 and big.ndim == 1 and 0.8 * bench.DUMP_MAX_ELEMENTS < big.size <= bench.DUMP_MAX_ELEMENTS
    assert (np.diff(big) > 0).all() and big[-1] < n                 # sorted unique elements of the array (here: their indices)
    np.testing.assert_array_equal(big, np.load(tmp_path / "b" / "big.npy"))
    assert info["big"]["shape"] == [n, 1] and info["radii"]["written"] == "all"
    with pytest.raises(SystemExit):
        bench.dump_outputs({str(i): torch.zeros(1) for i in range(17)}, str(tmp_path / "c"))


@pytest.mark.gpu
def test_bench_dumps_its_last_timed_step(tmp_path):
    out = tmp_path / "dump"
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--prewarm-s", "0", "--dump-outputs", str(out)],
                       cwd=ROOT, env=dict(os.environ, T4D_BENCH_DUMP_LOSSES="3"), capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-4000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["repeats"]["steps_per_region"] == 3
    # a plain run: the headline figures as ever, and nothing measured or checked beyond the timed steps
    assert line["metric"] == "rasterizer fwd+bwd views/sec" and line["unit"] == "views/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["value"] > 0 and abs(line["value"] * line["ms_per_step"] * 1e-3 - 24) < 0.01
    assert line["full"] is False
    for k in ("roofline", "cpu_baseline", "sequential", "strong", "view_sharded", "scenario_b", "single_view", "small_v", "forecast",
              "drop_in", "full_iteration", "c4", "dense_1m", "loss", "bake_8192"):
        assert line[k] is None, k
    # ... and at most 30 s of the run, start to exit, lie outside its warm-up and timed steps (writing the dump included here)
    outside = wall - (3 + 1) * line["ms_per_step"] * 1e-3
    print(f"plain run: {wall:.2f} s from start to exit, {outside:.2f} s outside its steps")
    assert outside <= 30.0, outside
    d = line["dump_outputs"]
    assert d["step"] == 2
    names = {"color", "radii", "depth", "alpha", "loss", "grad_means3D", "grad_means2D", "grad_opacities", "grad_colors_precomp",
             "grad_scales", "grad_rotations"}
    assert set(d["arrays"]) == names and {f[:-4] for f in os.listdir(out)} == names
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 << 20
    arrays = {n: np.load(out / (n + ".npy")) for n in names}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert d["arrays"]["color"]["shape"] == [24, 3, 512, 512] and arrays["loss"].shape == (24,)
    assert np.abs(arrays["color"]).max() > 0 and np.abs(arrays["grad_means3D"]).max() > 0
    # step 2 rendered again after the timed region (T4D_BENCH_DUMP_LOSSES): the same per-view losses, bit for bit
    np.testing.assert_array_equal(arrays["loss"], np.asarray(line["gathered_losses_first_steps"][2], np.float32))

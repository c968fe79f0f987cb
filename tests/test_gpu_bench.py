"""GPU: a plain `bench.py` run (no --full) launches the hot path exactly --steps times in its timed window, prints the lean line,
and --dump-outputs writes what the last timed step computed -- the values the oracle computes on the same seeded pairs, and the
same arrays on every run with the same workload."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, f32_hex

W = H = 8192
PAIRS = 2


def run_bench(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--workload", "8k-map",
           "--pairs", str(PAIRS), "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{") and '"metric"' in l]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["launches_timed"] == steps       # the library's own count of the timed launches
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["dtype"] == "f32" and line["higher_is_better"] is True
    for key in ("metric", "unit"):
        assert key in line
    for key in ("roofline", "valu", "sustained", "configs", "plan_regret", "cpu_baseline", "single_pair"):      # --full only
        assert key not in line, key
    return line


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path, oracle):
    import bench
    run_bench(tmp_path / "a", 3)
    run_bench(tmp_path / "b", 5)
    d = tmp_path / "a"
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 << 20
    for f in ("sums.npy", "ssim.npy", "map_sample.npy"):               # same workload, other step count: the same bits
        assert np.array_equal(np.load(d / f), np.load(tmp_path / "b" / f)), f

    sums, ssim, sample = np.load(d / "sums.npy"), np.load(d / "ssim.npy"), np.load(d / "map_sample.npy")
    assert sums.dtype == np.float64 and sums.shape == (PAIRS,) and ssim.dtype == np.float32 and ssim.shape == (PAIRS,)
    assert np.array_equal(ssim, (sums / float(W * H)).astype(np.float32))          # float(sum / double(W * H)) per pair
    assert sample.dtype == np.float32 and 0 < sample.size <= bench.MAP_SAMPLE_MAX
    # every pair against the oracle on the same seeded pair: the global float bit for bit (exact mode), and the map at the sampled positions
    threads = min(16, os.cpu_count() or 1)
    got = 0
    for i, sel in bench.map_sample_index(np, W * H, PAIRS):
        a, b = oracle.synth_pair(W, H, 0x5EED + i)
        v, _, m = oracle.ssim_f32(a, b, want_map=True, threads=threads)
        assert f32_hex(ssim[i]) == f32_hex(v), i
        assert np.array_equal(sample[got:got + sel.size].view(np.uint32), m.reshape(-1)[sel].view(np.uint32)), i
        got += sel.size
        del a, b, m
    assert got == sample.size
    assert f32_hex(ssim[0]) == "0x3f64b5b4"                                # the 8192^2 known answer (bench.WORKLOADS)

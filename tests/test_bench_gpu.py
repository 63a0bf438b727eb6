"""bench.py's plain run on an MI355X: exactly the timed steps and the result line, and --dump-outputs writing what the last
timed step computed (a seeded sample of y), checked against the 5-point stencil's closed form."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_bench_run_times_k_steps_and_dumps_its_outputs(cmi, tmp_path):
    import torch
    import bench
    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-1500:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["metric"] == "spmv_gflops_fp64_poisson5pt" and line["unit"] == "GFLOP/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["steps"] == 7 and line["warmup"] == 2 and line["value"] > 0 and line["ms_per_step"] > 0
    nnz = line["config"]["entries_per_gpu"]
    assert abs(line["value"] - 2.0 * nnz / (line["ms_per_step"] * 1e-3) / 1e9) <= 1e-3 * line["value"]
    # the timed kernel launches: 100 settle + W + K, nothing else in a plain run
    assert line["kernel_launch_ledger"] == [["settle", 100], ["warmup", 2], ["timed_steps", 7]]
    for k in ("roofline", "roofline_cold", "cg", "compressed_index_plan", "packed_tile_plan", "cpu_baseline", "cpu_baseline_omp"):
        assert k not in line, k
    # the outputs: f64, at most 64 MB, the same rows every run, y = A*x there bit for bit
    files = sorted(os.listdir(out_dir))
    assert files == ["y.npy", "y_rows.npy"], files
    assert sum(os.path.getsize(out_dir / f) for f in files) <= 64 << 20
    y, rows = np.load(out_dir / "y.npy"), np.load(out_dir / "y_rows.npy")
    assert y.dtype == np.float64 and rows.dtype == np.float64 and y.shape == rows.shape == (bench.DUMP_ROWS,)
    rows_i = rows.astype(np.int64)
    N = line["config"]["rows_per_gpu"]
    assert np.array_equal(rows_i, np.sort(np.random.default_rng(bench.DUMP_SEED).choice(N, size=bench.DUMP_ROWS, replace=False)))
    want = bench.stencil_expected(torch, cmi, bench.M, bench.M, 0, bench.M * bench.M, "cpu").numpy()
    assert np.array_equal(y, want[rows_i])

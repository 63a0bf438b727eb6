"""The sweep kernel of the maximal independent set (cmi_csr_ring_max_u64) against its byte model, the whole
cmi_csr_mis_aggregate call with its rounds, and -- in the same session -- what that call replaces: the host
standard_aggregate with both of its copies.

Matrix: the strength pattern (theta 0) of poisson5pt grid^2 for every --grids value (default 1000 and 3162).
    sweep            one cmi_csr_ring_max_u64 on random keys, two buffers swapped call by call.  Microseconds from HIP events:
                     ROUNDS rounds of BATCHES batches of LAUNCHES calls after warm-up, the median batch of each round, then the
                     median and the spread of the rounds; the rounds alternate with a device copy of the same 16 N bytes, the
                     yardstick of what this machine's memory gives to a kernel of this size.  The byte model is
                     4 nnz + 20 N (offsets, columns, the own key, the store; the 8 nnz gathered bytes are cache traffic),
                     quoted as GB/s and as a fraction of the 8 TB/s the data sheet gives.
    mis_aggregate    the whole call as host wall time (it synchronises), median of ROUNDS with [min, max]; rounds of MIS(2).
    aggregate_bench  tools/bin/aggregate_bench (make -C tools): mis_aggregate and standard_aggregate through the header layer,
                     timed in turn in one process; its output is passed through.

    python tools/mis_bench.py [--grids 1000,3162] [--json out.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS, BATCHES, LAUNCHES = 5, 5, 20
PEAK_GB_PER_S = 8000.0


def batch_us(torch, fn):
    times = []
    for _ in range(BATCHES):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(LAUNCHES):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / LAUNCHES)
    return float(np.median(times))


def interleaved(torch, fns):
    """name -> (median us over the rounds, min, max); every round times each variant once, in turn"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            t[k].append(batch_us(torch, fn))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in t.items()}


def run(cmi, torch, grid, out):
    A = cmi.poisson5pt(grid, grid, "csr", device="cuda")
    N = A.num_rows
    Sp, Sj, _ = cmi.csr_strength_symmetric(N, A.row_offsets, A.column_indices, A.values, 0.0)
    nnz = Sj.numel()
    gen = torch.Generator(device="cuda").manual_seed(7)
    keys = [torch.randint(0, 2**62, (N,), dtype=torch.int64, device="cuda", generator=gen), torch.empty(N, dtype=torch.int64, device="cuda")]
    turn = [0]

    def sweep():
        cmi.csr_ring_max(N, Sp, Sj, keys[turn[0]], keys[1 - turn[0]])
        turn[0] = 1 - turn[0]

    def copy():
        keys[1 - turn[0]].copy_(keys[turn[0]])

    # a check before the clock: the sweep of the pattern's own keys is the five-point maximum
    z = cmi.csr_ring_max(N, Sp, Sj, keys[0])
    k2 = keys[0].view(grid, grid)
    want = k2.clone()
    want[1:] = torch.maximum(want[1:], k2[:-1])
    want[:-1] = torch.maximum(want[:-1], k2[1:])
    want[:, 1:] = torch.maximum(want[:, 1:], k2[:, :-1])
    want[:, :-1] = torch.maximum(want[:, :-1], k2[:, 1:])
    assert torch.equal(z.view(grid, grid), want), "*** the sweep differs from the five-point maximum"
    del z, want

    t = interleaved(torch, {"sweep": sweep, "copy": copy})
    model = 4 * nnz + 20 * N
    us, lo, hi = t["sweep"]
    cu, clo, chi = t["copy"]
    row = {"grid": grid, "rows": N, "nnz": nnz, "sweep_us": round(us, 2), "sweep_min_max": [round(lo, 2), round(hi, 2)], "model_bytes": model,
           "model_GB_per_s": round(model / us / 1e3, 1), "fraction_of_8TBps": round(model / us / 1e3 / PEAK_GB_PER_S, 3),
           "copy_us": round(cu, 2), "copy_GB_per_s": round(16 * N / cu / 1e3, 1)}
    print(f"  poisson5pt {grid}^2 strength pattern: {N} rows, {nnz} entries")
    print(f"    sweep          {us:10.1f} us [{lo:.1f}, {hi:.1f}]  model {model / 1e6:.1f} MB -> {row['model_GB_per_s']:.0f} GB/s = {row['fraction_of_8TBps']:.3f} of 8 TB/s")
    print(f"    copy of 16 N   {cu:10.1f} us [{clo:.1f}, {chi:.1f}]  {row['copy_GB_per_s']:.0f} GB/s", flush=True)
    _, set_size, rounds = cmi.maximal_independent_set((N, Sp, Sj), k=2)
    cmi.mis_aggregate((N, Sp, Sj))
    wall = []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, count = cmi.mis_aggregate((N, Sp, Sj))
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    row.update({"mis_aggregate_ms": round(float(np.median(wall)), 3), "mis_aggregate_min_max": [round(min(wall), 3), round(max(wall), 3)], "mis_rounds": rounds,
                "mis_set_size": set_size, "aggregates": count})
    print(f"    mis_aggregate  {row['mis_aggregate_ms']:10.3f} ms [{min(wall):.3f}, {max(wall):.3f}]  MIS(2): {set_size} nodes in {rounds} rounds "
          f"({2 * rounds + 2} sweeps), {count} aggregates", flush=True)
    out.append(row)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grids", default="1000,3162")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import cusp_autotuned_amd as cmi
    print(f"mis_bench: {ROUNDS} interleaved rounds x {BATCHES} batches x {LAUNCHES} calls; us = median of the rounds [min, max]")
    rows = []
    for g in args.grids.split(","):
        run(cmi, torch, int(g), rows)
    exe = os.path.join(ROOT, "tools", "bin", "aggregate_bench")
    if not os.path.exists(exe):
        raise SystemExit(f"{exe} is missing: make -C tools")
    sys.stdout.flush()
    r = subprocess.run(["timeout", "-k", "10", "300", exe, f"--grids={args.grids}", f"--rounds={ROUNDS}"], capture_output=True, text=True)
    print(r.stdout, end="")
    if r.returncode != 0:
        raise SystemExit(f"aggregate_bench failed ({r.returncode}): {r.stderr[-2000:]}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    print(json.dumps({"mis_cases": len(rows), "sweep_fraction_of_8TBps": {str(r["grid"]): r["fraction_of_8TBps"] for r in rows}}))


if __name__ == "__main__":
    main()

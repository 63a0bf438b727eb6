"""The semiring CSR kernel (cmi_spmv_csr_semiring_*) against the multiplies it stands beside, and against its own byte models.

Matrices: poisson5pt grid^2 for every --grids value (default 3162 and 1000), float64 and float32.  Per matrix the cases are timed in
turn (ROUNDS rounds, each round one batch median per case), microseconds from HIP events, reported as median [min, max] of the rounds:
    (a) multiplies, plus     the new kernel | the plan-less cmi_spmv_csr_* of the same build | the planned multiply (cmi.multiply)
    (b) plus, minimum        the new kernel (min-plus: the same streams as (a))
    (c) project2nd, maximum  the new kernel with NULL values | cmi_csr_ring_max_u64 on the same pattern (64-bit keys)
    (d) project1st, maximum  the new kernel (no column indices, no x)
Byte models (what must come from memory once; gathered x beyond its first read is cache traffic), I = 4, T = the value size:
    (a), (b)   nnz (I + T) + rows (I + T) + cols T          offsets, columns, values, the y store, x
    (c)        nnz I + rows (I + T) + cols T                no values          (ring_max: 4 nnz + 20 rows)
    (d)        nnz T + rows (I + T)                         no columns, no x
quoted as GB/s and as a fraction of the 8 TB/s of the data sheet.  Every case is checked against a torch expression before the clock.
Nothing here is a gate.

    python tools/semiring_bench.py [--grids 3162,1000]
"""
import argparse
import json
import os
import sys

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
    """name -> (median us over the rounds, min, max); every round times each case once, in turn"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            t[k].append(batch_us(torch, fn))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in t.items()}


def five_point(torch, v, grid, pick):
    """pick (maximum / minimum) over the five-point neighbourhood of a grid^2 vector (what the pattern's rows gather)"""
    g = v.view(grid, grid)
    out = g.clone()
    out[1:] = pick(out[1:], g[:-1])
    out[:-1] = pick(out[:-1], g[1:])
    out[:, 1:] = pick(out[:, 1:], g[:, :-1])
    out[:, :-1] = pick(out[:, :-1], g[:, 1:])
    return out.reshape(-1)


def run(cmi, torch, grid, dtype, out):
    A = cmi.poisson5pt(grid, grid, "csr", device="cuda", dtype=dtype)
    N, nnz = A.num_rows, A.num_entries
    Ap, Aj, Ax = A.row_offsets, A.column_indices, A.values
    T = Ax.element_size()
    gen = torch.Generator(device="cuda").manual_seed(11)
    x = torch.rand(N, dtype=dtype, device="cuda", generator=gen) + 0.5
    y = [torch.empty(N, dtype=dtype, device="cuda") for _ in range(3)]
    keys = torch.randint(0, 2**62, (N,), dtype=torch.int64, device="cuda", generator=gen)
    z = torch.empty_like(keys)

    def semiring(combine, reduce, init, values=Ax, columns=Aj, vector=x):
        return lambda: cmi.spmv_csr_semiring(N, N, Ap, columns, values, vector, y[0], combine, reduce, None, init, num_entries=nnz)

    cases = {"a semiring": semiring("multiplies", "plus", 0.0),
             "a planless": lambda: cmi.spmv_csr(N, N, Ap, Aj, Ax, x, y[1]),
             "a planned": lambda: cmi.multiply(A, x, y[2]),
             "b plus-min": semiring("plus", "minimum", float("inf")),
             "c p2nd-max": semiring("project2nd", "maximum", float("-inf"), values=None),
             "c ring_max": lambda: cmi.csr_ring_max(N, Ap, Aj, keys, z),
             "d p1st-max": semiring("project1st", "maximum", float("-inf"), columns=None, vector=None)}
    # checks before the clock
    for k in ("a semiring", "a planless", "a planned"):
        cases[k]()
    torch.cuda.synchronize()
    assert torch.equal(y[0], y[1]), "*** (multiplies, plus) differs from the plan-less cmi_spmv_csr_* (both sum in storage order)"
    # a plan may re-associate a row's sum: held to rounding only, 8 eps x the row's sum of |a x| (at most 8 x 1.5 here)
    assert float((y[0] - y[2]).abs().max()) <= 8 * torch.finfo(dtype).eps * 12.0, "*** the planned multiply differs beyond rounding"
    cases["c p2nd-max"]()
    assert torch.equal(y[0], five_point(torch, x, grid, torch.maximum)), "*** (project2nd, maximum) differs from the five-point maximum"
    cases["d p1st-max"]()
    assert torch.equal(y[0], torch.full_like(x, 4.0)), "*** (project1st, maximum) is not the diagonal"
    cases["b plus-min"]()
    assert bool((y[0] <= five_point(torch, x, grid, torch.minimum) + 4.0).all()) and bool((y[0] >= x.min() - 1.0).all()), "*** (plus, minimum) out of range"

    t = interleaved(torch, cases)
    full, no_values, no_columns = nnz * (4 + T) + N * (4 + T) + N * T, nnz * 4 + N * (4 + T) + N * T, nnz * T + N * (4 + T)
    model = {"a semiring": full, "a planless": full, "a planned": full, "b plus-min": full, "c p2nd-max": no_values, "c ring_max": 4 * nnz + 20 * N,
             "d p1st-max": no_columns}
    tag = "f64" if T == 8 else "f32"
    print(f"  poisson5pt {grid}^2 {tag}: {N} rows, {nnz} entries")
    row = {"grid": grid, "dtype": tag, "rows": N, "nnz": nnz}
    for k, (us, lo, hi) in t.items():
        gbs = model[k] / us / 1e3
        print(f"    {k:12s} {us:9.1f} us [{lo:.1f}, {hi:.1f}]   model {model[k] / 1e6:7.1f} MB -> {gbs:6.0f} GB/s = {gbs / PEAK_GB_PER_S:.3f} of 8 TB/s", flush=True)
        row[k] = {"us": round(us, 2), "min_max": [round(lo, 2), round(hi, 2)], "model_bytes": model[k], "fraction_of_8TBps": round(gbs / PEAK_GB_PER_S, 3)}
    sus, slo, shi = t["a semiring"]
    pus, plo, phi = t["a planless"]
    spread = max(shi - slo, phi - plo)
    row["a_semiring_minus_planless_us"] = round(sus - pus, 2)
    row["a_within_twice_the_spread"] = bool(abs(sus - pus) <= 2 * spread)
    print(f"    (a) semiring - planless = {sus - pus:+.1f} us; twice the run's spread = {2 * spread:.1f} us -> {'within' if row['a_within_twice_the_spread'] else 'BEYOND'}", flush=True)
    out.append(row)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grids", default="3162,1000")
    args = ap.parse_args()
    import torch
    import cusp_autotuned_amd as cmi
    print(f"semiring_bench: {ROUNDS} interleaved rounds x {BATCHES} batches x {LAUNCHES} calls; us = median of the rounds [min, max]")
    rows = []
    for g in args.grids.split(","):
        for dtype in (torch.float64, torch.float32):
            run(cmi, torch, int(g), dtype, rows)
    print(json.dumps({"semiring_cases": len(rows), "a_semiring_minus_planless_us": {f"{r['grid']} {r['dtype']}": r["a_semiring_minus_planless_us"] for r in rows}}))


if __name__ == "__main__":
    main()

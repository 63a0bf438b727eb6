"""The fused CSR sweeps (cmi_spmv_csr_axpby_*, cmi_csr_jacobi_sweep_*) against the same steps made of the calls that were
there before them: the planned multiply (cmi_spmv_csr_plan_*) followed by cmi_blas_axpby_* or by the elementwise Jacobi
update, timed interleaved (A, B, A, B, ...) in one process.

Matrix: poisson5pt grid^2 (default 3162: BASELINE.json configs[1]) in f64 and f32.  Steps:
    residual         r <- b - A x          fused: 1 launch           unfused: multiply + axpby(b, y, r, 1, -1)
    polynomial step  h' <- A h + c r       fused: 1 launch           unfused: multiply + axpby(y, r, h', 1, c)
    jacobi sweep     x <- x + w (b - A x) / d
                                           fused: 1 launch + copy    unfused: multiply + elementwise update in place
                     ... and the fused launch alone ("ping-pong": what a caller that owns both buffers pays)
Per step: microseconds (HIP events, ROUNDS interleaved rounds of BATCHES batches of LAUNCHES launches after warm-up; the
median batch of each round, then the median and the spread of the rounds), the ratio fused / unfused, and the byte model
of the vectors (per row, beyond the multiply's own reads of the matrix: 32 -> 16, 32 -> 16, 48 -> 40 (24 without the
copy) for f64).  Every timed pair is checked bit for bit before it is printed.

    python tools/relax_bench.py [--grid 3162] [--dtypes f64,f32] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS, BATCHES, LAUNCHES = 5, 5, 20
TIMED_OMEGA = 1e-3   # omega of the timed Jacobi sweeps (the bit check uses 2/3)


def batch_us(torch, fn):
    """median batch time per call (us) of BATCHES x LAUNCHES event-timed calls"""
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


def same(torch, a, b):
    return bool(torch.equal(a.view(torch.int64 if a.dtype == torch.float64 else torch.int32),
                            b.view(torch.int64 if b.dtype == torch.float64 else torch.int32)))


def run(cmi, torch, grid, dtype, out):
    tag = "f64" if dtype == torch.float64 else "f32"
    s = 8 if dtype == torch.float64 else 4
    A = cmi.poisson5pt(grid, grid, "csr", device="cuda")
    N, nnz = A.num_rows, A.num_entries
    Ap, Aj, Ax = A.row_offsets, A.column_indices, A.values.to(dtype)
    plan = cmi.Plan.csr(dtype, N, N, Ap, Aj)
    gen = torch.Generator(device="cuda").manual_seed(7)
    x, b, r = (torch.randn(N, dtype=dtype, device="cuda", generator=gen) for _ in range(3))
    diag = torch.full((N,), 4.0, dtype=dtype, device="cuda")
    y, o1, o2 = (torch.empty(N, dtype=dtype, device="cuda") for _ in range(3))
    c, w = 0.7, 2.0 / 3.0
    matrix_bytes = (4 + s) * nnz + 4 * (N + 1) + s * N   # the multiply's own reads: indices, values, offsets, x once

    def report(step, res, fused, unfused, vec_fused, vec_unfused):
        tf, tu = res[fused], res[unfused]
        row = {"step": step, "dtype": tag, "rows": N, "nnz": nnz, "fused": fused, "unfused": unfused, "fused_us": round(tf[0], 2),
               "fused_min_max": [round(tf[1], 2), round(tf[2], 2)], "unfused_us": round(tu[0], 2), "unfused_min_max": [round(tu[1], 2), round(tu[2], 2)],
               "ratio": round(tf[0] / tu[0], 3), "byte_model_ratio": round((matrix_bytes + vec_fused * N) / (matrix_bytes + vec_unfused * N), 3)}
        out.append(row)
        print(f"{step:>24} {tag}: fused {tf[0]:8.1f} us [{tf[1]:.1f}, {tf[2]:.1f}]  unfused {tu[0]:8.1f} us [{tu[1]:.1f}, {tu[2]:.1f}]"
              f"  ratio {row['ratio']:.3f}  (byte model {row['byte_model_ratio']:.3f}: vectors {vec_fused} vs {vec_unfused} B/row)", flush=True)

    # ---- residual
    def res_fused():
        cmi.spmv_csr_axpby(N, N, Ap, Aj, Ax, x, -1.0, 1.0, b, o1, plan=plan)

    def res_unfused():
        cmi.spmv_csr_plan(plan, Ap, Aj, Ax, x, y)
        cmi.blas_axpby(1.0, b, -1.0, y, o2)

    t = interleaved(torch, {"axpby sweep": res_fused, "multiply + axpby": res_unfused})
    assert same(torch, o1, o2), "*** RESULT MISMATCH *** residual"
    report("residual", t, "axpby sweep", "multiply + axpby", 2 * s, 4 * s)

    # ---- one polynomial degree step
    def step_fused():
        cmi.spmv_csr_axpby(N, N, Ap, Aj, Ax, x, 1.0, c, r, o1, plan=plan)

    def step_unfused():
        cmi.spmv_csr_plan(plan, Ap, Aj, Ax, x, y)
        cmi.blas_axpby(1.0, y, c, r, o2)

    t = interleaved(torch, {"axpby sweep": step_fused, "multiply + axpby": step_unfused})
    assert same(torch, o1, o2), "*** RESULT MISMATCH *** polynomial step"
    report("polynomial step", t, "axpby sweep", "multiply + axpby", 2 * s, 4 * s)

    # ---- one Jacobi sweep.  The bit check runs once with omega = 2/3 on a fresh pair; the timed sweeps update x in place hundreds
    # of times, so they run with TIMED_OMEGA (a damped sweep stays finite; the work per sweep is the same)
    xa, xb, xc = x.clone(), x.clone(), x.clone()

    def jac_fused(omega=TIMED_OMEGA):
        cmi.csr_jacobi_sweep(N, Ap, Aj, Ax, diag, b, xa, omega, o1, plan=plan)
        cmi.blas_copy(o1, xa)

    def jac_unfused(omega=TIMED_OMEGA):
        cmi.spmv_csr_plan(plan, Ap, Aj, Ax, xb, y)
        cmi.relax_jacobi_update(diag, b, y, omega, xb)

    def jac_pingpong(omega=TIMED_OMEGA):
        cmi.csr_jacobi_sweep(N, Ap, Aj, Ax, diag, b, xc, omega, o2, plan=plan)

    jac_fused(w)
    jac_unfused(w)
    assert same(torch, xa, xb), "*** RESULT MISMATCH *** jacobi sweep"
    xa.copy_(x)
    xb.copy_(x)
    t = interleaved(torch, {"sweep + copy": jac_fused, "multiply + update": jac_unfused, "sweep alone": jac_pingpong})
    report("jacobi sweep", t, "sweep + copy", "multiply + update", 5 * s, 6 * s)
    report("jacobi sweep, ping-pong", t, "sweep alone", "multiply + update", 3 * s, 6 * s)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, default=3162)
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import cusp_autotuned_amd as cmi
    print(f"relax_bench: poisson5pt {args.grid}^2, {ROUNDS} interleaved rounds x {BATCHES} batches x {LAUNCHES} launches; us = median of the rounds [min, max]; Jacobi sweeps timed with omega = {TIMED_OMEGA}, checked bit for bit with omega = 2/3")
    rows = []
    for dt in args.dtypes.split(","):
        run(cmi, torch, args.grid, torch.float64 if dt == "f64" else torch.float32, rows)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    print(json.dumps({"relax_cases": len(rows), "ratios": {f"{r['step']} {r['dtype']}": r["ratio"] for r in rows}}))


if __name__ == "__main__":
    main()

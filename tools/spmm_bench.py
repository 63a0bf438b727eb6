"""CSR x dense block (SpMM, cmi_spmm_csr_*) against the loop it replaces: k planned SpMVs (cmi_spmv_csr_plan_*, one per
column), timed interleaved in the same process.

Cases: poisson5pt 3162^2 (BASELINE.json configs[1]) in f64 and f32, row-major contiguous X and Y, k in {1, 2, 4, 8, 16, 32};
the ldoor-like stand-in of tools/suitesparse_like.py at k = 8 (f64).  Per case: microseconds (HIP events, 10 batches of
>= 20 launches after warm-up -- the bench.py protocol; median batch), GFLOP/s = 2 nnz k / t, and the fraction of 8 TB/s
on the compulsory bytes B(k) = 4 (N + 1) + (4 + s) nnz + s k (num_cols + N) (+ s k N when accumulating).  Every timed
result is checked bit for bit against the column-by-column SpMV before it is printed.

    python tools/spmm_bench.py [--grid 3162] [--ks 1,2,4,8,16,32] [--no-ldoor] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PEAK = 8.0e12
BATCHES, LAUNCHES = 10, 20


def timed(torch, fn):
    """median batch time per launch (us): 3 warm-up calls, then BATCHES x LAUNCHES event-timed launches"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
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


def case(cmi, torch, name, A, k, dtype, rows_out):
    N, cols, nnz = A.num_rows, A.num_cols, A.num_entries
    s = 8 if dtype == torch.float64 else 4
    Ax = A.values.to(dtype)
    gen = torch.Generator(device="cuda").manual_seed(k)
    X = torch.randn((cols, k), dtype=dtype, device="cuda", generator=gen)
    Y = torch.empty((N, k), dtype=dtype, device="cuda")
    Xc = [X[:, c].contiguous() for c in range(k)]
    Yc = [torch.empty(N, dtype=dtype, device="cuda") for _ in range(k)]
    plan = cmi.Plan.csr(dtype, N, cols, A.row_offsets, A.column_indices)

    def spmm():
        cmi.spmm_csr(N, cols, A.row_offsets, A.column_indices, Ax, X, Y)

    def spmvs():
        for c in range(k):
            cmi.spmv_csr_plan(plan, A.row_offsets, A.column_indices, Ax, Xc[c], Yc[c])

    t_mm, t_mv = [], []
    for _ in range(3):  # interleaved: SpMM, then the k SpMVs, three rounds
        t_mm.append(timed(torch, spmm))
        t_mv.append(timed(torch, spmvs))
    torch.cuda.synchronize()
    exact = bool(torch.equal(Y, torch.stack(Yc, dim=1)))
    if not exact:
        raise SystemExit(f"*** RESULT MISMATCH *** {name} k={k} {dtype}: SpMM differs from the column-by-column SpMV")
    us, us_mv = float(np.median(t_mm)), float(np.median(t_mv))
    B = 4 * (N + 1) + (4 + s) * nnz + s * k * (cols + N)
    r = {"matrix": name, "dtype": "f64" if s == 8 else "f32", "k": k, "rows": N, "nnz": nnz, "us": round(us, 2),
         "gflops": round(2 * nnz * k / (us * 1e-6) / 1e9, 1), "bytes_model": B, "frac_8TBs": round(B / (us * 1e-6) / PEAK, 3),
         "spmv_loop_us": round(us_mv, 2), "speedup_vs_spmv_loop": round(us_mv / us, 2), "bit_exact": exact}
    rows_out.append(r)
    print(f"{name:>14} {r['dtype']} k={k:>2}: {us:9.1f} us  {r['gflops']:7.1f} GFLOP/s  {r['frac_8TBs']:.3f} of 8 TB/s (B={B / 1e9:.3f} GB)"
          f" | {k} planned SpMVs {us_mv:9.1f} us -> {r['speedup_vs_spmv_loop']:.2f}x  [bit-exact]", flush=True)


def main():
    global BATCHES
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, default=3162)
    ap.add_argument("--ks", default="1,2,4,8,16,32")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--no-ldoor", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--batches", type=int, default=BATCHES, help="timed batches per measurement (fewer for counter runs)")
    args = ap.parse_args()
    BATCHES = args.batches
    import torch
    import cusp_autotuned_amd as cmi
    rows = []
    A = cmi.poisson5pt(args.grid, args.grid, "csr", device="cuda")
    for dt in args.dtypes.split(","):
        dtype = torch.float64 if dt == "f64" else torch.float32
        for k in (int(v) for v in args.ks.split(",")):
            case(cmi, torch, f"poisson{args.grid}", A, k, dtype, rows)
    if not args.no_ldoor:
        import suitesparse_like
        Ap, Aj, Ax, _ = suitesparse_like.load("ldoor")
        L = cmi.CsrMatrix(len(Ap) - 1, len(Ap) - 1, len(Aj), torch.from_numpy(Ap).cuda(), torch.from_numpy(Aj).cuda(),
                          torch.from_numpy(Ax).cuda())
        case(cmi, torch, "ldoor_like", L, 8, torch.float64, rows)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    print(json.dumps({"spmm_cases": len(rows), "all_bit_exact": all(r["bit_exact"] for r in rows)}))


if __name__ == "__main__":
    main()

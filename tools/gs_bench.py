"""The colour sweeps of cusp::relaxation::gauss_seidel / sor (cmi_csr_gauss_seidel_colour_*, one call per colour) next to the
cusp::relaxation::jacobi step of the same build (planned multiply + cmi_relax_jacobi_update_*), the yardstick, timed
interleaved (A, B, A, B, ...) in one process.

Matrix: poisson5pt grid^2 (default 3162: BASELINE.json configs[1]) in f64 and f32; its greedy colouring is red-black, two
colours that interleave row by row, none of them with rows that depend on one another (so every call is the one-launch form).
    forward      colours 0, 1                                  2 launches
    symmetric    colours 0, 1, 1, 0                            4 launches
    sor step     copy, symmetric sweep, axpby                  6 launches
    jacobi step  multiply, elementwise update                  2 launches
Per step: microseconds (HIP events, ROUNDS interleaved rounds of BATCHES batches of LAUNCHES calls after warm-up; the median
batch of each round, then the median and the spread of the rounds), the ratio to the Jacobi step, and a byte model: the
matrix streams (Aj, Ax) are counted ONCE per colour pass that touches them -- the two colours interleave row by row, so each
pass touches nearly every cache line of both, and a forward sweep may move close to twice the multiply's matrix bytes.

    python tools/gs_bench.py [--grid 3162] [--dtypes f64,f32] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS, BATCHES, LAUNCHES = 5, 5, 10
TIMED_OMEGA = 1e-3   # omega of the timed Jacobi steps (a damped step stays finite over hundreds of in-place repeats)


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


def run(cmi, torch, grid, dtype, out):
    tag = "f64" if dtype == torch.float64 else "f32"
    s = 8 if dtype == torch.float64 else 4
    A = cmi.poisson5pt(grid, grid, "csr", device="cuda")
    N, nnz = A.num_rows, A.num_entries
    Ap, Aj, Ax = A.row_offsets, A.column_indices, A.values.to(dtype)
    plan = cmi.Plan.csr(dtype, N, N, Ap, Aj)
    # the greedy colouring of the 5-point stencil: (ix + iy) % 2, rows ascending inside a colour
    r = np.arange(N)
    colour = ((r % grid) + (r // grid)) % 2
    ordering = torch.from_numpy(np.argsort(colour, kind="stable").astype(np.int32)).cuda()
    offsets = [0, int((colour == 0).sum()), N]
    gen = torch.Generator(device="cuda").manual_seed(7)
    x0, b = (torch.randn(N, dtype=dtype, device="cuda", generator=gen) for _ in range(2))
    diag = torch.full((N,), 4.0, dtype=dtype, device="cuda")
    xg, xs, xo, xj = x0.clone(), x0.clone(), x0.clone(), x0.clone()
    y, temp = torch.empty_like(x0), torch.empty_like(x0)

    def colours(x, order):
        for c in order:
            cmi.csr_gauss_seidel_colour(N, Ap, Aj, Ax, b, x, ordering, offsets[c], offsets[c + 1])

    def forward():
        colours(xg, (0, 1))

    def symmetric():
        colours(xs, (0, 1, 1, 0))

    def sor_step(omega=1.5):
        cmi.blas_copy(xo, temp)
        colours(xo, (0, 1, 1, 0))
        cmi.blas_axpby(1.0 - omega, temp, omega, xo, xo)

    def jacobi_step():
        cmi.spmv_csr_plan(plan, Ap, Aj, Ax, xj, y)
        cmi.relax_jacobi_update(diag, b, y, TIMED_OMEGA, xj)

    # a check before the clock: one forward sweep lowers the residual of this diagonally dominant system
    def residual(x):
        cmi.spmv_csr_plan(plan, Ap, Aj, Ax, x, y)
        return float((b - y).norm())

    before = residual(xg)
    forward()
    after = residual(xg)
    assert after < before, f"*** a forward sweep did not lower the residual: {before} -> {after}"

    t = interleaved(torch, {"forward": forward, "symmetric": symmetric, "sor step": sor_step, "jacobi step": jacobi_step})
    assert all(bool(torch.isfinite(v).all()) for v in (xg, xs, xo, xj)), "*** a timed vector left the finite range"
    stream = (4 + s) * nnz                       # Aj and Ax once
    per_colour_pass = 4 * N + 4 * N // 2 + 3 * s * N // 2   # Ap gathered (two ints per row: ~all of it per pass), ordering, b, x read + write, per half
    model = {"forward": 2 * stream + 2 * per_colour_pass + s * N, "symmetric": 4 * stream + 4 * per_colour_pass + 2 * s * N,
             "sor step": 4 * stream + 4 * per_colour_pass + 2 * s * N + 5 * s * N,
             "jacobi step": stream + 4 * (N + 1) + 2 * s * N + 5 * s * N}
    tj = t["jacobi step"]
    for step in ("forward", "symmetric", "sor step", "jacobi step"):
        v = t[step]
        row = {"step": step, "dtype": tag, "rows": N, "nnz": nnz, "us": round(v[0], 2), "min_max": [round(v[1], 2), round(v[2], 2)],
               "ratio_to_jacobi": round(v[0] / tj[0], 3), "byte_model_ratio": round(model[step] / model["jacobi step"], 3),
               "model_GB_per_s": round(model[step] / v[0] / 1e3, 1)}
        out.append(row)
        print(f"{step:>12} {tag}: {v[0]:9.1f} us [{v[1]:.1f}, {v[2]:.1f}]  / jacobi step {row['ratio_to_jacobi']:.3f}"
              f"  (byte model {row['byte_model_ratio']:.3f}; {row['model_GB_per_s']:.0f} GB/s of the model's bytes)", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, default=3162)
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import cusp_autotuned_amd as cmi
    print(f"gs_bench: poisson5pt {args.grid}^2, {ROUNDS} interleaved rounds x {BATCHES} batches x {LAUNCHES} calls; us = median of the rounds "
          f"[min, max]; Jacobi steps timed with omega = {TIMED_OMEGA}, SOR with omega = 1.5")
    rows = []
    for dt in args.dtypes.split(","):
        run(cmi, torch, args.grid, torch.float64 if dt == "f64" else torch.float32, rows)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    print(json.dumps({"gs_cases": len(rows), "ratios_to_jacobi": {f"{r['step']} {r['dtype']}": r["ratio_to_jacobi"] for r in rows}}))


if __name__ == "__main__":
    main()

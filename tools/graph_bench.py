"""cusp::graph on the device against the header layer's host loops, and what a bandwidth-reducing ordering buys the planned
multiply.  Every figure is the median of ROUNDS interleaved rounds with [min, max]; the search calls
synchronise, so they are timed on the host clock.

    bfs deep      poisson5pt grid^2 (default 3162: 6323 levels from vertex 0, the launch-bound end), levels and predecessors, ms and
                  us per level -- through the library (K = cmi_bfs_levels_per_read() levels per host read) and through the copies
                  of the library that tools/Makefile builds with other K (tools/bin/libcusp_mi355x_bfs<K>.so), in turn
    bfs shallow   a random symmetric pattern of --shallow vertices (default 10^7), about 8 entries per row: ms and edges per second
    host          tools/bin/graph_bench_host on the same arrays (one core)
    ordering      symmetric_rcm and symmetric_permute (two gathers and the COO sort, as the header layer does on device_memory) on
                  poisson5pt grid^2 shuffled by a seeded random permutation, for every --grids value, against the host path
    multiply      the planned f64 cmi_spmv on the natural, shuffled and reordered copies, with the bandwidth of each

    make -C tools all bfs_variants && python tools/graph_bench.py [--grids 1000,3162] [--shallow 10000000] [--skip-host]
"""
import argparse
import ctypes
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS = 5


def wall_ms(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def interleaved(torch, fns, rounds=ROUNDS):
    """name -> (median ms, min, max); every round times each variant once, in turn"""
    for fn in fns.values():
        fn()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(wall_ms(torch, fn))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in t.items()}


def show(name, stat, extra=""):
    print(f"    {name:<44s} {stat[0]:10.3f} ms [{stat[1]:.3f}, {stat[2]:.3f}]  {extra}", flush=True)


def raw_search(L, cmi, torch, n, Ap, Aj, src, mark, labels):
    reached, depth = ctypes.c_int64(0), ctypes.c_int(0)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = L.cmi_csr_breadth_first_search(n, Aj.numel(), vp(Ap), vp(Aj), src, int(mark), vp(labels), ctypes.byref(reached), ctypes.byref(depth),
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0, st
    return reached.value, depth.value


def variant_libraries(cmi):
    """K -> a loaded copy of the library built with that many levels per host read (the library itself under its own K)"""
    out = {cmi.bfs_levels_per_read(): cmi.lib()}
    for path in sorted(glob.glob(os.path.join(ROOT, "tools", "bin", "libcusp_mi355x_bfs*.so"))):
        k = int(re.search(r"bfs(\d+)\.so$", path).group(1))
        if k not in out:
            L = ctypes.CDLL(path)
            i64, vp = ctypes.c_int64, ctypes.c_void_p
            L.cmi_csr_breadth_first_search.argtypes = [i64, i64, vp, vp, i64, ctypes.c_int, vp, ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_int), vp]
            assert L.cmi_bfs_levels_per_read() == k
            out[k] = L
    return dict(sorted(out.items()))


def host_bench(n, Ap, Aj, src, what, skip):
    exe = os.path.join(ROOT, "tools", "bin", "graph_bench_host")
    if skip:
        return
    if not os.path.exists(exe):
        raise SystemExit(f"{exe} is missing: make -C tools")
    with tempfile.TemporaryDirectory() as d:
        a, b = os.path.join(d, "Ap.bin"), os.path.join(d, "Aj.bin")
        Ap.cpu().numpy().tofile(a)
        Aj.cpu().numpy().tofile(b)
        sys.stdout.flush()
        r = subprocess.run(["timeout", "-k", "10", "400", exe, a, b, str(n), str(src), "3", *what], capture_output=True, text=True)
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            raise SystemExit(f"graph_bench_host failed ({r.returncode}): {r.stderr[-2000:]}")


def row_indices(cmi, torch, n, Ap, nnz):
    Ai = torch.empty(nnz, dtype=torch.int32, device="cuda")
    cmi.csr_row_indices(n, Ap, Ai)
    return Ai


def bandwidth(torch, cmi, n, Ap, Aj):
    return int((row_indices(cmi, torch, n, Ap, Aj.numel()) - Aj).abs().max())


def bfs_deep(cmi, torch, grid, skip_host, out):
    A = cmi.poisson5pt(grid, grid, "csr", device="cuda")
    n, Ap, Aj = A.num_rows, A.row_offsets, A.column_indices
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    libs = variant_libraries(cmi)
    own = cmi.bfs_levels_per_read()
    reached, depth = raw_search(cmi.lib(), cmi, torch, n, Ap, Aj, 0, True, labels)
    assert (reached, depth) == (n, 2 * (grid - 1)) and int(labels[-1]) == depth
    print(f"  bfs deep: poisson5pt {grid}^2 from vertex 0: {n} rows, {Aj.numel()} entries, {depth + 1} levels; K = levels per host read (the library: {own})")
    for mark, name in ((True, "levels"), (False, "predecessors")):
        t = interleaved(torch, {k: (lambda L=L: raw_search(L, cmi, torch, n, Ap, Aj, 0, mark, labels)) for k, L in libs.items()})
        for k, stat in t.items():
            show(f"device {name}, K = {k}{' (library)' if k == own else ''}", stat, f"{stat[0] * 1e3 / (depth + 1):.2f} us per level")
            out.append({"case": "bfs_deep", "grid": grid, "labels": name, "K": k, "ms": round(stat[0], 3), "min_max": [round(stat[1], 3), round(stat[2], 3)],
                        "us_per_level": round(stat[0] * 1e3 / (depth + 1), 3)})
    host_bench(n, Ap, Aj, 0, ["bfs"], skip_host)


def random_symmetric(torch, n, per_row, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    m = n * (per_row - 1) // 2
    i = torch.randint(0, n, (m,), device="cuda", generator=gen)
    j = torch.randint(0, n, (m,), device="cuda", generator=gen)
    keys = torch.unique(torch.cat([i * n + j, j * n + i, torch.arange(n, device="cuda") * (n + 1)]))
    del i, j
    rows = keys // n
    Aj = (keys - rows * n).to(torch.int32)
    Ap = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    Ap[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
    return Ap.to(torch.int32), Aj


def bfs_shallow(cmi, torch, n, skip_host, out):
    Ap, Aj = random_symmetric(torch, n, 8, 11)
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    reached, depth = raw_search(cmi.lib(), cmi, torch, n, Ap, Aj, 0, True, labels)
    first = torch.nonzero(labels >= 0).flatten()
    edges = int((Ap[first + 1] - Ap[first]).sum())               # the entries of the rows the search expands
    print(f"  bfs shallow: random symmetric pattern, {n} rows, {Aj.numel()} entries ({Aj.numel() / n:.2f} per row): depth {depth}, reached {reached}")
    t = interleaved(torch, {mark: (lambda mark=mark: raw_search(cmi.lib(), cmi, torch, n, Ap, Aj, 0, mark, labels)) for mark in (True, False)})
    for mark, stat in t.items():
        name = "levels" if mark else "predecessors"
        show(f"device {name}", stat, f"{edges / stat[0] / 1e6:.2f} G edges per second")
        out.append({"case": "bfs_shallow", "rows": n, "entries": Aj.numel(), "labels": name, "ms": round(stat[0], 3), "min_max": [round(stat[1], 3), round(stat[2], 3)],
                    "G_edges_per_s": round(edges / stat[0] / 1e6, 3)})
    host_bench(n, Ap, Aj, 0, ["bfs"], skip_host)


def permuted(cmi, torch, n, Ap, Aj, Ax, p):
    """symmetric_permute as the header layer does it on device_memory: (Ap, Aj, Ax) of P A P^T"""
    Ai = row_indices(cmi, torch, n, Ap, Aj.numel())
    ni, nj, nx = cmi.gather(Ai, p, n), cmi.gather(Aj, p, n), Ax.clone()
    cmi.coo_sort_by_row(n, n, ni, nj, nx, and_column=True)
    offsets = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    assert cmi.coo_row_offsets(n, ni, offsets)
    return offsets, nj, nx


def spmv_us(cmi, torch, n, Ap, Aj, Ax, x, y):
    plan = cmi.Plan.csr(torch.float64, n, n, Ap, Aj, None, None)
    fn = lambda: cmi.spmv_csr_plan(plan, Ap, Aj, Ax, x, y)  # noqa: E731
    for _ in range(5):
        fn()
    times = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / 20)
    return float(np.median(times)), plan


def ordering(cmi, torch, grid, skip_host, out):
    A = cmi.poisson5pt(grid, grid, "csr", device="cuda")
    n = A.num_rows
    gen = torch.Generator(device="cuda").manual_seed(5)
    shuffle = torch.randperm(n, device="cuda", generator=gen).to(torch.int32)
    Sp, Sj, Sx = permuted(cmi, torch, n, A.row_offsets, A.column_indices, A.values, shuffle)
    print(f"  ordering: poisson5pt {grid}^2 shuffled by a seeded random permutation: {n} rows, {Sj.numel()} entries")
    p, vertex = cmi.symmetric_rcm(n, Sp, Sj)
    _, _, searches = cmi.pseudo_peripheral_vertex(n, Sp, Sj)
    t = interleaved(torch, {"rcm": lambda: cmi.symmetric_rcm(n, Sp, Sj), "permute": lambda: permuted(cmi, torch, n, Sp, Sj, Sx, p)})
    show("device symmetric_rcm", t["rcm"], f"{searches} searches, pseudo-peripheral vertex {vertex}")
    show("device symmetric_permute", t["permute"], "two gathers + the COO sort by (row, column) + row offsets")
    host_bench(n, Sp, Sj, 0, ["rcm"], skip_host)
    Rp, Rj, Rx = permuted(cmi, torch, n, Sp, Sj, Sx, p)
    x = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen)
    y = torch.empty(n, dtype=torch.float64, device="cuda")
    copies = {"natural": (A.row_offsets, A.column_indices, A.values), "shuffled": (Sp, Sj, Sx), "reordered": (Rp, Rj, Rx)}
    us = {k: [] for k in copies}
    band = {k: bandwidth(torch, cmi, n, v[0], v[1]) for k, v in copies.items()}
    kernels = {}
    for _ in range(ROUNDS):
        for k, (Bp, Bj, Bx) in copies.items():
            t_us, plan = spmv_us(cmi, torch, n, Bp, Bj, Bx, x, y)
            us[k].append(t_us)
            kernels[k] = plan.config().kernel
    for k in copies:
        med = float(np.median(us[k]))
        print(f"    planned f64 cmi_spmv, {k:<10s} {med:10.1f} us [{min(us[k]):.1f}, {max(us[k]):.1f}]  bandwidth {band[k]}, kernel id {kernels[k]}, "
              f"{(12 * Sj.numel() + 20 * n) / med / 1e3:.0f} GB/s of the 12 nnz + 20 N model", flush=True)
        out.append({"case": "spmv", "grid": grid, "copy": k, "us": round(med, 2), "min_max": [round(min(us[k]), 2), round(max(us[k]), 2)], "bandwidth": band[k]})
    out.append({"case": "ordering", "grid": grid, "rcm_ms": round(t["rcm"][0], 3), "permute_ms": round(t["permute"][0], 3), "searches": searches})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grids", default="1000,3162")
    ap.add_argument("--deep", type=int, default=3162)
    ap.add_argument("--shallow", type=int, default=10_000_000)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import cusp_autotuned_amd as cmi
    print(f"graph_bench: medians of {ROUNDS} interleaved rounds [min, max]; searches on the host clock (they synchronise), multiplies by HIP events")
    rows = []
    bfs_deep(cmi, torch, args.deep, args.skip_host, rows)
    bfs_shallow(cmi, torch, args.shallow, args.skip_host, rows)
    for g in args.grids.split(","):
        ordering(cmi, torch, int(g), args.skip_host, rows)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    print(json.dumps({"graph_cases": len(rows)}))


if __name__ == "__main__":
    main()

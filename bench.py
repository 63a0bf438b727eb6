#!/usr/bin/env python3
"""bench.py -- SpMV GFLOP/s + achieved HBM GB/s (fp64) on 5-point Poisson, the metric of BASELINE.json.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
         --master-port P bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the K steps and prints the result line (`value`, `ms_per_step`, the workload's
config).  Everything below the timed steps -- the kernel's roofline (replayed and cold), the CG leg, the opt-in plans, the COO
tile kernel, the N > 1 exchange comparison and configs4 leg, the CPU baselines and their parity gate -- runs only with --full.
--dump-outputs DIR writes what the last timed step computed, a fixed, seeded sample of y with its global row indices
(DIR/y.npy, DIR/y_rows.npy, f64; N > 1: one pair per rank, suffixed _rank<r>), before any other leg runs.

A "step" = one pass of the hot path over one batch of synthetic input = one y = A*x with A, x, y resident in HBM:
cmi.multiply(A, x, y) -> the matrix's plan (cmi_plan_create, once) -> cmi_spmv_csr_plan_f64 -> the kernel the plan chose
(5-point rows in f64 beyond the cache: wave tiles with the 16-byte-vector body, csr_wavev V = 1; r2-r4 until session 20: csr_wave).

N = 1: BASELINE.json configs[1], poisson5pt 3162x3162 (9 998 244 rows, 49 978 572 entries), CSR,
       int32/f64, kernel + launch shape from the persisted tuning table.
N > 1: weak scaling -- every rank owns a 3162x3162-point row block of the global
       poisson5pt(3162, 3162*N) (N=8: 8.0e7 rows), global column indices; a step = exchange of x over xGMI + the
       local SpMV.  BOTH exchanges are timed with the same protocol and K and reported under `exchanges`:
         * the default ("auto"): the one-sided halo pull -- each rank copies the 2*3162 boundary values its rows
           reference straight out of its neighbours' mapped buffers with one small kernel on its own stream ("peer") --
           PROVEN FIRST IN A CHILD PROCESS that every rank starts before it makes any GPU call (a fault in the
           cross-GPU peer access then costs the child, and the run goes on with the two-sided RCCL halo exchange
           "halo"); it carries `value`;
         * "allgather": the north-star's literal exchange, an RCCL all-gather of the whole x before each multiply
           (cusp-autotuned_amd/distributed.py), with its y compared against the default exchange's.
       Per exchange: end-to-end GFLOP/s and ms per step, the exchange alone, the SpMV alone.
       `configs4` (N == 8, or --configs4 on): BASELINE.json configs[4]'s literal shape -- poisson5pt(10000, 10000),
       1e8 rows, row blocks of 1250 grid lines per rank -- SpMV with both exchanges and the fused CG on top, each
       validated (stencil closed form; recurrence residual against b - A x).

Timing protocol (reference performance/spmv/benchmark.h:84-120): W untimed warm-up steps, then
exactly K steps between a barrier + device synchronise on both sides; MAX over ranks.
The dominant kernel's launch duration is measured live with HIP events on the stream the kernel is launched
on (cmi_event_*): 10 batches of >= 20 launches (>= 200 in all, whatever --steps says), mean / median / fastest
batch; roofline.achieved uses the mean.

`roofline` is the REPLAY figure (the reference's protocol, performance/spmv/benchmark.h:84-120: one matrix multiplied back to back --
x (80 MB) and whatever else survives stays in the 256 MiB Infinity Cache between launches, and FETCH_SIZE counts its hits);
`roofline_cold` (N = 1) is the same kernel on FOUR distinct (A, x, y) sets at different addresses, visited round-robin -- 3.2 GB
touched between two uses of any line, so every launch streams everything from HBM: the figure a solver whose other kernels evict the
matrix, or a matrix ten times the size, would see.  Same 10 x >= 20 launch event protocol.

The `cpu_baseline` leg (rank 0, N = 1 only) times the REFERENCE's own sequential host kernel
(oracle/_ref, kind "reference", 1 core) -- or the C restatement (kind "port") when that library is absent --
on the same matrix for ~12 s, and checks the GPU result against it bit for bit; `cpu_baseline_omp` is the
OpenMP row-parallel kernel (kind "port": the reference's omp header does not compile here) on copies first-touched
in parallel, one pinned thread per allowed CPU (at most 16), timed in C.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# the host driver of this pool only supports dmabuf IPC (needed by RCCL and by the one-sided exchange's buffer mapping);
# normally exported already -- set before the HIP runtime is loaded in case it is not
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

M = 3162  # grid side: 3162^2 = 9 998 244 rows per GPU
# --format hyb: ELL width of the split.  4 leaves the fifth entry of every interior row (9 985 596 entries) to the COO part,
# so both kernels of the HYB multiply are timed (5 = the longest row would be ELL alone; the tuned width rule is
# cmi_hyb_entries_per_row, tools/autotune_hyb.py)
HYB_WIDTH = 4
HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E peak (MI355X_MICROARCH.md); ~6300 GB/s is what a copy achieves
DUMP_ROWS = 1 << 21     # --dump-outputs: rows of y sampled over all ranks (y and its row indices in f64: 32 MB)
DUMP_SEED = 20240607


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cg-iterations", type=int, default=300, help="iterations of the secondary CG leg (0 = skip)")
    ap.add_argument("--exchange", default="auto", choices=["auto", "peer", "halo", "allgather"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--format", default="csr", choices=["csr", "ell", "dia", "coo", "hyb"],
                    help="N=1 only: bench another format of the same matrix (BASELINE.json configs[2])")
    ap.add_argument("--configs4", default="auto", choices=["auto", "on", "off"],
                    help="N>1: the secondary leg on BASELINE.json configs[4]'s literal shape, poisson5pt(10000,10000) row-block "
                         "sharded over the N ranks, SpMV with both exchanges + CG (auto: when N == 8)")
    ap.add_argument("--configs4-grid", type=int, default=int(os.environ.get("CMI_BENCH_CONFIGS4_GRID", "10000")),
                    help="grid side of that leg (tests shrink it)")
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary legs: kernel roofline (replayed and cold), CG, the opt-in plans, the COO tile kernel, "
                         "N>1 exchange comparison and configs[4], the CPU baselines and their parity gate")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed (a fixed, seeded sample of y) as DIR/*.npy")
    ap.add_argument("--probe-peer", action="store_true", help=argparse.SUPPRESS)  # child mode, see peer_probe_child
    return ap.parse_args()


def peer_probe_child(args):
    """CHILD process (started by every rank of an N>1 run before the parent has made a single GPU call): maps the
    neighbours' exchange buffers over IPC and pulls from them with cmi_copy_ranges -- the one-sided exchange end to end on
    a small vector -- and reports through its exit code.  A GPU fault in the peer access kills this process, not the
    benchmark: the parent then times the two-sided / all-gather exchange instead.  Control plane: gloo on
    a port of its own (the probe must not depend on RCCL or disturb the parent's rendezvous)."""
    import torch
    import torch.distributed as dist
    import cusp_autotuned_amd as cmi
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = 0 if os.environ.get("CMI_BENCH_REHEARSAL", "0") == "1" else int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist.init_process_group("gloo", init_method=f"tcp://{os.environ.get('MASTER_ADDR', '127.0.0.1')}:{os.environ['MASTER_PORT']}",
                            rank=rank, world_size=world)
    piece, halo = 1 << 16, M  # the bench's halo: one grid line from each neighbour
    n = world * piece
    lo, hi = rank * piece, (rank + 1) * piece
    vec = cmi.distributed.ShardedVectorExchange(n, rank, world, max(lo - halo, 0), min(hi + halo, n) - 1, torch.float64, dev, mode="auto")
    ok = vec.plan.mode == "peer"  # _setup_peer mapped the neighbours and verified one pull on every rank
    if ok:  # and the steady state: repeated pulls of fresh values
        for it in range(3):
            vec.x_local.fill_(float(100 * it + rank + 1))
            vec.fence()
            vec.exchange()
            torch.cuda.synchronize()
            for p, (l, h) in enumerate(vec.plan.recv):
                if h > l and not bool((vec.x_full[l:h] == float(100 * it + p + 1)).all()):
                    ok = False
            vec.fence()
    vec.close()
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 3)


def run_peer_probe(world):
    """Parent side: spawn the probe, (ok, note).  Called before anything in this process touches the GPU."""
    import subprocess
    # (torchrun's TORCHELASTIC_USE_AGENT_STORE would make every child a CLIENT of a store nobody serves: the children run
    # their own tcp:// rendezvous, rank 0 serving)
    env = {k: v for k, v in os.environ.items() if not k.startswith("TORCHELASTIC_")}
    env["MASTER_PORT"] = str(int(env.get("MASTER_PORT", "29500")) + 23)
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--probe-peer", "--gpus", str(world)], env=env, timeout=300,  # a cold box pages torch in for a minute or two; the parents import it from a warm cache afterwards
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        return False, "probe timed out"
    if r.returncode == 0:
        return True, "ok"
    return False, f"probe exit {r.returncode}: {(r.stderr or r.stdout)[-200:]}"


def pmc_traffic(kernel_substr, ran=None):
    """(HBM-side bytes per launch of the dominant kernel, source file) from the newest committed rocprofv3 --pmc summary
    that has this kernel (profiles/*pmc*.json, produced by tools/pmc_summary.py from separate --pmc passes over the same
    matrix and tuning-table config), or (None, None).  PMC collection needs the profiler around the process, so the
    figure is a committed measurement of this kernel, not one taken in this run: the line says so (`traffic_source`)."""
    pdir = os.path.join(ROOT, "profiles")
    # the SpMV kernel of each format (not the builders / converters that carry the format's name too)
    names = {"csr": ("csr_wavev_kernel", "csr_wave_kernel", "csr_stream_kernel", "csr_balanced_kernel", "csr_vector_kernel", "csr_scalar_kernel"), "ell": ("ell_row_kernel",),
             "dia": ("dia_row_kernel", "dia_row2_kernel"), "coo": ("csr_wavev_kernel", "csr_wave_kernel", "csr_stream_kernel", "csr_balanced_kernel"),  # sorted entries through a plan: the CSR kernels on the plan's row offsets
             "coo_tile": ("coo_tile_kernel",), "hyb": ("hyb_tile_kernel",), "csr16": ("csr_wave16_kernel", "csr_stream16_kernel"),
             "csr16p": ("csr_wave16p_kernel",)}[kernel_substr]
    if ran is not None:  # the CSR kernel the matrix's plan actually runs (cmi_config.kernel): a summary of ANOTHER csr kernel is not this one's traffic
        by_enum = {1: "csr_scalar_kernel", 2: "csr_vector_kernel", 3: "csr_stream_kernel", 5: "csr_balanced_kernel", 7: "csr_wave_kernel", 8: "csr_wavev_kernel", 9: "csr_wavex_kernel", 11: "csr_waver_kernel"}
        names = (by_enum[ran],) if ran in by_enum else names
    best, src = None, None
    if os.path.isdir(pdir):
        for f in sorted(os.listdir(pdir)):
            if f.endswith(".json") and "pmc" in f and "before" not in f:
                try:
                    doc = json.load(open(os.path.join(pdir, f)))
                    if kernel_substr.split("_")[0] not in doc.get("probe", {}).get("formats", [kernel_substr]):
                        continue  # (a HYB run also launches ELL / COO kernels: only the run made for this format counts)
                    for k in doc.get("kernels", []):
                        if any(n in k.get("kernel", "") for n in names) and k.get("hbm_bytes_per_launch") and k.get("launches", 0) >= 5:
                            best, src = float(k["hbm_bytes_per_launch"]), "profiles/" + f
                except Exception:
                    pass
    return best, src


def cpu_baseline(cmi, A, x_host, y_gpu_host, seconds):
    """Times the reference's sequential host SpMV on the same matrix; checks the GPU result."""
    import numpy as np
    import oracle
    Ap, Aj, Ax = (t.cpu().numpy() for t in (A.row_offsets, A.column_indices, A.values))
    nnz = A.num_entries
    orc = oracle.Oracle()
    kind = "reference" if oracle.have_reference() else "port"
    if kind == "reference":
        refl = oracle.Reference()
        run = lambda: refl.spmv_csr(A.num_cols, Ap, Aj, Ax, x_host)  # noqa: E731
    else:
        run = lambda: orc.spmv_csr(Ap, Aj, Ax, x_host)  # noqa: E731
    y = run()  # warm-up (first touch)
    t0 = time.perf_counter()
    reps = 0
    while reps < 3 or (time.perf_counter() - t0 < seconds and reps < 500):
        y = run()
        reps += 1
    dt = (time.perf_counter() - t0) / reps
    exact = bool(np.array_equal(y, y_gpu_host))
    max_rel = float(np.max(np.abs(y - y_gpu_host)) / max(float(np.max(np.abs(y))), 1e-300))
    out = {"value": round(2.0 * nnz / dt / 1e9, 4), "unit": "GFLOP/s", "cores": 1, "kind": kind,
           "sample": f"{reps} full SpMVs of the same poisson5pt {M}x{M} CSR fp64 matrix ({dt * 1e3:.1f} ms each), "
                     "single thread, -O3 -ffp-contract=off",
           "ms_per_spmv": round(dt * 1e3, 3), "gpu_result_bit_exact": exact, "gpu_max_rel_err": max_rel}
    # The multi-core baseline: the OpenMP row-parallel kernel (reference omp/detail/multiply/csr_spmv.h:51-86, restated --
    # that header cannot be compiled here, DESIGN.md section 5 -- so kind "port"), on copies first-touched in parallel by the
    # threads that use them, one pinned thread per allowed CPU (at most 16: the CPU share of a one-GPU box), timed in C.
    try:
        allowed = len(os.sched_getaffinity(0))
    except AttributeError:
        allowed = os.cpu_count() or 1
    threads = max(1, min(allowed, 16))
    try:
        numa_nodes = len([d for d in os.listdir("/sys/devices/system/node") if d.startswith("node") and d[4:].isdigit()])
    except OSError:
        numa_nodes = None
    r = orc.bench_csr_omp(A.num_cols, Ap, Aj, Ax, x_host, threads=threads, seconds=max(seconds / 3, 2.0))
    dt2 = r["seconds_per_spmv"]
    omp_exact = bool(np.array_equal(r["y"], y))
    omp = {"value": round(2.0 * nnz / dt2 / 1e9, 4), "unit": "GFLOP/s", "cores": r["threads"], "kind": "port",
           "sample": f"{r['reps']} full SpMVs of the same matrix ({dt2 * 1e3:.2f} ms each), OpenMP static row split, "
                     "gcc -O3 -ffp-contract=off",
           "ms_per_spmv": round(dt2 * 1e3, 3), "threads_pinned": r["pinned"], "cpus": r["cpus"],
           "nproc": os.cpu_count(), "cpus_allowed": allowed, "numa_nodes": numa_nodes,
           "numa_policy": "default (local) allocation; every array first-touched in parallel by the thread that reads or "
                          "writes it (static row blocks; x by slices)",
           "identical_to_sequential_reference": omp_exact}
    if not (exact or max_rel <= 1e-6):
        raise SystemExit(f"parity gate failed: GPU y differs from the CPU reference (max rel {max_rel})")
    return out, omp


def stencil_expected(torch, cmi, m, n, lo, hi, dev, scale=1.0):
    """Rows [lo, hi) of y = poisson5pt(m, n) * x for the bench's x (cmi.fill_x), from the stencil itself:
    no matrix, no exchange, no kernel of the library.  Same arithmetic as the reference host loop
    (sequential/multiply/csr_spmv.h:60-72) on the gallery layout (columns ascending: i-m, i-1, i, i+1, i+m;
    values -1,-1,4,-1,-1): sum = 0, then sum = sum + a*x in storage order -- bit-exact in fp64 because -1*x
    and 4*x are exact.  Used to validate an N>1 exchange before it is timed and by the 1e8-row test."""
    N = m * n
    e0, e1 = max(lo - m, 0), min(hi + m, N)
    xe = (cmi.fill_x(e1 - e0, start=e0) * scale).to(dev)          # this rank's rows +- one grid line
    i = torch.arange(lo, hi, dtype=torch.int64, device=dev)
    ix = i % m
    zero = torch.zeros((), dtype=torch.float64, device=dev)

    def term(off, mask, coef):
        j = (i + off - e0).clamp_(0, e1 - e0 - 1)
        return torch.where(mask, coef * xe[j], zero)

    s = torch.zeros(hi - lo, dtype=torch.float64, device=dev)
    s = s + term(-m, i >= m, -1.0)
    s = s + term(-1, ix > 0, -1.0)
    s = s + term(0, i >= 0, 4.0)
    s = s + term(1, ix < m - 1, -1.0)
    s = s + term(m, i + m < N, -1.0)
    return s


def dump_outputs(out_dir, y, lo, rank, world):
    """--dump-outputs: what a caller of the timed path receives from its last step -- this rank's rows of y = A*x (f64) -- as a
    fixed, seeded sample of DUMP_ROWS / world rows (all of them when fewer): y.npy and y_rows.npy (global row indices, f64);
    N > 1: one pair per rank, suffixed _rank<r>.  Same arguments, same rows, same file names."""
    import numpy as np
    yh = y.cpu().numpy()
    n = yh.shape[0]
    k = min(n, DUMP_ROWS // world)
    rows = np.arange(n) if k == n else np.sort(np.random.default_rng(DUMP_SEED + rank).choice(n, size=k, replace=False))
    suffix = "" if world == 1 else f"_rank{rank}"
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, f"y{suffix}.npy"), yh[rows].astype(np.float64))
    np.save(os.path.join(out_dir, f"y_rows{suffix}.npy"), (rows + lo).astype(np.float64))


def configs4_leg(torch, cmi, dist, args, rank, world, dev, barrier, timed_steps):
    """poisson5pt(g, g) (g = 10000: 1e8 rows, 499 960 000 entries) in row blocks of whole grid lines, one per rank, global
    column indices: SpMV with the default exchange and with the all-gather, each validated against the stencil's closed
    form, then the fused CG (p exchanged once with the one-sided exchange, cusp/krylov/detail/cg.inl:77-105 otherwise)."""
    g = args.configs4_grid
    lines = -(-g // world)
    l0, l1 = min(rank * lines, g), min((rank + 1) * lines, g)
    lo, hi = l0 * g, l1 * g
    N, nnz = g * g, cmi.poisson5pt_num_entries(g, g)
    offsets = [min(r * lines, g) * g for r in range(world + 1)]
    A = cmi.poisson5pt(g, g, "csr", dtype=torch.float64, device=dev, row_begin=lo, row_end=hi)
    xh = cmi.fill_x(hi - lo, start=lo).to(dev)
    want = stencil_expected(torch, cmi, g, g, lo, hi, dev)
    span = (max(lo - g, 0), min(hi + g, N) - 1)
    out = {"workload": f"poisson5pt {g}x{g} CSR int32/f64 ({N} rows, {nnz} entries), row blocks of {lines} grid lines x{world}",
           "rows_per_gpu": hi - lo, "exchanges": {}}
    y = torch.empty(hi - lo, dtype=torch.float64, device=dev)
    steps = max(5, min(args.steps, 50))
    default_mode = None
    for mode in (args.exchange, "allgather"):
        if mode == default_mode:
            continue
        sh = cmi.distributed.ShardedCsr(A, N, rank, world, mode=mode, col_span=span, offsets=offsets)
        got_mode = sh.vec.plan.mode
        if default_mode is None:
            default_mode = got_mode
        elif got_mode in out["exchanges"]:
            sh.vec.close()
            continue
        sh.x_local.copy_(xh)
        sh.vec.fence()
        y.fill_(10.0)
        sh.multiply(y)
        good = torch.tensor([int(torch.equal(y, want))], dtype=torch.int32, device=dev)
        dist.all_reduce(good, op=dist.ReduceOp.MIN)
        sec = timed_steps(lambda: sh.multiply(y), steps)
        rec = {"value": round(2.0 * nnz / sec / 1e9, 3), "unit": "GFLOP/s", "ms_per_step": round(sec * 1e3, 5), "steps": steps,
               "bit_exact_vs_stencil_closed_form": bool(int(good.item())),
               "exchange_only_ms": round(timed_steps(sh.vec.exchange, steps) * 1e3, 5)}
        if args.cg_iterations > 0:
            its = min(args.cg_iterations, 50)
            x_sol = torch.zeros(hi - lo, dtype=torch.float64, device=dev)
            cmi.krylov.cg(sh, x_sol.clone(), xh, iteration_limit=2, relative_tolerance=0.0)
            barrier()
            t0 = time.perf_counter()
            mon = cmi.krylov.cg(sh, x_sol, xh, iteration_limit=its, relative_tolerance=0.0)
            barrier()
            tt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            sh.vec.fence()
            sh.x_local.copy_(x_sol)
            sh.vec.fence()
            r_true = torch.empty_like(xh)
            sh.multiply(r_true)
            rr = ((xh - r_true) ** 2).sum().reshape(1)
            dist.all_reduce(rr)
            true_norm = float(rr.item()) ** 0.5
            rec["cg"] = {"iterations": mon.iteration_count, "iterations_per_s": round(mon.iteration_count / float(tt.item()), 1),
                         "us_per_iteration": round(float(tt.item()) / max(mon.iteration_count, 1) * 1e6, 2),
                         "final_residual_norm": mon.residuals[-1], "true_residual_norm": true_norm,
                         "residual_consistent": bool(abs(true_norm - mon.residuals[-1]) <= 1e-6 * mon.residuals[0])}
        out["exchanges"][got_mode] = rec
        sh.vec.close()
    return out


def main():
    args = parse()
    if args.probe_peer:
        return peer_probe_child(args)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    # N>1 with the one-sided exchange in play: prove it in a CHILD process first -- before this process makes any GPU call --
    # so that a fault in the cross-GPU peer access (never exercised between two devices before the driver's 8-GPU run)
    # costs a child, not the benchmark.  Every rank spawns its child; the verdicts are agreed on below (all-reduce MIN).
    peer_probe = None
    if world > 1 and world == args.gpus and args.exchange in ("auto", "peer") and os.environ.get("CMI_EXCHANGE_PEER", "1") != "0":
        peer_probe = run_peer_probe(world)
    import torch
    import cusp_autotuned_amd as cmi

    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit(f"--gpus {args.gpus} needs one process per GPU: launch with "
                             f"python -m torch.distributed.run --nproc-per-node {args.gpus} ... bench.py --gpus {args.gpus}")
        raise SystemExit(f"WORLD_SIZE={world} does not match --gpus {args.gpus}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    # CMI_BENCH_REHEARSAL=1 (tests only): all ranks share GPU 0 and talk over gloo, so that the N>1
    # code path can be exercised end to end on a one-GPU box.  RCCL refuses two ranks on one device.
    rehearsal = os.environ.get("CMI_BENCH_REHEARSAL", "0") == "1"
    if rehearsal:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        if rehearsal:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        if peer_probe is not None:
            flag = torch.tensor([int(peer_probe[0])], dtype=torch.int32, device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if os.environ.get("CMI_BENCH_FAIL_PROBE", "0") == "1":
                flag.zero_()  # tests only: pretend a child faulted, to exercise the hand-over
            if int(flag.item()) == 0:
                os.environ["CMI_EXCHANGE_PEER"] = "0"  # distributed.py: "auto" then means the two-sided halo exchange
                if args.exchange == "peer":
                    args.exchange = "halo"
                peer_probe = (False, peer_probe[1] if not peer_probe[0] else "another rank's probe failed")
                print(f"[bench] rank {rank}: one-sided exchange not used: {peer_probe[1]}", file=sys.stderr, flush=True)

    lib = cmi.lib()
    stream = torch.cuda.current_stream()
    sptr = ctypes.c_void_p(stream.cuda_stream)

    # ---- workload --------------------------------------------------------------------------
    m, n = M, M * world
    rows_per_rank = M * M
    lo, hi = rank * rows_per_rank, (rank + 1) * rows_per_rank
    A = cmi.poisson5pt(m, n, "csr", dtype=torch.float64, device=dev, row_begin=lo, row_end=hi)
    N_global = m * n
    nnz_global = cmi.poisson5pt_num_entries(m, n)
    fmt = args.format if world == 1 else "csr"
    Afmt = A if fmt == "csr" else (cmi.poisson5pt(m, n, "dia", device=dev) if fmt == "dia" else
                                   cmi.convert(A, fmt, num_entries_per_row=HYB_WIDTH if fmt == "hyb" else None))
    # deterministic, RNG-free input; each rank generates only its own slice
    x_host = cmi.fill_x(rows_per_rank, start=lo).numpy()
    y = torch.full((rows_per_rank,), 10.0, dtype=torch.float64, device=dev)

    if world == 1:
        x = torch.from_numpy(x_host).to(dev)
        step = lambda: cmi.multiply(Afmt, x, y)  # noqa: E731
        exchange_info = None
    else:
        # The exchange is validated BEFORE anything is timed: one sharded multiply against the stencil's closed
        # form (bit-exact, no other exchange involved).  A transport that maps its neighbours' buffers but
        # delivers wrong halos is dropped for the next one (peer -> halo -> allgather), on every rank alike.
        span = (max(lo - m, 0), min(hi + m, N_global) - 1)
        want = stencil_expected(torch, cmi, m, n, lo, hi, dev)
        rejected = []
        sh = None
        for mode_try in {"auto": ["auto", "halo", "allgather"], "peer": ["peer", "halo", "allgather"],
                         "halo": ["halo", "allgather"], "allgather": ["allgather"]}[args.exchange]:
            if sh is not None:
                sh.vec.close()
            sh = cmi.distributed.ShardedCsr(A, N_global, rank, world, mode=mode_try, col_span=span)
            sh.x_local.copy_(torch.from_numpy(x_host).to(dev))
            sh.vec.fence()
            y.fill_(10.0)
            sh.multiply(y)
            good = torch.tensor([int(torch.equal(y, want))], dtype=torch.int32, device=dev)
            if sh.vec.plan.mode in os.environ.get("CMI_BENCH_REJECT", "").split(","):
                good.zero_()  # tests only: pretend this exchange delivered wrong halos, to exercise the hand-over
            dist.all_reduce(good, op=dist.ReduceOp.MIN)
            if int(good.item()) == 1:
                break
            rejected.append(sh.vec.plan.mode)
        else:
            raise SystemExit(f"parity gate failed: sharded y differs from the stencil's closed form with every exchange {rejected}")
        del want
        step = lambda: sh.multiply(y)  # noqa: E731
        # per rank: the data path's communicator as the LIBRARY reports it (cmi_comm_rank: ncclCommCount of the RCCL communicator behind
        # the C-ABI) and the exchange that carries `value` -- so that the N > 1 line itself shows N ranks talking through RCCL
        me = {"rank": rank, "device": torch.cuda.current_device(), "exchange": sh.vec.plan.mode, "data_path": "torch.distributed", "comm_world": None}
        if sh.vec.comm is not None:
            r_, w_ = ctypes.c_int(-1), ctypes.c_int(-1)
            cmi.check(cmi.lib().cmi_comm_rank(sh.vec.comm.handle, ctypes.byref(r_), ctypes.byref(w_)))
            me.update(data_path="cmi_comm (RCCL behind the C-ABI)", comm_rank=r_.value, comm_world=w_.value, rccl_version=sh.vec.comm.library_version())
        per_rank = [None] * world
        dist.all_gather_object(per_rank, me)
        p = sh.vec.plan
        exchange_info = {"mode": p.mode, "values_received_per_rank": p.allgather_values if p.mode == "allgather" else p.recv_values,
                         "allgather_values": p.allgather_values, "validated_against": "stencil closed form (bit-exact)",
                         "rejected_exchanges": rejected,
                         "peer_probe_in_child_process": None if peer_probe is None else {"ok": peer_probe[0], "note": peer_probe[1]},
                         "ranks": per_rank}

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # ---- settle, warm-up, then exactly K timed steps ----------------------------------------------
    # Settle phase (disclosed as `settle_launches`, not part of W or K): the device comes out of setup at idle clocks
    # and a 20-step timed region lasts < 3 ms, so the clocks are brought up first.  Then the contract's W warm-up steps.
    SETTLE = 100
    # launch ledger of the hot path's kernel at N = 1 (phase, launches), in launch order: a rocprofv3 kernel trace of this command can
    # then be cut into its phases (tools/trace_phases.py) -- the replay legs and the cold leg launch the SAME kernel, so the trace's one
    # average per kernel name mixes them ("rocprofv3 average duration for that kernel must agree" is checked per phase)
    ledger = []
    for _ in range(SETTLE):
        step()
    barrier()
    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    ledger += [["settle", SETTLE], ["warmup", args.warmup], ["timed_steps", args.steps]]
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs:  # before any secondary leg launches anything
        dump_outputs(args.dump_outputs, y, lo, rank, world)

    # ---- N>1: BOTH exchanges are first-class results: the default one (one-sided halo pull where it
    #      validated) carries `value`; the north-star's literal exchange -- RCCL all-gather of the whole x before each
    #      multiply -- is timed beside it with the SAME protocol and the same K, and its y compared with the default's.
    #      Per exchange: end-to-end GFLOP/s and ms per step, the exchange alone, and (below) the SpMV alone. ------------------
    def timed_steps(fn, steps, warm=3):
        for _ in range(warm):
            fn()
        barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        barrier()
        tt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        if dist is not None:
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        return float(tt.item()) / steps

    exchanges = None
    if dist is not None and args.full:
        exchanges = {exchange_info["mode"]: {"value": round(2.0 * nnz_global / (elapsed / args.steps) / 1e9, 3), "unit": "GFLOP/s",
                                             "ms_per_step": round(elapsed / args.steps * 1e3, 5), "steps": args.steps,
                                             "values_received_per_rank": exchange_info["values_received_per_rank"],
                                             "exchange_only_ms": round(timed_steps(sh.vec.exchange, args.steps) * 1e3, 5),
                                             "carries_value": True}}
        if exchange_info["mode"] != "allgather":
            try:
                sh_ag = cmi.distributed.ShardedCsr(A, N_global, rank, world, mode="allgather")
                sh_ag.x_local.copy_(sh.x_local)
                y_ag = torch.empty_like(y)
                ag_s = timed_steps(lambda: sh_ag.multiply(y_ag), args.steps)
                same = torch.tensor([int(torch.equal(y_ag, y))], dtype=torch.int32, device=dev)
                dist.all_reduce(same, op=dist.ReduceOp.MIN)
                exchanges["allgather"] = {"value": round(2.0 * nnz_global / ag_s / 1e9, 3), "unit": "GFLOP/s", "ms_per_step": round(ag_s * 1e3, 5),
                                          "steps": args.steps, "values_received_per_rank": sh_ag.vec.plan.allgather_values,
                                          "exchange_only_ms": round(timed_steps(sh_ag.vec.exchange, args.steps) * 1e3, 5),
                                          "y_identical_to_default_exchange": bool(int(same.item())), "carries_value": False}
                del sh_ag, y_ag
            except Exception as e:  # noqa: BLE001 -- a secondary leg must never take the main line down
                exchanges["allgather"] = {"error": f"{type(e).__name__}: {e}"[:300]}

    # ---- dominant kernel: launch duration with HIP events on ITS stream ---------------------------------------
    # >= 200 launches whatever --steps says, as KERNEL_BATCHES batches of launches each bracketed by its own event pair
    # (a batch, not a single launch: an event pair around one launch also times the ~2 us launch gap).  Reported:
    # the mean over all batches (= the average launch duration, what roofline.achieved is computed from), the median
    # batch and the fastest batch.  Launch-to-launch spread on this pool is 130-161 us (archive/profiles/r01_bench_kernel_stats.csv),
    # so 20 launches after a cold start -- round 1's protocol -- could land 5 % off the average.
    KERNEL_BATCHES = 10
    per_batch = max(20, -(-max(args.steps, 200) // KERNEL_BATCHES))
    x_kernel = x if world == 1 else sh.x_view
    kernel_only = (lambda: cmi.multiply(Afmt, x_kernel, y))
    kernel_ms = None
    if args.full:
        evs = []
        for _ in range(2 * KERNEL_BATCHES):
            e = ctypes.c_void_p()
            cmi.check(lib.cmi_event_create(ctypes.byref(e)))
            evs.append(e)
        for _ in range(10):  # re-warm: the secondary legs above ran other kernels
            kernel_only()
        torch.cuda.synchronize()
        for bi in range(KERNEL_BATCHES):
            cmi.check(lib.cmi_event_record(evs[2 * bi], sptr))
            for _ in range(per_batch):
                kernel_only()
            cmi.check(lib.cmi_event_record(evs[2 * bi + 1], sptr))
        ledger += [["roofline_rewarm", 10], ["roofline", KERNEL_BATCHES * per_batch]]
        batch_ms = []
        for bi in range(KERNEL_BATCHES):
            ms = ctypes.c_float()
            cmi.check(lib.cmi_event_elapsed_ms(evs[2 * bi], evs[2 * bi + 1], ctypes.byref(ms)))
            batch_ms.append(ms.value / per_batch)
        for e in evs:
            cmi.check(lib.cmi_event_destroy(e))
        kernel_ms = sum(batch_ms) / len(batch_ms)
        kernel_ms_median = sorted(batch_ms)[len(batch_ms) // 2]
        kernel_ms_min = min(batch_ms)
        if dist is not None:
            t = torch.tensor([kernel_ms, kernel_ms_median, kernel_ms_min], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            kernel_ms, kernel_ms_median, kernel_ms_min = (float(v) for v in t.tolist())

    # ---- cold leg (N = 1): the same kernel with nothing of its operands left in any cache ---------------------
    # COLD_SETS distinct copies of (A, x, y) -- 800 MB each for CSR -- multiplied round-robin: between two uses of a line 3 other
    # sets (2.4 GB) have streamed through the 256 MiB Infinity Cache and the 8 x 4 MiB L2s.  Each copy has its own plan (plans are
    # keyed by the arrays' addresses), made and warmed before the timed batches.
    cold = None
    COLD_SETS = 4
    if args.full and world == 1 and os.environ.get("CMI_BENCH_COLD", "1") != "0":
        try:
            import copy as _copy

            def clone_matrix(Am):
                B2 = _copy.copy(Am)
                for k, v in vars(Am).items():
                    if isinstance(v, torch.Tensor):
                        setattr(B2, k, v.clone())
                    elif hasattr(v, "__dict__") and any(isinstance(t, torch.Tensor) for t in vars(v).values()):  # hyb's ell / coo parts
                        setattr(B2, k, clone_matrix(v))
                for k in ("_plan", "_plan_key", "_plan_args"):
                    if hasattr(B2, k):
                        setattr(B2, k, None)
                return B2
            sets = [(Afmt, x, y)] + [(clone_matrix(Afmt), x.clone(), torch.empty_like(y)) for _ in range(COLD_SETS - 1)]
            for Ak, xk, yk in sets:
                cmi.multiply(Ak, xk, yk)
            same = all(bool(torch.equal(yk, y)) for _, _, yk in sets)
            torch.cuda.synchronize()
            cevs = []
            for _ in range(2 * KERNEL_BATCHES):
                e = ctypes.c_void_p()
                cmi.check(lib.cmi_event_create(ctypes.byref(e)))
                cevs.append(e)
            per_cold = -(-per_batch // COLD_SETS) * COLD_SETS
            for bi in range(KERNEL_BATCHES):
                cmi.check(lib.cmi_event_record(cevs[2 * bi], sptr))
                for i in range(per_cold):
                    Ak, xk, yk = sets[i % COLD_SETS]
                    cmi.multiply(Ak, xk, yk)
                cmi.check(lib.cmi_event_record(cevs[2 * bi + 1], sptr))
            cb = []
            for bi in range(KERNEL_BATCHES):
                ms = ctypes.c_float()
                cmi.check(lib.cmi_event_elapsed_ms(cevs[2 * bi], cevs[2 * bi + 1], ctypes.byref(ms)))
                cb.append(ms.value / per_cold)
            for e in cevs:
                cmi.check(lib.cmi_event_destroy(e))
            cold = {"kernel_avg_ms": sum(cb) / len(cb), "kernel_median_ms": sorted(cb)[len(cb) // 2], "kernel_min_ms": min(cb),
                    "sets": COLD_SETS, "launches": per_cold * KERNEL_BATCHES, "results_identical_across_sets": same}
            del sets
            torch.cuda.empty_cache()
            for _ in range(10):  # re-warm the replay state for the legs below
                kernel_only()
            torch.cuda.synchronize()
            ledger += [["cold_first_touch", COLD_SETS], ["roofline_cold", per_cold * KERNEL_BATCHES], ["cold_rewarm", 10]]
        except Exception as e:  # noqa: BLE001 -- a secondary leg
            cold = {"error": f"{type(e).__name__}: {e}"[:300]}

    # ---- the caller: CG iterations/s on the same matrix (cusp::krylov::cg's loop, cg.inl:80-105; fused device
    #      path, sharded when N>1), with the recurrence residual checked against b - A x at the end -----------
    cg_leg = None
    if args.full and fmt == "csr" and args.cg_iterations > 0:
        try:
            b_vec = torch.from_numpy(x_host).to(dev)
            x_sol = torch.zeros(rows_per_rank, dtype=torch.float64, device=dev)
            op = A if world == 1 else sh
            cmi.krylov.cg(op, x_sol.clone(), b_vec, iteration_limit=3, relative_tolerance=0.0)  # warm-up
            barrier()
            t0 = time.perf_counter()
            mon = cmi.krylov.cg(op, x_sol, b_vec, iteration_limit=args.cg_iterations, relative_tolerance=0.0)
            barrier()
            t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
            if dist is not None:
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
            # true residual of the returned x
            r_true = torch.empty_like(b_vec)
            if world == 1:
                cmi.multiply(A, x_sol, r_true)
            else:
                sh.vec.fence()
                sh.x_local.copy_(x_sol)
                sh.vec.fence()
                sh.multiply(r_true)
            rr = ((b_vec - r_true) ** 2).sum().reshape(1)
            if dist is not None:
                dist.all_reduce(rr)
            true_norm = float(rr.item()) ** 0.5
            cg_s = float(t.item())
            # the marginal iteration: the same solve with half the iterations, subtracted (the first SpMV, r = b - A x, the first dot,
            # the closing synchronisation are in both)
            half = max(args.cg_iterations // 2, 1)
            barrier()
            t0 = time.perf_counter()
            cmi.krylov.cg(op, torch.zeros_like(x_sol), b_vec, iteration_limit=half, relative_tolerance=0.0)
            barrier()
            th = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
            if dist is not None:
                dist.all_reduce(th, op=dist.ReduceOp.MAX)
            marginal = (cg_s - float(th.item())) / max(mon.iteration_count - half, 1) * 1e6
            cg_leg = {"iterations": mon.iteration_count, "iterations_per_s": round(mon.iteration_count / cg_s, 1),
                      "us_per_iteration": round(cg_s / max(mon.iteration_count, 1) * 1e6, 2),
                      "us_per_marginal_iteration": round(marginal, 2),
                      "final_residual_norm": mon.residuals[-1], "true_residual_norm": true_norm,
                      "residual_consistent": bool(abs(true_norm - mon.residuals[-1]) <= 1e-6 * mon.residuals[0]),
                      "exchange": None if world == 1 else sh.vec.plan.mode}
        except Exception as e:  # noqa: BLE001 -- a secondary leg
            cg_leg = {"error": f"{type(e).__name__}: {e}"[:300]}

    # ---- opt-in plans: the 16-bit column copy (CMI_CSR_STREAM_C16, csrc/spmv_csr16.hip) and the PACKED wave tiles (CMI_CSR_STREAM_PACKED: per
    #      tile of 64 rows one contiguous span [row starts | 16-bit columns | values]) -- NOT the headline: `value` and
    #      `roofline` above are the plain kernel reading the caller's 32-bit arrays.  Reported beside them, replayed AND cold (the headline's
    #      two protocols), because moving fewer bytes / one stream instead of four is the one way left to make this multiply faster: same
    #      products, same sums, same bits.
    def opt_in_leg(kind):
        """kind "c16" | "packed": (dict) replay + cold timing of the headline matrix through that plan"""
        def make(Ap_, Aj_, Ax_):
            if kind == "c16":
                return cmi.Plan.csr(torch.float64, A.num_rows, A.num_cols, Ap_, Aj_, cfg=cmi.Config(kernel=cmi.CSR_STREAM_C16))
            return cmi.Plan.csr_values(A.num_rows, A.num_cols, Ap_, Aj_, Ax_, cfg=cmi.Config(kernel=cmi.CSR_STREAM_PACKED))
        want_kernel = cmi.CSR_STREAM_C16 if kind == "c16" else cmi.CSR_STREAM_PACKED
        pl = make(A.row_offsets, A.column_indices, A.values)
        pc = pl.config()
        if pc.kernel != want_kernel:
            return {"granted": False, "why": "a row tile spans 65536+ columns or does not fit one LDS pass"}, None
        yk = torch.full_like(y, -1.0)
        run = lambda: cmi.spmv_csr_plan(pl, A.row_offsets, A.column_indices, A.values, x, yk)  # noqa: E731
        for _ in range(20):
            run()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * KERNEL_BATCHES)]
        for bi in range(KERNEL_BATCHES):
            ev[2 * bi].record()
            for _ in range(per_batch):
                run()
            ev[2 * bi + 1].record()
        torch.cuda.synchronize()
        bb = [ev[2 * bi].elapsed_time(ev[2 * bi + 1]) / per_batch for bi in range(KERNEL_BATCHES)]
        ms = sum(bb) / len(bb)
        cmi.multiply(A, x, y)
        wtiles = -(-A.num_rows // pc.rows_per_block)
        if kind == "c16":
            moved = 10 * A.num_entries + 20 * A.num_rows + 4 + 4 * wtiles
            owned = 2 * A.num_entries + 16 + 4 * wtiles
        else:
            owned = pl.device_bytes()
            moved = owned + 16 * A.num_rows  # the packed tiles + x once + y once
        out = {"granted": True, "kernel_config": pc.as_dict(), "kernel_avg_ms": round(ms, 6), "kernel_min_ms": round(min(bb), 6),
               "gflops": round(2.0 * A.num_entries / (ms * 1e-3) / 1e9, 2),
               "bytes_read_and_written_per_launch": moved, "moved_gbps": round(moved / (ms * 1e-3) / 1e9, 2),
               "moved_frac_of_peak": round(moved / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
               "csr_algorithmic_bytes_over_time_gbps": round(cmi.csr_bytes(A.num_rows, A.num_entries) / (ms * 1e-3) / 1e9, 2),
               "hbm_bytes_owned_by_the_plan": owned,
               "y_identical_to_the_plain_kernel": bool(torch.equal(yk, y)),
               "speedup_over_the_headline_kernel": round(kernel_ms / ms, 4)}
        out["traffic"], out["traffic_source"] = pmc_traffic("csr16" if kind == "c16" else "csr16p")
        # cold: COLD_SETS distinct (A, x, y, plan) sets round-robin, as roofline_cold does for the headline kernel
        if os.environ.get("CMI_BENCH_COLD", "1") != "0":
            sets = [(A.row_offsets, A.column_indices, A.values, x, yk, pl)]
            for _ in range(COLD_SETS - 1):
                a2, j2, v2 = A.row_offsets.clone(), A.column_indices.clone(), A.values.clone()
                sets.append((a2, j2, v2, x.clone(), torch.empty_like(y), make(a2, j2, v2)))
            for a2, j2, v2, x2, y2, p2 in sets:
                cmi.spmv_csr_plan(p2, a2, j2, v2, x2, y2)
            same = all(bool(torch.equal(t[4], y)) for t in sets)
            per_cold = -(-per_batch // COLD_SETS) * COLD_SETS
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * KERNEL_BATCHES)]
            torch.cuda.synchronize()
            for bi in range(KERNEL_BATCHES):
                ev[2 * bi].record()
                for i in range(per_cold):
                    a2, j2, v2, x2, y2, p2 = sets[i % COLD_SETS]
                    cmi.spmv_csr_plan(p2, a2, j2, v2, x2, y2)
                ev[2 * bi + 1].record()
            torch.cuda.synchronize()
            cb2 = [ev[2 * bi].elapsed_time(ev[2 * bi + 1]) / per_cold for bi in range(KERNEL_BATCHES)]
            cms = sum(cb2) / len(cb2)
            out["cold"] = {"kernel_avg_ms": round(cms, 6), "kernel_min_ms": round(min(cb2), 6), "sets": COLD_SETS,
                           "moved_frac_of_peak": round(moved / (cms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                           "csr_algorithmic_bytes_over_time_gbps": round(cmi.csr_bytes(A.num_rows, A.num_entries) / (cms * 1e-3) / 1e9, 2),
                           "speedup_over_the_headline_kernel_cold": None if not cold or "error" in cold else round(cold["kernel_avg_ms"] / cms, 4),
                           "results_identical_across_sets": same}
            del sets
            torch.cuda.empty_cache()
        del yk
        return out, pl

    c16 = packed = None
    if args.full and fmt == "csr" and world == 1:
        try:
            c16, p16 = opt_in_leg("c16")
            if c16.get("granted") and args.cg_iterations > 0:
                A.plan(compress=True)
                b_vec = torch.from_numpy(x_host).to(dev)
                x_sol = torch.zeros(rows_per_rank, dtype=torch.float64, device=dev)
                cmi.krylov.cg(A, x_sol.clone(), b_vec, iteration_limit=3, relative_tolerance=0.0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                mon = cmi.krylov.cg(A, x_sol, b_vec, iteration_limit=args.cg_iterations, relative_tolerance=0.0)
                torch.cuda.synchronize()
                cg_s = time.perf_counter() - t0
                c16["cg_us_per_iteration"] = round(cg_s / max(mon.iteration_count, 1) * 1e6, 2)
                c16["cg_final_residual_norm"] = mon.residuals[-1]
                A.plan(compress=False)
            del p16
        except Exception as e:  # noqa: BLE001 -- a secondary leg
            c16 = {"error": f"{type(e).__name__}: {e}"[:300]}
        try:
            packed, ppk = opt_in_leg("packed")
            if packed.get("granted") and c16 and c16.get("granted"):
                packed["speedup_over_the_16_bit_plan"] = round(c16["kernel_avg_ms"] / packed["kernel_avg_ms"], 4)
                if "cold" in packed and "cold" in c16:
                    packed["cold"]["speedup_over_the_16_bit_plan_cold"] = round(c16["cold"]["kernel_avg_ms"] / packed["cold"]["kernel_avg_ms"], 4)
            del ppk
        except Exception as e:  # noqa: BLE001 -- a secondary leg
            packed = {"error": f"{type(e).__name__}: {e}"[:300]}
        cmi.multiply(A, x, y)

    # ---- N>1: BASELINE.json configs[4]'s literal shape -- poisson5pt(10000, 10000), 1e8 rows, row-block sharded over the
    #      N ranks, inside cusp::krylov::cg -- as a secondary leg (the headline stays weak-scaled: 3162^2 rows per GPU) ----
    configs4 = None
    if args.full and dist is not None and (args.configs4 == "on" or (args.configs4 == "auto" and world == 8)):
        try:
            configs4 = configs4_leg(torch, cmi, dist, args, rank, world, dev, barrier, timed_steps)
        except Exception as e:  # noqa: BLE001
            configs4 = {"error": f"{type(e).__name__}: {e}"[:300]}

    # ---- numbers -------------------------------------------------------------------------------
    ms_per_step = elapsed / args.steps * 1e3
    gflops = 2.0 * nnz_global / (elapsed / args.steps) / 1e9
    local_nnz, local_rows = A.num_entries, A.num_rows
    if fmt == "csr":
        alg_bytes = cmi.csr_bytes(local_rows, local_nnz)
        kname = "csr"
    elif fmt == "ell":
        alg_bytes, kname = cmi.ell_bytes(local_rows, Afmt.num_entries_per_row, Afmt.pitch), "ell"
    elif fmt == "dia":
        alg_bytes, kname = cmi.dia_bytes(local_rows, 5, Afmt.pitch), "dia"
    elif fmt == "coo":
        # Sorted COO multiplies through its plan: the CSR kernel on plan-built row offsets -- the row indices are never read.  The
        # roofline is priced on the bytes THAT kernel must move (CSR's 12 nnz + 20 N + 4: offsets instead of row indices), so `frac`
        # cannot exceed 1 (priced on COO's 16 bytes per entry the same launch printed 1.011); COO's own byte
        # count and the COO tile kernel, which does read the row indices, are reported beside it (`coo_tile_kernel`).
        coo_bytes_ = cmi.coo_bytes(local_rows, local_nnz)
        through_csr = world == 1 and Afmt.plan().config().kernel in (cmi.CSR_STREAM, cmi.CSR_STREAM_WAVE, cmi.CSR_STREAM_WAVEV, cmi.CSR_BALANCED, cmi.CSR_SCALAR, cmi.CSR_VECTOR)
        alg_bytes, kname = (cmi.csr_bytes(local_rows, local_nnz) if through_csr else coo_bytes_), "coo"
    else:  # hyb: the ELL part's bytes (x and y once) + the COO part's three streams; one launch (the matrix's HYB plan)
        alg_bytes, kname = cmi.ell_bytes(local_rows, HYB_WIDTH, Afmt.ell.pitch) + 16 * Afmt.coo.num_entries, "hyb"
    cfg = cmi.tuning_select({"csr": 0, "ell": 1, "dia": 2, "coo": 3, "hyb": 1}[fmt], cmi.F64, local_rows, N_global,
                            local_nnz if fmt in ("csr", "coo") else local_rows * (HYB_WIDTH if fmt == "hyb" else 5))
    if world == 1 and fmt in ("csr", "coo"):  # what actually ran: the matrix's plan may have turned the table entry into another kernel
        try:                                   # (stencil rows: the wave-tile kernel; skewed rows: the merge-path kernel)
            cfg = Afmt.plan().config()
        except Exception:  # noqa: BLE001
            pass
    if args.full:
        achieved = alg_bytes / (kernel_ms * 1e-3) / 1e9
        traffic, traffic_src = pmc_traffic(kname, cfg.kernel if world == 1 and fmt in ("csr", "coo") else None)
    coo_tile = None
    if args.full and fmt == "coo" and world == 1:
        # what ran above: the matrix's plan found the entries sorted, built the row offsets they imply and multiplies with the CSR
        # kernel on them (the row indices are not read: 12 instead of 16 bytes per entry) -- `roofline` prices it on COO's 16.
        # Beside it: the COO format's own kernel for sorted entries (coo_tile: reads the row indices, no plan-owned memory).
        cfg = Afmt.plan().config()
        tcfg = cmi.Config(kernel=cmi.COO_TILE, nontemporal=3, xcd_swizzle=32)
        run_tile = lambda: cmi.spmv_coo(local_rows, N_global, Afmt.row_indices, Afmt.column_indices, Afmt.values, x, y, cfg=tcfg)  # noqa: E731
        for _ in range(20):
            run_tile()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * KERNEL_BATCHES)]
        for bi in range(KERNEL_BATCHES):
            ev[2 * bi].record()
            for _ in range(per_batch):
                run_tile()
            ev[2 * bi + 1].record()
        torch.cuda.synchronize()
        bt = [ev[2 * bi].elapsed_time(ev[2 * bi + 1]) / per_batch for bi in range(KERNEL_BATCHES)]
        mt = sum(bt) / len(bt)
        coo_tile = {"kernel_avg_ms": round(mt, 6), "kernel_min_ms": round(min(bt), 6), "algorithmic_bytes_per_launch": coo_bytes_,
                    "achieved_gbps": round(coo_bytes_ / (mt * 1e-3) / 1e9, 2),
                    "frac": round(coo_bytes_ / (mt * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4), "traffic": pmc_traffic("coo_tile")[0],
                    "kernel_config": tcfg.as_dict()}
        cmi.multiply(Afmt, x, y)

    if rank == 0:
        line = {
            "metric": "spmv_gflops_fp64_poisson5pt",
            "value": round(gflops, 3),
            "unit": "GFLOP/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 5),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic" if not rehearsal else "synthetic (REHEARSAL: ranks share one GPU over gloo; not a measurement)",
            "hbm_gbps": round(alg_bytes * world / (elapsed / args.steps) / 1e9, 2),
            "config": {"workload": f"poisson5pt {m}x{n} {fmt.upper()} int32/f64, y = A*x "
                                   f"({N_global} rows, {nnz_global} entries; {M}x{M} grid points per GPU)",
                       "format": fmt, **({"hyb_ell_width": HYB_WIDTH, "hyb_coo_entries": Afmt.coo.num_entries} if fmt == "hyb" else {}),
                       "rows_per_gpu": local_rows, "entries_per_gpu": local_nnz,
                       "kernel_config": cfg.as_dict(), "parallelism": f"row-block x{world}",
                       "x_exchange": exchange_info},
            "settle_launches": SETTLE,
        }
        if world == 1:
            line["kernel_launch_ledger"] = ledger  # (phase, launches of the hot path's kernel) in launch order; later legs (CG, opt-in plans) follow
        if args.full:
            line["roofline"] = {"bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                "frac": round(achieved / HBM_PEAK_GBPS, 4), "traffic": traffic,
                                "traffic_source": None if traffic is None else f"{traffic_src}: committed rocprofv3 --pmc summary of this kernel on this matrix and config (separate passes, FETCH_SIZE x2 correction); not collected in this run",
                                "kernel_avg_ms": round(kernel_ms, 6), "kernel_median_ms": round(kernel_ms_median, 6),
                                "kernel_min_ms": round(kernel_ms_min, 6),
                                "kernel_timing": f"{KERNEL_BATCHES} batches x {per_batch} launches, one HIP event pair per batch on the launch stream",
                                "kernel_avg_over_ms_per_step": round(kernel_ms / ms_per_step, 4),
                                # the dominant kernel cannot take longer than the step that contains it: checked, not assumed
                                "kernel_avg_le_step_x1.02": bool(kernel_ms <= ms_per_step * 1.02),
                                "algorithmic_bytes_per_launch": alg_bytes,
                                "kernel_gflops": round(2.0 * local_nnz / (kernel_ms * 1e-3) / 1e9, 2)}
            line["roofline"]["protocol"] = ("replay: one (A, x, y) multiplied back to back (the reference's protocol); x and part of the streams are served "
                                            "from the 256 MiB Infinity Cache between launches -- see roofline_cold for the all-from-HBM figure")
        if cold is not None:
            if "error" in cold:
                line["roofline_cold"] = cold
            else:
                ca = alg_bytes / (cold["kernel_avg_ms"] * 1e-3) / 1e9
                line["roofline_cold"] = {"bound": "hbm", "achieved": round(ca, 2), "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(ca / HBM_PEAK_GBPS, 4),
                                         "kernel_avg_ms": round(cold["kernel_avg_ms"], 6), "kernel_median_ms": round(cold["kernel_median_ms"], 6),
                                         "kernel_min_ms": round(cold["kernel_min_ms"], 6), "algorithmic_bytes_per_launch": alg_bytes,
                                         "kernel_gflops": round(2.0 * local_nnz / (cold["kernel_avg_ms"] * 1e-3) / 1e9, 2),
                                         "protocol": f"{cold['sets']} distinct (A, x, y) sets at different addresses visited round-robin ({cold['launches']} launches in "
                                                     f"{KERNEL_BATCHES} event-bracketed batches): {cold['sets'] - 1} other sets stream through the caches between two uses of a line",
                                         "results_identical_across_sets": cold["results_identical_across_sets"]}
        if exchanges is not None:
            for v in exchanges.values():
                if "error" not in v:
                    v["spmv_only_ms"] = round(kernel_ms, 6)
            line["exchanges"] = exchanges
        if configs4 is not None:
            line["configs4"] = configs4
        if cg_leg is not None:
            line["cg"] = cg_leg
        if c16 is not None:
            line["compressed_index_plan"] = c16
        if packed is not None:
            line["packed_tile_plan"] = packed
        if coo_tile is not None:
            line["coo_tile_kernel"] = coo_tile
            line["roofline"]["note"] = ("sorted COO through its plan = the CSR kernel on plan-built row offsets (built once, 4 bytes per row owned by the plan); "
                                        "priced on the bytes that kernel moves (12 per entry + 20 per row); the COO arrays hold 16 per entry: coo_tile_kernel "
                                        "is the format's own kernel reading them")
            line["roofline"]["coo_algorithmic_bytes_per_launch"] = coo_bytes_
        if args.full and world == 1 and not args.no_cpu_baseline and fmt == "csr":
            base, omp = cpu_baseline(cmi, A, x_host, y.cpu().numpy(), args.cpu_seconds)
            line["cpu_baseline"] = base
            line["cpu_baseline_omp"] = omp
        if args.full and not line["roofline"]["kernel_avg_le_step_x1.02"]:
            print(f"bench.py: WARNING kernel_avg_ms {kernel_ms:.6f} > 1.02 x ms_per_step {ms_per_step:.6f}: the {args.steps} timed steps ran faster "
                  "than the kernel's average over the 200+ launches behind them (clock / placement drift between the two timed regions)", file=sys.stderr, flush=True)
        print(json.dumps(line), flush=True)
    if dist is not None:
        sh.vec.close()  # barrier + unmap the peers' buffers before anyone frees them
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

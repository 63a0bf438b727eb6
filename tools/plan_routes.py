#!/usr/bin/env python3
"""The decision table of plan creation: which kernel, launch shape and plan-owned arrays every kind of matrix and request gets.

    python tools/plan_routes.py --record tests/golden/plan_routes.json    # writes the table + the commit it was recorded at
    python tools/plan_routes.py --matrix NAME                             # prints one matrix's rows (JSON)
    python tools/plan_routes.py --env-child NAME                          # (used by --record and the test) one environment setting's rows

A case is a matrix recipe plus plan requests (constructor, value type, Config or none).  Matrices are generated on the device: row
lengths from a hash of the row number, columns `row + (j - len / 2) * spread + offset` clipped to the matrix (or `row + offsets[j]` for
stencil rows) -- `spread` sets the share of entries 16+ columns from their predecessor, `spread * len` the share within 1536 columns of
the diagonal, the two quantities the rules of csrc/plan.hip read.  Sizes sit on either side of the rules' gates (4096 rows, 200 000 rows,
4 M / 8 M entries, 0.75 x and 1.25 x 256 MiB of index + value stream, the table's waver_rule.min_entries).  Nothing is multiplied.

tests/test_plan_routes_gpu.py compares a build against tests/golden/plan_routes.json field by field.  The golden file is re-recorded
only by a change that MEANS to alter a rule; a refactor of plan creation leaves it alone.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

F64, F32 = "f64", "f32"


class Matrix:
    def __init__(self, rows, cols, Ap, Aj):
        self.rows, self.cols, self.Ap, self.Aj = rows, cols, Ap, Aj
        self.nnz = int(Aj.numel())

    def values(self, dtype):
        import torch
        return torch.ones(self.nnz, dtype=dtype, device=self.Aj.device)

    def row_indices(self):
        import torch
        lens = (self.Ap[1:] - self.Ap[:-1]).to(torch.int64)
        return torch.repeat_interleave(torch.arange(self.rows, dtype=torch.int64, device=self.Ap.device), lens).to(torch.int32)


# ---- generators (device) ------------------------------------------------------------------------------------------------------------
def _assemble(lens, cols, col_of):
    import torch
    rows, dev = lens.numel(), lens.device
    Ap = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
    if rows:
        Ap[1:] = torch.cumsum(lens, 0)
    nnz = int(Ap[-1]) if rows else 0
    row = torch.repeat_interleave(torch.arange(rows, dtype=torch.int64, device=dev), lens)
    j = torch.arange(nnz, dtype=torch.int64, device=dev) - Ap[row]
    col = col_of(row, j, lens[row]).clamp_(0, max(cols - 1, 0))
    return Matrix(rows, cols, Ap.to(torch.int32), col.to(torch.int32))


def band(rows, lo, hi, spread, offset=0, long_rows=(), cols=None):
    """rows of lo..hi entries (a hash of the row number; lo == hi: equal rows), columns row + (j - len / 2) * spread + offset, clipped"""
    import torch
    i = torch.arange(rows, dtype=torch.int64, device="cuda")
    lens = lo + ((i * 2654435761) >> 11) % (hi - lo + 1)
    for r, n in long_rows:
        lens[r] = n
    return _assemble(lens, cols or rows, lambda row, j, ln: row + (j - ln // 2) * spread + offset)


def stencil(rows, offsets):
    """equal rows: columns row + offsets[j], clipped at the matrix's ends"""
    import torch
    off = torch.tensor(offsets, dtype=torch.int64, device="cuda")
    lens = torch.full((rows,), len(offsets), dtype=torch.int64, device="cuda")
    return _assemble(lens, rows, lambda row, j, ln: row + off[j])


def nine_point(n):
    return stencil(n * n, [-n - 1, -n, -n + 1, -1, 0, 1, n - 1, n, n + 1])


def poisson(n):
    import cusp_autotuned_amd as cmi
    A = cmi.poisson5pt(n, n, "csr", device="cuda")
    return Matrix(A.num_rows, A.num_cols, A.row_offsets, A.column_indices)


def dof2(n, points):
    """a 5- / 9-point stencil on an n x n grid with 2 degrees of freedom per point (tools/autotune.py: dense 2 x 2 blocks)"""
    import numpy as np
    import torch
    import autotune as at
    pts = at.stencil_points(9) if points == 9 else [(0, -1, 0, -1.0), (-1, 0, 0, -1.0), (0, 0, 0, 4.0), (1, 0, 0, -1.0), (0, 1, 0, -1.0)]
    Ap, Aj, Ax = at.stencil_csr(n, n, 1, pts, np.float32)
    Ap, Aj, _ = at.block_expand(Ap, Aj, Ax, 2, np.float32)
    return Matrix(len(Ap) - 1, len(Ap) - 1, torch.from_numpy(Ap).cuda(), torch.from_numpy(Aj).cuda())


def thermal2_like(scale):
    import numpy as np
    import torch
    import suitesparse_like as ssl
    Ap, Aj, _ = ssl.GENERATORS["thermal2"](scale)
    return Matrix(len(Ap) - 1, len(Ap) - 1, torch.from_numpy(np.ascontiguousarray(Ap, np.int32)).cuda(), torch.from_numpy(np.ascontiguousarray(Aj, np.int32)).cuda())


def poisson_synthetic(rows, mean):
    """Poisson row lengths, columns anywhere within +-2000 of the diagonal (tools/autotune.py synthetic_csr)"""
    import numpy as np
    import torch
    import autotune as at
    Ap, Aj, _ = at.synthetic_csr(rows, rows, mean, 5, np.float32)
    return Matrix(rows, rows, torch.from_numpy(Ap).cuda(), torch.from_numpy(Aj).cuda())


def empty_rows(rows):
    import torch
    return Matrix(rows, max(rows, 1), torch.zeros(rows + 1, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"))


MATRICES = {
    # AUTO plans
    "skew_tail": lambda: band(100000, 4, 4, 1, long_rows=[(777, 20000)]),            # one row of 20 000: balanced
    "long_row": lambda: band(100000, 4, 4, 1, long_rows=[(777, 600)]),               # a row of 512+ entries
    "nine_point_900": lambda: nine_point(900),                                       # 7.3 M entries: over min_entries, f64 and f32
    "nine_point_650": lambda: nine_point(650),                                       # 3.8 M: under it
    "poisson_3162": lambda: poisson(3162),                                           # the benchmark's matrix (beyond the cache)
    "poisson_2900": lambda: poisson(2900),                                           # 42.0 M entries: f32 just over 1.25 x the cache
    "poisson_2370": lambda: poisson(2370),                                           # 28.1 M: f64 just over 1.25 x the cache
    "poisson_2360": lambda: poisson(2360),                                           # 27.8 M: f64 just under
    "poisson_1000": lambda: poisson(1000),                                           # inside the cache
    "far_five": lambda: stencil(5800000, [-40000, -1, 0, 1, 40000]),                 # a tile spans more than 65535 columns
    "far_five_small": lambda: stencil(200000, [-40000, -1, 0, 1, 40000]),
    "tridiagonal": lambda: stencil(10000000, [-1, 0, 1]),                            # rows of 3 beyond the cache
    "rows_of_10": lambda: band(2900000, 10, 10, 2),                                  # rows of 10 beyond the cache, no column runs
    "equal6_band": lambda: band(5000000, 6, 6, 600),                                 # equal rows of 6, columns anywhere in +-2000
    "dof2_five_472": lambda: dof2(472, 5),                                           # 4.45 M entries: just over the f64 min_entries
    "dof2_five_466": lambda: dof2(466, 5),                                           # 4.34 M: just under
    "dof2_nine_450": lambda: dof2(450, 9),                                           # 18 per row, 7.3 M: V = 4
    "dof2_nine_340": lambda: dof2(340, 9),                                           # 4.2 M: under min_entries, not stencil-like
    "no_runs": lambda: band(450000, 10, 10, 2),                                      # 4.5 M entries, pieces of 1: the copy is dropped
    "fem20": lambda: band(1400000, 10, 30, 2),                                       # 28 M entries, 20 per row, columns share x lines
    "band20": lambda: band(1300000, 20, 20, 150),                                    # 26 M, columns anywhere in +-1500
    "scattered": lambda: band(3800000, 3, 11, 5000, offset=2500),                    # no entry within 1536 columns of the diagonal
    "scattered_small": lambda: band(300000, 3, 11, 20000, offset=10000),             # a tile of rows spans more than 65535 columns
    "short7": lambda: band(3700000, 5, 9, 1),                                        # 25.9 M entries, 7 per row: f32 over 0.75 x the cache
    "short7_long": lambda: band(3700000, 5, 9, 1, long_rows=[(1000, 300), (2000000, 300), (3600000, 300)]),
    "short7_2500k": lambda: band(2500000, 5, 9, 1),                                  # 17.5 M: f64 just over 0.75 x the cache
    "short7_2300k": lambda: band(2300000, 5, 9, 1),                                  # 16.1 M: f64 just under
    "short7_250k": lambda: band(250000, 5, 9, 1),                                    # short_f64_rows: over 200 000 rows
    "short7_190k": lambda: band(190000, 5, 9, 1),                                    # ... and under
    "thermal2_like": lambda: thermal2_like(0.3),
    "band6_1400k": lambda: band(1400000, 3, 9, 500),                                 # band_candidate: 8.4 M entries
    "band6_1300k": lambda: band(1300000, 3, 9, 500),                                 # 7.8 M: f64 under, f32 over
    "band6_650k": lambda: band(650000, 3, 9, 500),                                   # 3.9 M: f32 under
    "poisson_rows_16": lambda: poisson_synthetic(600000, 16.0),                      # 9.6 M entries, Poisson(16) lengths, +-2000
    "no_rows": lambda: empty_rows(0),
    "no_entries": lambda: empty_rows(10),
    # asked-for kernels and the environment switches' small matrices
    "irregular": lambda: band(20000, 2, 8, 1),
    "irregular_4000": lambda: band(4000, 2, 8, 1),
    "irregular_4200": lambda: band(4200, 2, 8, 1),
    "irregular_row200": lambda: band(20000, 2, 8, 1, long_rows=[(5000, 200)]),
    "poisson_300": lambda: poisson(300),
    "three_columns": lambda: band(3, 2, 2, 1),
}


# ---- requests -----------------------------------------------------------------------------------------------------------------------
def req(ctor, dtype, **cfg):
    return (ctor, dtype, cfg or None)


def auto4():
    return [req("plan", F64), req("plan", F32), req("csr", F64), req("csr", F32)]


def _asked():
    import cusp_autotuned_amd as cmi
    K = cmi
    out = []
    # CSR_STREAM_WAVE on a plan-built partition
    out += [req("plan", F64, kernel=K.CSR_STREAM_WAVE, rows_per_block=-1), req("plan", F32, kernel=K.CSR_STREAM_WAVE, rows_per_block=-1, items_per_thread=4),
            req("csr", F64, kernel=K.CSR_STREAM_WAVE, rows_per_block=-1, nontemporal=1), req("plan", F64, kernel=K.CSR_STREAM_WAVE, rows_per_block=-1, items_per_thread=1)]
    # CSR_STREAM_WAVEV
    for v in (0, 1, 2, 4):
        out.append(req("plan", F64, kernel=K.CSR_STREAM_WAVEV, items_per_thread=v))
    out += [req("plan", F32, kernel=K.CSR_STREAM_WAVEV, items_per_thread=2, nontemporal=1), req("plan", F64, kernel=K.CSR_STREAM_WAVEV, nontemporal=3),
            req("plan", F64, kernel=K.CSR_STREAM_WAVEV, xcd_swizzle=-1), req("plan", F64, kernel=K.CSR_STREAM_WAVEV, xcd_swizzle=8),
            req("csr", F64, kernel=K.CSR_STREAM_WAVEV, items_per_thread=1, nontemporal=3 | K.POLICY_COLS16),
            req("csr", F32, kernel=K.CSR_STREAM_WAVEV, items_per_thread=2, nontemporal=K.POLICY_COLS16),
            req("plan", F64, kernel=K.CSR_STREAM_WAVEV, items_per_thread=1, nontemporal=3 | K.POLICY_COLS16), req("plan", F64, kernel=K.CSR_STREAM_WAVEV, items_per_thread=3)]
    # CSR_STREAM_WAVEX
    out += [req("plan", F64, kernel=K.CSR_STREAM_WAVEX), req("csr", F32, kernel=K.CSR_STREAM_WAVEX, rows_per_block=2048, items_per_thread=1),
            req("plan", F64, kernel=K.CSR_STREAM_WAVEX, rows_per_block=4096, items_per_thread=2, nontemporal=2, xcd_swizzle=4)]
    # CSR_STREAM_WAVER / _PACKED
    out += [req("csr", F64, kernel=K.CSR_STREAM_WAVER), req("csr", F32, kernel=K.CSR_STREAM_WAVER, threads_per_row=3), req("csr", F64, kernel=K.CSR_STREAM_WAVER, items_per_thread=1, threads_per_row=4),
            req("csr", F64, kernel=K.CSR_STREAM_WAVER, nontemporal=1, xcd_swizzle=-1), req("csr", F64, kernel=K.CSR_STREAM_WAVER, xcd_swizzle=8),
            req("csr_values", F64, kernel=K.CSR_STREAM_PACKED), req("csr_values", F32, kernel=K.CSR_STREAM_PACKED, threads_per_row=3, nontemporal=2),
            req("csr_values", F64, kernel=K.CSR_STREAM_WAVER), req("csr", F64, kernel=K.CSR_STREAM_PACKED), req("plan", F64, kernel=K.CSR_STREAM_WAVER)]
    # CSR_STREAM_C16 and the kernels for which nothing is built
    out += [req("csr", F64, kernel=K.CSR_STREAM_C16), req("csr", F32, kernel=K.CSR_STREAM_C16, block_size=256, rows_per_block=128, items_per_thread=2), req("plan", F64, kernel=K.CSR_STREAM_C16),
            req("plan", F64, kernel=K.CSR_STREAM), req("csr", F32, kernel=K.CSR_STREAM, block_size=256, rows_per_block=64, items_per_thread=2),
            req("plan", F64, kernel=K.CSR_SCALAR), req("csr", F64, kernel=K.CSR_VECTOR, threads_per_row=8), req("plan", F32, kernel=K.CSR_STREAM_PIPE)]
    return out


def requests_of(name):
    import cusp_autotuned_amd as cmi
    K = cmi
    if name in ("irregular", "poisson_300"):
        extra = [req("coo", F64), req("coo_offsets", F64), req("coo_unsorted", F64), req("coo_offsets_unsorted", F32), req("coo", F32, kernel=K.COO_TILE), req("coo_unsorted", F64, kernel=K.COO_TILE)] if name == "poisson_300" else []
        return auto4() + _asked() + extra
    if name == "irregular_row200":
        return auto4() + [req("plan", F64, kernel=K.CSR_STREAM_WAVEV, items_per_thread=1), req("plan", F64, kernel=K.CSR_STREAM_WAVEV), req("plan", F64, kernel=K.CSR_STREAM_WAVEX),
                          req("csr", F64, kernel=K.CSR_STREAM_WAVER, items_per_thread=1), req("csr", F64, kernel=K.CSR_STREAM_WAVER), req("plan", F64, kernel=K.CSR_STREAM_WAVE, rows_per_block=-1)]
    if name == "long_row":
        return auto4() + [req("plan", F64, kernel=K.CSR_STREAM_WAVEV), req("csr", F64, kernel=K.CSR_STREAM_WAVER), req("plan", F64, kernel=K.CSR_STREAM_WAVE, rows_per_block=-1)]
    if name == "three_columns":
        return auto4() + [req("csr", F32, kernel=K.CSR_STREAM_WAVER), req("csr", F64, kernel=K.CSR_STREAM_WAVER), req("csr_values", F32, kernel=K.CSR_STREAM_PACKED)]
    if name in ("poisson_1000", "far_five_small", "short7_250k", "scattered_small"):  # the process-wide index-compression default, off and on
        more = {"poisson_1000": [req("csr_values", F64, kernel=K.CSR_STREAM_PACKED)],
                "far_five_small": [req("csr", F64, kernel=K.CSR_STREAM_WAVEV, items_per_thread=1, nontemporal=3 | K.POLICY_COLS16), req("csr", F64, kernel=K.CSR_STREAM_C16),
                                   req("csr_values", F64, kernel=K.CSR_STREAM_PACKED)]}
        return auto4() + [req("csr", F64, compress=1), req("csr", F32, compress=1), req("plan", F64, compress=1)] + more.get(name, [])
    if name == "poisson_3162":
        return auto4() + [req("csr", F64, compress=1), req("coo", F64), req("csr", F64, kernel=K.CSR_STREAM_WAVEV, items_per_thread=1, nontemporal=3 | K.POLICY_COLS16), req("csr", F64, kernel=K.CSR_STREAM_C16)]
    if name == "no_entries":
        return auto4() + [req("bad_offsets", F64), req("plan", F64, kernel=K.CSR_STREAM_WAVEV), req("csr", F64, kernel=K.CSR_STREAM_WAVER)]
    if name == "nine_point_900":
        return auto4() + [req("coo", F64)]
    return auto4()


def label(r):
    ctor, dtype, cfg = r
    return ctor + ":" + dtype + (":" + ",".join(f"{k}={v}" for k, v in cfg.items()) if cfg else "")


def observe(M, r):
    """one row of the table: status (+ the error's text), else config, info, device bytes, marked shift tiles"""
    import torch
    import cusp_autotuned_amd as cmi
    ctor, dtype, cfg = r
    cfg = dict(cfg or {})
    compress = cfg.pop("compress", 0)
    tdt = torch.float64 if dtype == F64 else torch.float32
    c = cmi.Config(**cfg) if cfg else None
    cmi.set_index_compression(bool(compress))
    try:
        if ctor == "plan":
            p = cmi.Plan(cmi.FORMAT_CSR, tdt, M.rows, M.cols, M.nnz, M.Ap, c)
        elif ctor == "bad_offsets":  # the row offsets do not end at num_entries
            p = cmi.Plan(cmi.FORMAT_CSR, tdt, M.rows, M.cols, M.nnz + 7, M.Ap, c)
        elif ctor == "csr":
            p = cmi.Plan.csr(tdt, M.rows, M.cols, M.Ap, M.Aj, cfg=c)
        elif ctor == "csr_values":
            p = cmi.Plan.csr_values(M.rows, M.cols, M.Ap, M.Aj, M.values(tdt), cfg=c)
        elif ctor in ("coo", "coo_offsets", "coo_unsorted", "coo_offsets_unsorted"):
            Ai = M.row_indices()
            if ctor.endswith("unsorted"):
                Ai = torch.flip(Ai, [0]).contiguous()
            p = cmi.Plan.coo(tdt, M.rows, M.cols, Ai, M.Aj, cfg=c) if ctor in ("coo", "coo_unsorted") else cmi.Plan(cmi.FORMAT_COO, tdt, M.rows, M.cols, M.nnz, Ai, c)
        else:
            raise ValueError(ctor)
    except cmi.CmiError as e:
        return {"status": int(e.status), "error": str(e)}
    finally:
        cmi.set_index_compression(False)
    return {"status": 0, "config": p.config().as_dict(), "info": p.info(), "device_bytes": int(p.device_bytes()), "shifted_tiles": int(p.shifted_tiles())}


def run_matrix(name, requests=None):
    import torch
    M = MATRICES[name]()
    out = {label(r): observe(M, r) for r in (requests or requests_of(name))}
    del M
    torch.cuda.empty_cache()
    return out


# ---- environment switches: read once per process, so one child process per setting, one after the other --------------------------------
ENV_SETTINGS = {
    "CMI_CSR_WAVE=0": ["poisson_1000", "nine_point_650", "irregular"],
    "CMI_CSR_WAVE=2": ["irregular", "irregular_4000", "irregular_4200", "poisson_1000"],   # the only way into the plan-built csr_wave for AUTO plans
    "CMI_CSR_WAVEV=0": ["short7_250k", "short7_2500k", "band6_1400k"],
    "CMI_CSR_WAVEV=1": ["irregular", "irregular_4000", "irregular_4200", "short7_250k"],
    "CMI_CSR_WAVER=0": ["nine_point_900", "dof2_five_472", "irregular"],
    "CMI_CSR_WAVER=1": ["dof2_five_466", "irregular", "irregular_4000", "irregular_4200"],
    "CMI_CSR_WAVE_VEC=0": ["poisson_2370", "poisson_1000", "irregular"],
    "CMI_CSR_WAVEX=0": ["band20", "poisson_1000", "irregular"],
    "CMI_COO_PLAN_OFFSETS=0": ["poisson_300", "irregular", "poisson_1000"],
}


def env_requests(setting, name):
    return auto4() + ([req("coo", F64), req("coo_offsets", F32)] if setting.startswith("CMI_COO") else [])


def env_child(setting):
    """(in the child) the rows of one setting"""
    key, value = setting.split("=")
    assert os.environ.get(key) == value, "start this through run_env_child"
    return {name: run_matrix(name, env_requests(setting, name)) for name in ENV_SETTINGS[setting]}


class ChildDied(RuntimeError):
    """the child was ended by a signal or a time limit: whoever started it starts nothing further on the GPU"""


def run_env_child(setting, timeout=300):
    """a fresh process with the setting in its environment; raises when the child fails or runs out of time"""
    key, value = setting.split("=")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--env-child", setting], env=dict(os.environ, **{key: value}), capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        raise ChildDied(f"{setting}: child ended with {r.returncode}\n{r.stderr[-2000:]}")
    if r.returncode != 0:
        raise RuntimeError(f"{setting}: child exited with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def commit_hash():
    r = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
    return r.stdout.strip() if r.returncode == 0 and r.stdout.strip() else os.environ.get("CMI_RECORD_COMMIT", "unknown")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record")
    ap.add_argument("--commit", help="the commit the build under test was made from (default: git rev-parse HEAD)")
    ap.add_argument("--matrix")
    ap.add_argument("--env-child")
    args = ap.parse_args()
    if args.env_child:
        print(json.dumps(env_child(args.env_child)))
        return
    if args.matrix:
        print(json.dumps(run_matrix(args.matrix), indent=1))
        return
    if not args.record:
        ap.error("one of --record, --matrix, --env-child")
    table = {"recorded_at_commit": args.commit or commit_hash(), "matrices": {}, "environment": {}}
    for name in MATRICES:
        table["matrices"][name] = run_matrix(name)
        print(name, "ok", flush=True)
    for setting in ENV_SETTINGS:  # one after the other; a child that fails ends the recording
        table["environment"][setting] = run_env_child(setting)
        print(setting, "ok", flush=True)
    with open(args.record, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

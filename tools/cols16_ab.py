#!/usr/bin/env python3
"""csr_wavev with the caller's 32-bit columns against the plan's 16-bit column copy (cfg.nontemporal bit 8): the A/B that the AUTO rule's
use of the copy rests on.  One process, two explicit plans per matrix (nontemporal 3 and 11, the rule's V), interleaved round-robin:

    replay   median of R rounds x L launches of the multiply on one (A, x, y)
    cold     the same over 4 copies of (A, x, y) in rotation (nothing comes from the Infinity Cache)
    dot      the multiply with the fused <y, x> (the CG instance), replayed

and per figure the larger of the two variants' max - min over the rounds (the round spread a difference has to clear).

    python3 tools/cols16_ab.py [--matrices 5pt,7pt,5pt32,7pt32,rank] [--rounds 5]

`rank`: configs[4]'s per-rank block, rows [0, 1.25e7) of poisson5pt(10000, 10000) with global columns and an x of 1e8 entries."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import cusp_autotuned_amd as cmi  # noqa: E402
import stencil_tiles_probe as stp  # noqa: E402


def matrix_sets(key, copies):
    """[(Ap, Aj, Ax, x, y)] x copies on the device, columns of x, the value type, a title."""
    if key == "rank":
        g, rows = 10000, 12_500_000
        sets = []
        for _ in range(copies):
            A = cmi.poisson5pt(g, g, "csr", dtype=torch.float64, device="cuda", row_begin=0, row_end=rows)
            sets.append((A.row_offsets, A.column_indices, A.values, cmi.fill_x(g * g, torch.float64, "cuda"), torch.empty(rows, dtype=torch.float64, device="cuda")))
        return sets, g * g, torch.float64, "configs[4] rank block: rows [0, 1.25e7) of poisson5pt(10000, 10000) f64, x of 1e8"
    name, build, dt = stp.MATS[key]
    Ap, Aj, Ax = build()
    rows = len(Ap) - 1
    sets = [(torch.from_numpy(Ap).cuda(), torch.from_numpy(Aj).cuda(), torch.from_numpy(Ax).cuda().to(dt), cmi.fill_x(rows, dt, "cuda"), torch.empty(rows, dtype=dt, device="cuda"))
            for _ in range(copies)]
    return sets, rows, dt, name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="5pt,7pt,5pt32,7pt32,rank")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40)
    args = ap.parse_args()
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for key in args.matrices.split(","):
        sets, cols, dt, name = matrix_sets(key, 2 if key == "rank" else 4)
        dAp, dAj, dAx, x, y = sets[0]
        rows, nnz = y.numel(), dAj.numel()
        V = 1 if dt == torch.float64 else 2
        cmi.spmv_csr(rows, cols, dAp, dAj, dAx, x, y, cfg=cmi.Config(kernel=cmi.CSR_SCALAR))
        want = y.clone()
        alg = cmi.csr_bytes(rows, nnz, 8 if dt == torch.float64 else 4)
        print(f"# {name}: rows {rows} entries {nnz} V = {V}; algorithmic bytes {alg / 1e6:.1f} MB (32-bit columns), {(alg - 2 * nnz) / 1e6:.1f} MB (16-bit copy)", flush=True)
        plans = {}
        for label, pol in (("32-bit columns", 3), ("16-bit copy", 3 | cmi.POLICY_COLS16)):
            p = cmi.Plan.csr(dt, rows, cols, dAp, dAj, cfg=cmi.Config(kernel=cmi.CSR_STREAM_WAVEV, items_per_thread=V, nontemporal=pol))
            c = p.config()
            if c.nontemporal != pol:  # some tile spans more than 65535 columns: nothing to compare
                print(f"  the copy is REFUSED (a wave tile spans more than 65535 columns): the plan reports nontemporal {c.nontemporal} and runs the 32-bit kernel", flush=True)
                break
            assert (c.kernel, c.items_per_thread) == (cmi.CSR_STREAM_WAVEV, V), (label, c.kernel, c.items_per_thread)
            y.fill_(float("nan"))
            cmi.spmv_csr_plan(p, dAp, dAj, dAx, x, y)
            assert torch.equal(y, want), label
            plans[label] = p
        auto = cmi.Plan.csr(dt, rows, cols, dAp, dAj).config()
        if len(plans) < 2:
            print(f"  [the AUTO plan of this tree: kernel {auto.kernel} V {auto.items_per_thread} nontemporal {auto.nontemporal}]", flush=True)
            del sets, plans, dAp, dAj, dAx, x, y, want
            torch.cuda.empty_cache()
            continue
        res = torch.zeros(1, dtype=torch.float64, device="cuda")
        ws = cmi.blas_workspace()
        n = len(sets)
        out = {label: {"replay": [], "cold": [], "dot": []} for label in plans}
        for _ in range(args.rounds):
            for label, p in plans.items():
                go = lambda i, p=p: cmi.spmv_csr_plan(p, dAp, dAj, dAx, x, y)  # noqa: E731
                stp.settle(go)
                out[label]["replay"].append(stp.group_us(go, args.launches))
                gc = lambda i, p=p: cmi.spmv_csr_plan(p, *sets[i % n])  # noqa: E731
                stp.settle(gc)
                out[label]["cold"].append(stp.group_us(gc, args.launches))
                gd = lambda i, p=p: cmi.spmv_csr_dot(rows, cols, dAp, dAj, dAx, x, y, x[:rows], res, ws, plan=p)  # noqa: E731
                stp.settle(gd)
                out[label]["dot"].append(stp.group_us(gd, args.launches))
        for label in plans:
            o = out[label]
            print(f"  {label:15s} replay {med(o['replay']):7.1f} us (rounds {' '.join(f'{v:.1f}' for v in o['replay'])})  cold {med(o['cold']):7.1f} us (rounds {' '.join(f'{v:.1f}' for v in o['cold'])})  "
                  f"with the fused dot {med(o['dot']):7.1f} us (rounds {' '.join(f'{v:.1f}' for v in o['dot'])})  plan owns {plans[label].device_bytes() / 1e6:.1f} MB", flush=True)
        a, b = out["32-bit columns"], out["16-bit copy"]
        print("  16-bit / 32-bit: " + "  ".join(f"{k} {med(b[k]) / med(a[k]):.3f} ({med(b[k]) - med(a[k]):+.1f} us; round spread {max(max(a[k]) - min(a[k]), max(b[k]) - min(b[k])):.1f})" for k in ("replay", "cold", "dot"))
              + f"   [the AUTO plan of this tree: kernel {auto.kernel} V {auto.items_per_thread} nontemporal {auto.nontemporal}]", flush=True)
        del sets, plans, dAp, dAj, dAx, x, y, want
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

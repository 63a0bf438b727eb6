"""GPU test (-m gpu) of the N>1 path with the REAL local multiply: two ranks share the one GPU of the
box (gloo as the transport -- RCCL refuses two ranks on one device), each owns a row block of
poisson5pt built in HBM with global column indices, exchanges x (halo and all-gather) and runs the
HIP SpMV on its block.  The concatenated y must equal the oracle's whole-matrix result bit for bit.
The 8-GPU RCCL run itself is the driver's (bench.py --gpus N)."""
import os
import socket

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, mode, m, n, out_dir):
    import sys
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import cusp_autotuned_amd as cmi
        N = m * n
        offs = cmi.distributed.partition_rows(N, world)
        lo, hi = offs[rank], offs[rank + 1]
        A = cmi.poisson5pt(m, n, "csr", row_begin=lo, row_end=hi)
        sh = cmi.distributed.ShardedCsr(A, N, rank, world, mode=mode)
        sh.x_local.copy_(cmi.fill_x(hi - lo, start=lo).cuda())
        y = torch.full((hi - lo,), 10.0, dtype=torch.float64, device="cuda")
        # the one-sided exchange needs the peers' writes of x ordered before the pull and the pull ordered
        # before their next write: fence() is that epoch boundary (a no-op requirement for the two-sided modes)
        sh.vec.fence()
        sh.multiply(y)
        sh.vec.fence()
        sh.x_local.mul_(-2.0)
        sh.vec.fence()
        y2 = torch.empty_like(y)
        sh.multiply(y2)
        torch.cuda.synchronize()
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), y=y.cpu().numpy(), y2=y2.cpu().numpy(), mode=sh.vec.plan.mode,
                 recv=sh.vec.plan.recv_values, interior=-1 if sh.interior is None else sh.interior[1] - sh.interior[0])
        sh.vec.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("mode,world", [("halo", 2), ("allgather", 2), ("peer", 2), ("peer", 3), ("peer", 4), ("auto", 2), ("halo", 3)])
def test_ranks_share_one_gpu_real_kernels(tmp_path, orc, mode, world):
    import oracle
    import torch.multiprocessing as mp
    m, n = 300, 201
    mp.spawn(_worker, args=(world, _free_port(), mode, m, n, str(tmp_path)), nprocs=world, join=True)
    Ap, Aj, Ax = orc.poisson5pt_csr(m, n)
    x = oracle.fill_x(m * n)
    parts = [np.load(tmp_path / f"r{r}.npz") for r in range(world)]
    assert np.array_equal(np.concatenate([p["y"] for p in parts]), orc.spmv_csr(Ap, Aj, Ax, x))
    assert np.array_equal(np.concatenate([p["y2"] for p in parts]), orc.spmv_csr(Ap, Aj, Ax, -2.0 * x))
    inner = [r for r in range(world) if 0 < r < world - 1]
    if mode == "halo":
        assert all(str(p["mode"]) == "halo" for p in parts) and all(int(p["interior"]) > 0 for p in parts)
    if mode in ("peer", "auto"):  # auto: the buffers are in HBM and the peers' buffers map -> one-sided
        assert all(str(p["mode"]) == "peer" and int(p["interior"]) == -1 for p in parts)
    if mode != "allgather":
        assert all(int(parts[r]["recv"]) == (2 * m if r in inner else m) for r in range(world))


def _worker_by_entries(rank, world, port, mode, out_dir):
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import torch.distributed as dist
    from test_distributed_cpu import _irregular
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import cusp_autotuned_amd as cmi
        N, Ap, Aj, Ax = _irregular()
        offs = cmi.distributed.partition_by_entries(Ap, world)
        lo, hi = offs[rank], offs[rank + 1]
        lAp = torch.from_numpy((Ap[lo:hi + 1] - Ap[lo]).astype(np.int32)).cuda()
        lAj = torch.from_numpy(Aj[Ap[lo]:Ap[hi]].copy()).cuda()
        lAx = torch.from_numpy(Ax[Ap[lo]:Ap[hi]].copy()).cuda()
        A = cmi.CsrMatrix(hi - lo, N, lAx.numel(), lAp, lAj, lAx)
        sh = cmi.distributed.ShardedCsr(A, N, rank, world, mode=mode, offsets=offs)
        sh.x_local.copy_(cmi.fill_x(hi - lo, start=lo).cuda())
        y = torch.empty(hi - lo, dtype=torch.float64, device="cuda")
        sh.vec.fence()
        sh.multiply(y)
        sh.vec.fence()
        sh.x_local.mul_(3.0)
        sh.vec.fence()
        y2 = torch.empty_like(y)
        sh.multiply(y2)
        torch.cuda.synchronize()
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), y=y.cpu().numpy(), y2=y2.cpu().numpy(), mode=sh.vec.plan.mode, rows=hi - lo)
        sh.vec.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["peer", "allgather", "halo"])
def test_unequal_row_blocks_balanced_by_entries(tmp_path, orc, mode):
    """Three ranks, row blocks of different lengths (equal entry counts) of a heavy-tailed matrix: every exchange
    reassembles x at its global positions; the all-gather pads and un-pads with cmi_copy_ranges."""
    import oracle
    import torch.multiprocessing as mp
    from test_distributed_cpu import _irregular
    world = 3
    mp.spawn(_worker_by_entries, args=(world, _free_port(), mode, str(tmp_path)), nprocs=world, join=True)
    N, Ap, Aj, Ax = _irregular()
    x = oracle.fill_x(N)
    parts = [np.load(tmp_path / f"r{r}.npz") for r in range(world)]
    assert len({int(p["rows"]) for p in parts}) > 1 and all(str(p["mode"]) == mode for p in parts)
    want, want2 = orc.spmv_csr(Ap, Aj, Ax, x), orc.spmv_csr(Ap, Aj, Ax, 3.0 * x)
    bound = orc.spmv_csr(Ap, Aj, np.abs(Ax), np.abs(x))
    got, got2 = np.concatenate([p["y"] for p in parts]), np.concatenate([p["y2"] for p in parts])
    assert np.all(np.abs(got - want) <= 1e-12 * bound + 1e-300) and np.all(np.abs(got2 - want2) <= 3e-12 * bound + 1e-300)


def test_bench_two_ranks_rehearsal(tmp_path):
    """bench.py --gpus 2 end to end on the one GPU of the box (CMI_BENCH_REHEARSAL=1: both ranks on GPU 0,
    gloo): launch line as the driver's, one JSON line from rank 0, one-sided exchange selected."""
    import json
    import subprocess
    import sys
    env = dict(os.environ, CMI_BENCH_REHEARSAL="1", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "5", "--warmup", "2",
           "--cg-iterations", "100", "--configs4", "on", "--configs4-grid", "400"]
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 5 and line["scaling"] == "weak" and line["value"] > 0
    assert line["config"]["x_exchange"]["mode"] == "peer"
    assert line["config"]["x_exchange"]["values_received_per_rank"] == 3162
    assert line["config"]["rows_per_gpu"] == 3162 * 3162 and "cpu_baseline" not in line
    cg = line["cg"]                  # the caller, sharded: one-sided scheme, recurrence residual == b - A x
    assert "error" not in cg and cg["iterations"] == 100 and cg["residual_consistent"] and cg["exchange"] == "peer"
    # the one-sided exchange was proven in a child process before the parents touched the GPU
    assert line["config"]["x_exchange"]["peer_probe_in_child_process"] == {"ok": True, "note": "ok"}
    # both exchanges are first-class: same steps, value + exchange alone + SpMV alone each
    ex = line["exchanges"]
    assert set(ex) == {"peer", "allgather"} and ex["peer"]["carries_value"] and ex["peer"]["value"] == line["value"]
    ag = ex["allgather"]             # the north-star's literal exchange, timed beside the default
    assert "error" not in ag and ag["y_identical_to_default_exchange"] and ag["values_received_per_rank"] == 3162 * 3162
    for v in ex.values():
        assert v["steps"] == 5 and v["value"] > 0 and v["exchange_only_ms"] > 0 and v["spmv_only_ms"] > 0
    # BASELINE.json configs[4]'s shape (shrunk: 400x400 over 2 ranks), SpMV with both exchanges + CG, each validated
    c4 = line["configs4"]
    assert "error" not in c4 and c4["rows_per_gpu"] == 200 * 400 and set(c4["exchanges"]) == {"peer", "allgather"}
    for v in c4["exchanges"].values():
        assert v["bit_exact_vs_stencil_closed_form"] and v["value"] > 0 and v["cg"]["residual_consistent"]


def test_bench_survives_a_failed_peer_probe(tmp_path):
    """The child-process probe of the one-sided exchange reports failure (CMI_BENCH_FAIL_PROBE pretends a child faulted):
    every rank agrees, the one-sided exchange is never attempted in the parents, the two-sided halo exchange carries value."""
    import json
    import subprocess
    import sys
    env = dict(os.environ, CMI_BENCH_REHEARSAL="1", MASTER_ADDR="127.0.0.1", CMI_BENCH_FAIL_PROBE="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--cg-iterations", "5"]
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    ex = line["config"]["x_exchange"]
    assert ex["mode"] == "halo" and ex["rejected_exchanges"] == [] and ex["peer_probe_in_child_process"]["ok"] is False
    assert set(line["exchanges"]) == {"halo", "allgather"} and line["cg"]["exchange"] == "halo" and line["cg"]["residual_consistent"]


def test_bench_hands_over_to_the_next_exchange_when_one_is_rejected(tmp_path):
    """bench.py validates the exchange against the stencil's closed form before timing; an exchange that fails is closed and
    the next one takes over on every rank (CMI_BENCH_REJECT pretends the one-sided pull failed): two-sided halo exchange."""
    import json
    import subprocess
    import sys
    env = dict(os.environ, CMI_BENCH_REHEARSAL="1", MASTER_ADDR="127.0.0.1", CMI_BENCH_REJECT="peer")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--cg-iterations", "5"]
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    ex = line["config"]["x_exchange"]
    probe = ex.get("peer_probe_in_child_process") or {}
    # (a box on which the child-process probe of the one-sided exchange did not succeed -- it timed out on a slow box in round 4 -- never
    #  offers "peer": then there is nothing to reject and the two-sided halo exchange is simply the first choice)
    assert ex["rejected_exchanges"] == (["peer"] if probe.get("ok", True) else []), (ex["rejected_exchanges"], probe)
    assert ex["mode"] == "halo" and ex["validated_against"].startswith("stencil")
    assert line["value"] > 0 and line["cg"]["residual_consistent"] and line["cg"]["exchange"] == "halo"
    assert line["exchanges"]["allgather"]["y_identical_to_default_exchange"] and line["exchanges"]["halo"]["carries_value"]

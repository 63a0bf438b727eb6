"""What a plan owns after the paths of plan creation that hand a device block over, drop one, or build nothing: cmi_plan_device_bytes is
the sum of the blocks the plan still holds, so a block that was dropped must not be counted and one that was kept must be.

Paths that already had such an assertion are not repeated here: the packed stencil plan's exact byte count
(test_round4_gpu.py::test_packed_wave_tiles_on_stencils), the granted / refused 16-bit copies (test_cols16_gpu.py, test_csr16_gpu.py,
test_shift_tiles_gpu.py) and every route's count in tests/golden/plan_routes.json (test_plan_routes_gpu.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = {"f64": 1e-6, "f32": 1e-5}  # test_spmv_gpu.py's bar for kernels that re-associate a row sum (two-launch HYB: its COO half)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch


def dev(a, torch):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_hyb_plan_that_drops_its_one_launch_attempt(cmi, torch_cuda, orc, tag):
    """2048 rows, ELL width 2, a sorted COO part of 4200 entries all in ONE row: light enough on average for the one-launch kernel (<= 3
    per row), so the per-tile ranges are built -- and dropped again, because one tile of 256 rows holds more than 4096 entries.  The plan
    then runs two launches and owns exactly what its COO sub-plan owns; the result is the host loops' within the two-launch bar."""
    torch = torch_cuda
    dtype, tdt = (np.float64, torch.float64) if tag == "f64" else (np.float32, torch.float32)
    rng = np.random.default_rng(5)
    rows, cols, width, heavy = 2048, 6000, 2, 777
    lens = np.full(rows, width)
    lens[heavy] += 4200
    Ap = np.r_[0, np.cumsum(lens)].astype(np.int32)
    Aj = np.concatenate([np.sort(rng.choice(cols, size=l, replace=False)) for l in lens]).astype(np.int32)
    Ax = rng.standard_normal(len(Aj)).astype(dtype)
    x = rng.standard_normal(cols).astype(dtype)
    p, hAj, hAx, cAi, cAj, cAx = orc.csr_to_hyb(Ap, Aj, Ax, width)
    assert len(cAi) == 4200 and (cAi == heavy).all() and len(cAi) <= 3.0 * rows
    d = [dev(a, torch) for a in (hAj, hAx, cAi, cAj, cAx)]
    plan = cmi.Plan.hyb(tdt, rows, cols, width, d[2])
    assert plan.info()["coo_sorted"] is True
    assert plan.hyb_launches() == 2
    coo_alone = cmi.Plan(cmi.FORMAT_COO, tdt, rows, cols, len(cAi), d[2])
    assert coo_alone.device_bytes() >= 4 * (rows + 1)  # (sorted: its row offsets at least)
    assert plan.device_bytes() == coo_alone.device_bytes(), (plan.device_bytes(), coo_alone.device_bytes())
    want = orc.spmv_hyb(rows, width, p, hAj, hAx, cAi, cAj, cAx, x)
    bound = orc.spmv_hyb(rows, width, p, hAj, np.abs(hAx), cAi, cAj, np.abs(cAx), np.abs(x))
    y = torch.full((rows,), 10.0, dtype=tdt, device="cuda")
    cmi.spmv_hyb_plan(plan, p, *d, dev(x, torch), y)
    err = np.abs(y.cpu().numpy().astype(np.float64) - want.astype(np.float64))
    assert np.all(err <= TOL[tag] * np.maximum(bound.astype(np.float64), np.finfo(dtype).tiny)), err.max()


def _waver_child():
    """Run as a script with CMI_CSR_WAVER=1 in the environment: the AUTO plan of the 5-point 64 x 64 matrix made with the columns."""
    import torch
    import cusp_autotuned_amd as cmi
    A = cmi.poisson5pt(64, 64, "csr")
    N = A.num_rows
    plan = cmi.Plan.csr(torch.float64, N, N, A.row_offsets, A.column_indices)
    print(json.dumps({"config": plan.config().as_dict(), "device_bytes": plan.device_bytes()}))


def test_waver_attempt_refused_by_min_piece_leaves_nothing_behind(cmi, torch_cuda):
    """A plain 5-point stencil has pieces of 1 + 3 + 1 columns: 1.67 entries per piece, below the rule's min_piece.  With $CMI_CSR_WAVER=1
    ("whenever the rows qualify") the AUTO plan made with the columns BUILDS the run-compressed copy to measure that, and drops it; what is
    left is the plan of the next route -- the one this process, without the switch, makes without trying.  The switch is read once per
    process, hence the child process."""
    torch = torch_cuda
    assert cmi.tuning_waver_rule(cmi.F64).as_dict()["min_piece"] > 5.0 / 3.0
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=120, cwd=root,
                       env=dict(os.environ, CMI_CSR_WAVER="1", PYTHONPATH=os.pathsep.join(p for p in (root, os.environ.get("PYTHONPATH")) if p)))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    tried = json.loads(r.stdout.strip().splitlines()[-1])
    A = cmi.poisson5pt(64, 64, "csr")
    N = A.num_rows
    plain = cmi.Plan.csr(torch.float64, N, N, A.row_offsets, A.column_indices)
    assert tried["config"]["kernel"] not in (cmi.CSR_STREAM_WAVER, cmi.CSR_STREAM_PACKED)
    assert tried["config"] == plain.config().as_dict()
    assert tried["device_bytes"] == plain.device_bytes() == 0  # (csr_wave's fixed tiles of 64 rows: nothing is built)


def test_sorted_coo_plan_owns_its_offsets_and_handles_end_cleanly(cmi, torch_cuda, orc):
    """A row-sorted COO plan of 300 rows owns 4 (rows + 1) bytes of row offsets plus what the CSR plan of those offsets owns; it and a
    SpGEMM result (the other handle that owns device blocks) are created, used and destroyed."""
    torch = torch_cuda
    rng = np.random.default_rng(12)
    rows = cols = 300
    lens = rng.integers(0, 9, size=rows)
    Ap = np.r_[0, np.cumsum(lens)].astype(np.int32)
    Aj = np.concatenate([np.sort(rng.choice(cols, size=l, replace=False)) for l in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    Ax = rng.standard_normal(len(Aj))
    x = rng.standard_normal(cols)
    Ai = orc.csr_row_indices(Ap)
    dAi, dAj, dAx, dAp = dev(Ai, torch), dev(Aj, torch), dev(Ax, torch), dev(Ap, torch)
    plan = cmi.Plan(cmi.FORMAT_COO, torch.float64, rows, cols, len(Aj), dAi)
    sub = cmi.Plan(cmi.FORMAT_CSR, torch.float64, rows, cols, len(Aj), dAp)
    assert plan.info()["coo_sorted"] is True and plan.config().as_dict() == sub.config().as_dict()
    assert plan.device_bytes() == 4 * (rows + 1) + sub.device_bytes(), (plan.device_bytes(), sub.device_bytes())
    y = torch.full((rows,), 10.0, dtype=torch.float64, device="cuda")
    cmi.spmv_coo_plan(plan, dAi, dAj, dAx, dev(x, torch), y)
    want = orc.spmv_coo(rows, Ai, Aj, Ax, x)
    bound = orc.spmv_csr(Ap, Aj, np.abs(Ax), np.abs(x))
    assert np.all(np.abs(y.cpu().numpy() - want) <= 1e-6 * np.maximum(bound, 1e-300))
    del plan, sub
    # C = B B for a 50 x 50 matrix of small positive integers: exact in f64, no cancellation
    n = 50
    D = np.where(rng.random((n, n)) < 0.15, rng.integers(1, 5, size=(n, n)), 0).astype(np.float64)
    Bp = np.r_[0, np.cumsum((D != 0).sum(axis=1))].astype(np.int32)
    Bj = np.nonzero(D)[1].astype(np.int32)
    Bx = D[D != 0]
    dB = [dev(a, torch) for a in (Bp, Bj, Bx)]
    Cp, Cj, Cx, info = cmi.spgemm_csr(n, n, n, *dB, *dB)
    Cp, Cj, Cx = (t.cpu().numpy() for t in (Cp, Cj, Cx))
    got = np.zeros((n, n))
    got[np.repeat(np.arange(n), np.diff(Cp)), Cj] = Cx
    assert info["slabs"] >= 1 and np.array_equal(got, D @ D) and len(Cj) == np.count_nonzero(D @ D)
    torch.cuda.synchronize()


if __name__ == "__main__":
    _waver_child()

"""Every multiply path that re-associates a row sum, held to its rounding-error bound (-m gpu).

The older bar of these paths, |y - y_ref| <= 1e-6 * sum|a x|, sits five to ten orders of magnitude above what a correct f64
kernel can produce, so it accepts a lane sum carried in float, a float atomic in the f64 instantiation or an LDS fold through
an array of the wrong type (tests/test_rounding_refs.py shows exactly that on the CPU).  Here y is compared with the EXACT row
sum (tests/rounding_refs.py: error-free products, math.fsum) under

    |y - exact| <= min(1e-6 | 1e-5, gamma_{n+1}(u_T)) * (sum|a x| + |y0|),

a theorem for any kernel that multiplies and adds in the working precision in any order; rows without entries must be +0.0 (or
y0's bits), rows of one entry their rounded product.  Every case names its kernel in an explicit config, so the tuning table
cannot route around it, and every (path, matrix) pair below is listed as RUNS or as refused with a given status.

$CMI_ROUNDING_TABLE=<file>: the worst err / (gamma_{n+1} B) per path and type is written there when the module finishes
(profiles/r22_rounding_bound.txt is such a file) -- information, not a threshold.
"""
import math
import os

import numpy as np
import pytest

import rounding_refs as rr

pytestmark = pytest.mark.gpu

DT = {"f64": np.float64, "f32": np.float32}
RUNS = "runs"
INVALID_VALUE = 1  # cmi_status CMI_ERROR_INVALID_VALUE (include/cusp_mi355x.h)
LONG_ROW = 512  # csr_stream with threads_per_row 0: shorter rows are summed in storage order (tests/test_spmv_gpu.py claims their bits)

WORST = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch


@pytest.fixture(scope="module", autouse=True)
def worst_ratio_table():
    yield
    path = os.environ.get("CMI_ROUNDING_TABLE")
    if path and WORST:
        with open(path, "w") as f:
            f.write("worst err / (gamma_(n+1) B) per path and value type, over the rows of 2+ terms and over the rows of 512+ terms (0: the\n")
            f.write("path's matrices have none): information, not a threshold.  tests/test_rounding_gpu.py on an MI355X; ladder / giant /\n")
            f.write("ell_ladder matrices, both value profiles, plain and accumulate.  Honest orders on the CPU reach 0.34 .. 0.60.\n")
            f.write("Rows whose entries meet in atomics (shuffled COO) are added in an order that changes from run to run, and so do their figures.\n\n")
            f.write(f"{'path':<40} {'f64 2+':>9} {'f64 512+':>9} {'f32 2+':>9} {'f32 512+':>9}\n")
            for p in sorted({p for p, _ in WORST}):
                cells = [f"{v:9.4f}" for t in ("f64", "f32") for v in WORST.get((p, t), (float("nan"), float("nan")))]
                f.write(f"{p:<40} " + " ".join(cells) + "\n")


_dev_cache = {}


def device(M, torch):
    """The matrix's arrays on the device, uploaded once."""
    key = (M.name, M.profile, M.dtype)
    if key not in _dev_cache:
        _dev_cache[key] = tuple(torch.from_numpy(np.array(a)).cuda() for a in (M.Ap, M.Aj, M.Ax, M.x, M.y0))
    return _dev_cache[key]


def up(a, torch):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the cached matrices are read-only)


def offset_view(a, torch):
    """`a` on the device as a view one element into a larger tensor: 4 or 8 bytes past a 16-byte boundary."""
    big = torch.empty(len(a) + 5, dtype=torch.from_numpy(a[:0].copy()).dtype, device="cuda")
    big[1:1 + len(a)] = up(a, torch)
    view = big[1:1 + len(a)]
    assert view.data_ptr() % 16 != 0 or len(a) == 0
    return view


def fresh_y(M, acc, torch):
    return device(M, torch)[4].clone() if acc else torch.full((M.rows,), 10.0, dtype=device(M, torch)[3].dtype, device="cuda")


def hold(path, tag, M, acc, y, what=""):
    """y against the exact row sums of M; the failure names the path, the row, n, err / B and the bar."""
    exact, B, n = rr.exact_of(M, acc)
    got = y.cpu().numpy()
    bad = rr.within_rounding_bound(got, exact, B, n, M.dtype)
    assert not bad, f"{path} {what} on {M.name}/{M.profile} {tag} acc={acc}: {len(bad)} rows outside the bound: {rr.describe(bad)}"
    was = WORST.get((path, tag), (0.0, 0.0))
    WORST[(path, tag)] = (max(was[0], rr.worst_ratio(got, exact, B, n, M.dtype)), max(was[1], rr.worst_ratio(got, exact, B, n, M.dtype, LONG_ROW)))
    return got


def matrices(names, dtype):
    return [rr.matrix(name, profile, dtype) for name in names for profile in rr.PROFILES]


def run_cases(cases, tag, torch, cmi, multiply):
    """cases: (path, config, {matrix name: RUNS | status}).  multiply(M, cfg, acc, y) launches; a refusal must carry the listed
    status; a path that runs on none of its matrices is a mistake in the list."""
    for path, cfg, expect in cases:
        ran = 0
        for name, outcome in expect.items():
            for profile in rr.PROFILES:
                M = rr.matrix(name.split()[0], profile, DT[tag])
                for acc in (False, True):
                    y = fresh_y(M, acc, torch)
                    if outcome == RUNS:
                        multiply(M, name, cfg, acc, y)
                        hold(path, tag, M, acc, y, name)
                        ran += 1
                    else:
                        with pytest.raises(cmi.CmiError) as e:
                            multiply(M, name, cfg, acc, y)
                        assert e.value.status == outcome, f"{path} on {name}: status {e.value.status}, listed {outcome}"
        assert ran, f"{path}: runs on none of its matrices"


# ------------------------------------------------------------------------------------------------------------------------
# CSR, plan-less, explicit configs
# ------------------------------------------------------------------------------------------------------------------------
def csr_cases(cmi):
    L, LG = {"ladder": RUNS}, {"ladder": RUNS, "giant": RUNS}
    out = [(f"csr_vector t{t}", cmi.Config(kernel=cmi.CSR_VECTOR, threads_per_row=t), L) for t in (2, 4, 8, 16, 32, 64)]
    out.append(("csr_stream t0", cmi.Config(kernel=cmi.CSR_STREAM, threads_per_row=0), LG))
    out += [(f"csr_stream t{t}", cmi.Config(kernel=cmi.CSR_STREAM, threads_per_row=t), L) for t in (2, 8, 64)]
    # csr_stream_pipe: its launcher (launch_pipe, spmv_csr.hip) never reads threads_per_row -- one lane per row whatever the field says -- and
    # refuses arrays that are not 16-byte aligned (and matrices of fewer than 4 entries: none here)
    out += [(f"csr_stream_pipe t{t}", cmi.Config(kernel=cmi.CSR_STREAM_PIPE, threads_per_row=t),
             {"ladder": RUNS, "giant": RUNS, "ladder (offset views)": INVALID_VALUE} if t == 0 else L) for t in (0, 2, 8, 64)]
    out.append(("csr_balanced", cmi.Config(kernel=cmi.CSR_BALANCED), LG))
    out.append(("csr_balanced items_per_thread=1", cmi.Config(kernel=cmi.CSR_BALANCED, items_per_thread=1), LG))
    out.append(("csr_balanced blocks_per_cu=1", cmi.Config(kernel=cmi.CSR_BALANCED, blocks_per_cu=1), LG))
    out.append(("csr NULL config", None, LG))
    return out


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_csr_explicit_configs(cmi, torch_cuda, orc, tag):
    torch = torch_cuda
    views = {}

    def multiply(M, name, cfg, acc, y):
        dAp, dAj, dAx, dx, _ = device(M, torch)
        if "offset views" in name:
            key = (M.name, M.profile)
            if key not in views:
                views[key] = (offset_view(M.Aj, torch), offset_view(M.Ax, torch))
            dAj, dAx = views[key]
        cmi.spmv_csr(M.rows, M.cols, dAp, dAj, dAx, dx, y, accumulate=acc, cfg=cfg)
        pipe = cfg is not None and cfg.kernel == cmi.CSR_STREAM_PIPE
        if pipe or (cfg is not None and cfg.kernel == cmi.CSR_STREAM and cfg.threads_per_row == 0):
            # the storage-order claims the suite already makes: pipe on every row, csr_stream t0 on rows shorter than 512 (without a
            # plan it never launches its long-row instance; test_csr_plans_on_giant runs that one)
            want = orc.spmv_csr(M.Ap, M.Aj, M.Ax, M.x, M.y0.copy() if acc else None)
            short = np.ones(M.rows, bool) if pipe else M.lengths < LONG_ROW
            assert np.array_equal(y.cpu().numpy()[short], want[short]), f"{name} acc={acc}: a storage-order row differs from the host loop"

    run_cases(csr_cases(cmi), tag, torch, cmi, multiply)


# ------------------------------------------------------------------------------------------------------------------------
# CSR through plans on `giant`: the profile-steered long-row instance / merge-path choice, and the 16-bit column plan
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_csr_plans_on_giant(cmi, torch_cuda, orc, tag):
    torch = torch_cuda
    for M in matrices(("giant",), DT[tag]):
        dAp, dAj, dAx, dx, _ = device(M, torch)
        plans = {
            "plan AUTO": cmi.Plan.csr(dx.dtype, M.rows, M.cols, dAp, dAj),
            "plan csr_stream_c16": cmi.Plan.csr(dx.dtype, M.rows, M.cols, dAp, dAj, cfg=cmi.Config(kernel=cmi.CSR_STREAM_C16)),
            # a plan KNOWS the longest row, so this one launches csr_stream's long-row instance (a plan-less call never does)
            "plan csr_stream t0": cmi.Plan(cmi.FORMAT_CSR, dx.dtype, M.rows, M.cols, len(M.Aj), dAp, cmi.Config(kernel=cmi.CSR_STREAM, threads_per_row=0)),
        }
        for path, plan in plans.items():
            info, c = plan.info(), plan.config()
            assert info["max_row_length"] == rr.GIANT_LENGTH
            assert info["storage_order_sums"] == 0, f"{path}: claims storage-order sums with a row of {rr.GIANT_LENGTH} entries ({c})"
            if path == "plan csr_stream t0":
                assert c.kernel == cmi.CSR_STREAM and c.threads_per_row == 0
            for acc in (False, True):
                y = fresh_y(M, acc, torch)
                cmi.spmv_csr_plan(plan, dAp, dAj, dAx, dx, y, accumulate=acc)
                got = hold(path, tag, M, acc, y, f"(kernel {c.kernel})")
                if c.kernel == cmi.CSR_STREAM and c.threads_per_row <= 1:  # the class whose short rows the suite pins bit for bit
                    want = orc.spmv_csr(M.Ap, M.Aj, M.Ax, M.x, M.y0.copy() if acc else None)
                    short = M.lengths < LONG_ROW
                    assert np.array_equal(got[short], want[short]), f"{path} acc={acc}: a row shorter than {LONG_ROW} is not the host loop's"


# ------------------------------------------------------------------------------------------------------------------------
# ELL: several lanes per row
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_ell_lanes(cmi, torch_cuda, orc, tag):
    torch = torch_cuda
    for M in matrices(("ell_ladder",), DT[tag]):
        width = int(M.lengths.max())
        assert width == 129
        _, _, _, dx, _ = device(M, torch)
        # threads_per_row 0 must not quietly be the one-lane kernel here: the auto rule splits rows of 129 slots
        auto = cmi.Plan(cmi.FORMAT_ELL, dx.dtype, M.rows, M.cols, M.rows * width, None, cfg=cmi.Config(kernel=cmi.ELL_ROW, threads_per_row=0))
        assert auto.info()["storage_order_sums"] is False
        ran = {}
        for alignment in (1, 32):  # pitch = the row count (492: odd pairs of rows), and the default pitch (a multiple of 32)
            pitch, eAj, eAx = orc.csr_to_ell(M.Ap, M.Aj, M.Ax, width, alignment=alignment)
            assert pitch == (M.rows if alignment == 1 else -(-M.rows // 32) * 32)
            deAj, deAx = up(eAj, torch), up(eAx, torch)
            rl = up(M.lengths.astype(np.int32), torch)
            for lanes in (2, 4, 8, 16, 0):  # 0: the auto rule -- 129 slots, 492 rows: 8 lanes (ell_lanes_per_row, spmv_ell_dia.hip)
                for ellr in (False, True):
                    path = f"ell_row t{lanes}{' ellr' if ellr else ''}"
                    for acc in (False, True):
                        y = fresh_y(M, acc, torch)
                        cmi.spmv_ell(M.rows, M.cols, width, pitch, deAj, deAx, dx, y, row_lengths=rl if ellr else None, accumulate=acc,
                                     cfg=cmi.Config(kernel=cmi.ELL_ROW, threads_per_row=lanes))
                        hold(path, tag, M, acc, y, f"pitch {pitch}")
                        ran[path] = ran.get(path, 0) + 1
        assert len(ran) == 10 and all(v == 4 for v in ran.values())


# ------------------------------------------------------------------------------------------------------------------------
# COO: the order-agnostic kernels (segmented reduction + atomics)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("name", ["ladder", "giant"])
def test_coo_kernels(cmi, torch_cuda, orc, tag, name):
    torch = torch_cuda
    for M in matrices((name,), DT[tag]):
        _, _, _, dx, _ = device(M, torch)
        Ai = orc.csr_row_indices(M.Ap)
        perm = np.random.default_rng(21).permutation(len(Ai))
        orders = {
            "csr order": tuple(up(a, torch) for a in (Ai, M.Aj, M.Ax)),
            "shuffled": tuple(up(a[perm], torch) for a in (Ai, M.Aj, M.Ax)),
            "offset views": tuple(offset_view(a, torch) for a in (Ai, M.Aj, M.Ax)),  # not 16-byte aligned: the scalar-load path
        }
        for kern, kname in ((cmi.COO_SEGMENTED, "coo_segmented"), (cmi.COO_LANE4, "coo_lane4")):
            for order, (dAi, dAj, dAx) in orders.items():
                for acc in (False, True):
                    y = fresh_y(M, acc, torch)
                    cmi.spmv_coo(M.rows, M.cols, dAi, dAj, dAx, dx, y, accumulate=acc, cfg=cmi.Config(kernel=kern))
                    hold(f"{kname} {order}", tag, M, acc, y)


# ------------------------------------------------------------------------------------------------------------------------
# HYB: two launches (ELL part, COO part on top), and through a plan
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_hyb_two_launches_and_plan(cmi, torch_cuda, orc, tag):
    torch = torch_cuda
    for M in matrices(("ladder",), DT[tag]):
        _, _, _, dx, _ = device(M, torch)
        for width in (0, 3, 16):
            pitch, eAj, eAx, cAi, cAj, cAx = orc.csr_to_hyb(M.Ap, M.Aj, M.Ax, width)
            assert len(cAi) == int(np.maximum(M.lengths - width, 0).sum()) > 0
            perm = np.random.default_rng(22).permutation(len(cAi))
            deAj, deAx = up(eAj, torch), up(eAx, torch)
            for order, coo in (("", (cAi, cAj, cAx)), (" coo shuffled", (cAi[perm], cAj[perm], cAx[perm]))):
                d = [up(a, torch) for a in coo]
                for acc in (False, True):
                    y = fresh_y(M, acc, torch)
                    cmi.spmv_hyb(M.rows, M.cols, width, pitch, deAj, deAx, *d, dx, y, accumulate=acc)
                    hold(f"hyb two launches w{width}{order}", tag, M, acc, y)
                if width == 3:
                    plan = cmi.Plan.hyb(dx.dtype, M.rows, M.cols, width, d[0])
                    if order == "":
                        assert plan.info()["coo_sorted"] is True
                    for acc in (True, False):
                        y = fresh_y(M, acc, torch)
                        cmi.spmv_hyb_plan(plan, pitch, deAj, deAx, *d, dx, y, accumulate=acc)
                        hold(f"hyb plan w{width}{order}", tag, M, acc, y, f"({plan.hyb_launches()} launches)")


# ------------------------------------------------------------------------------------------------------------------------
# fused multiply + dot on re-associating kernels
# ------------------------------------------------------------------------------------------------------------------------
def hold_dot(path, y, w, res):
    terms = (y.astype(np.float64) * w.astype(np.float64)).tolist()  # (f32: exact in float64; f64: the products the kernel forms)
    ref, mag = math.fsum(terms), math.fsum(abs(t) for t in terms)
    assert abs(res - ref) <= 1e-12 * mag, f"{path}: <y, w> = {res!r}, fsum of the returned y gives {ref!r}, sum|y w| = {mag!r}"


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_fused_dots_on_lane_group_kernels(cmi, torch_cuda, orc, tag):
    torch = torch_cuda
    ws = cmi.blas_workspace()
    for M in matrices(("ladder", "giant"), DT[tag]):
        dAp, dAj, dAx, dx, _ = device(M, torch)
        w = np.random.default_rng(23).standard_normal(M.rows).astype(M.dtype)
        for t in (4, 32):
            res = torch.zeros(1, dtype=torch.float64, device="cuda")
            y = fresh_y(M, False, torch)
            cmi.spmv_csr_dot(M.rows, M.cols, dAp, dAj, dAx, dx, y, up(w, torch), res, ws, cfg=cmi.Config(kernel=cmi.CSR_VECTOR, threads_per_row=t))
            got = hold(f"csr_dot csr_vector t{t}", tag, M, False, y)
            hold_dot(f"csr_dot csr_vector t{t} on {M.name}/{M.profile} {tag}", got, w, res.item())
    for M in matrices(("ell_ladder",), DT[tag]):
        _, _, _, dx, _ = device(M, torch)
        w = np.random.default_rng(24).standard_normal(M.rows).astype(M.dtype)
        width = int(M.lengths.max())
        pitch, eAj, eAx = orc.csr_to_ell(M.Ap, M.Aj, M.Ax, width)
        for ellr in (False, True):
            res = torch.zeros(1, dtype=torch.float64, device="cuda")
            y = fresh_y(M, False, torch)
            cmi.spmv_ell_dot(M.rows, M.cols, width, pitch, up(eAj, torch), up(eAx, torch), dx, y, up(w, torch), res, ws,
                             row_lengths=up(M.lengths.astype(np.int32), torch) if ellr else None, cfg=cmi.Config(kernel=cmi.ELL_ROW, threads_per_row=4))
            got = hold(f"ell_dot ell_row t4{' ellr' if ellr else ''}", tag, M, False, y)
            hold_dot(f"ell_dot t4 on {M.name}/{M.profile} {tag}", got, w, res.item())

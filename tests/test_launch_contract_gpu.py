"""What the host code between "a launch shape has been chosen" and the launch promises, pinned to what the parent build did.

Everything here compares against tests/golden/launch_contract.json, which `record()` (below, run by hand on an MI355X with the
library of the commit the file names) wrote.  Nothing is compared with a second run of the code under test.  Three parts:

1. Refusals: every fail(...) of the launchers in spmv_csr.hip, spmv_csr16.hip, spmv_csr_runs.hip, spmv_ell_dia.hip and
   spmv_coo_hyb.hip that a 300-row tridiagonal matrix reaches -- status and the exact cmi_last_error() text.  A case the library
   completes instead of refusing (tuning.hip rounds threads_per_row 3 to 4 and items_per_thread 3 to 4 before any launcher sees
   them; a WAVEX plan turns items_per_thread 1 into 2) or refuses at plan creation already (items_per_thread 3 on WAVEV / WAVER,
   PACKED without the values) is recorded and asserted as that.
   Not asserted, because no small shape reaches them: the "<kernel>: grid too large" checks (a grid beyond INT32_MAX workgroups),
   "tile does not fit 160 KiB of LDS" of csr_stream and csr_stream_c16 (block_size is rounded to at most 1024 lanes: 64 KiB + the row
   offsets), "csr_balanced: matrix too large", the "sizes exceed the int32 index type" / "too many entries for the tile kernel"
   checks, and "CMI_CSR_STREAM_PACKED: the plan holds no packed copy" (a plan's kernel is PACKED only when the copy was made).
   Misaligned views are asserted only where the launcher refuses them before the launch: csr_wavev takes any x, csr_waver any Aj.
2. Partial counts: cmi_spmv_csr_dot_plan_partials on every CSR route that fuses <y, w>, asked for with XCD dealing 0, 1 and 4, on a
   pentadiagonal matrix of 4100 rows (17 tiles of 256 rows: not a multiple of 8, the last one partial): the plan's resolved config,
   the count, and the bits of the scalar after the fold.  csr_wave on a plan's partition and csr_wavev's 16-bit copy WITHOUT shift
   tiles need rows that are not all alike: they run on the same matrix with every fourth row cut down to its diagonal.  ELL, DIA,
   HYB and COO expose only the scalar.  Routes that take the table's dealing whatever the caller asks (csr_wave on a partition, the
   wave-tiled 16-bit copy, packed 16-bit tiles) show that in their recorded config.
3. Fall-back: 131 073 tiles, one more than the workspace holds partials -- the count is 0 and the scalar is the library's dot of the
   computed y, bit for bit.  csr_stream is called without a plan (through a plan its launcher widens the tiles until they fit; that
   count is recorded too)."""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_FILE = os.path.join(ROOT, "tests", "golden", "launch_contract.json")
TAGS = {"f64": np.float64, "f32": np.float32}
N, NT, NBIG = 4100, 300, 1048584
SWIZZLES = (0, 1, 4)


# ------------------------------------------------------------------------------------------------
# inputs (host, seeded) and their device copies, made once
# ------------------------------------------------------------------------------------------------
def banded_csr(n, offsets, dtype, seed, thin=False):
    """CSR of the band matrix with these diagonals, values uniform in [-1, 1); thin: every fourth row keeps only its diagonal."""
    rows = np.repeat(np.arange(n, dtype=np.int64), len(offsets))
    cols = rows + np.tile(np.asarray(offsets, np.int64), n)
    keep = (cols >= 0) & (cols < n)
    if thin:
        keep &= (rows % 4 != 3) | (cols == rows)
    rows, cols = rows[keep], cols[keep]
    Ap = np.zeros(n + 1, np.int64)
    np.add.at(Ap, rows + 1, 1)
    Ax = np.random.default_rng(seed).uniform(-1.0, 1.0, rows.size).astype(dtype)
    return np.cumsum(Ap).astype(np.int32), cols.astype(np.int32), Ax


def vectors(n, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, n).astype(dtype), rng.uniform(-1.0, 1.0, n).astype(dtype)


MATRICES = {
    "penta": lambda dt: banded_csr(N, (-64, -1, 0, 1, 64), dt, 17),
    "thin": lambda dt: banded_csr(N, (-64, -1, 0, 1, 64), dt, 17, thin=True),
    "tri": lambda dt: banded_csr(NT, (-1, 0, 1), dt, 19),
    "big": lambda dt: banded_csr(NBIG, (-1, 0, 1), dt, 23),
}


class Dev:
    """One matrix of one value type on the device, with x, w and a workspace."""

    def __init__(self, b, torch, name, tag):
        dt = TAGS[tag]
        self.hAp, self.hAj, self.hAx = MATRICES[name](dt)
        self.n, self.nnz = self.hAp.size - 1, self.hAj.size
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.up = up
        self.Ap, self.Aj, self.Ax = up(self.hAp), up(self.hAj), up(self.hAx)
        hx, hw = vectors(self.n, dt, 29)
        self.x, self.w = up(hx), up(hw)
        self.tdt = self.x.dtype
        self.ws = b.blas_workspace()
        self.torch = torch

    def y(self):
        return self.torch.full((self.n,), 10.0, dtype=self.tdt, device="cuda")  # poisoned: every row must be written

    def res(self):
        return self.torch.zeros(1, dtype=self.torch.float64, device="cuda")

    def ell(self, width=None):
        """(width, pitch, Aj, Ax) column-major with -1 / 0 padding, and the COO rest (Ai, Aj, Ax) of rows longer than `width`."""
        L = np.diff(self.hAp)
        full = int(L.max())
        width = full if width is None else width
        eAj = np.full((width, self.n), -1, np.int32)
        eAx = np.zeros((width, self.n), self.hAx.dtype)
        for k in range(width):
            r = np.nonzero(L > k)[0]
            eAj[k, r], eAx[k, r] = self.hAj[self.hAp[r] + k], self.hAx[self.hAp[r] + k]
        Ai = np.repeat(np.arange(self.n, dtype=np.int32), L)
        rest = np.arange(self.nnz) - np.repeat(self.hAp[:-1], L) >= width
        return (width, self.n, self.up(eAj.ravel()), self.up(eAx.ravel())), tuple(self.up(a[rest]) for a in (Ai, self.hAj, self.hAx))

    def dia(self):
        off = np.array((-64, -1, 0, 1, 64), np.int32)
        Ai = np.repeat(np.arange(self.n), np.diff(self.hAp))
        vals = np.zeros((off.size, self.n), self.hAx.dtype)
        vals[np.searchsorted(off, self.hAj - Ai), Ai] = self.hAx
        return self.up(off), self.up(vals.ravel())


_dev = {}


def dev(b, torch, name, tag):
    if (name, tag) not in _dev:
        _dev[(name, tag)] = Dev(b, torch, name, tag)
    return _dev[(name, tag)]


def bits(t):
    return format(int(t.cpu().numpy().view(np.uint64)[0]), "016x")


def outcome(b, fn):
    """What a call did: its result dict, or the status and message it was refused with."""
    try:
        return dict(fn() or {}, status=0)
    except b.CmiError as e:
        return {"status": e.status, "error": str(e)}


def misaligned(torch, t):
    """The same contents one element past a 16-byte boundary."""
    big = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    big[1:] = t
    return big[1:]


# ------------------------------------------------------------------------------------------------
# part 1: refusals
# ------------------------------------------------------------------------------------------------
def planless(kernel, **kw):
    def run(b, torch, D, view=None):
        a = {"Aj": D.Aj, "Ax": D.Ax, "x": D.x}
        if view:
            a[view] = misaligned(torch, a[view])
        b.spmv_csr(D.n, D.n, D.Ap, a["Aj"], a["Ax"], a["x"], D.y(), cfg=b.Config(kernel=getattr(b, kernel), **kw))
    return run


def planned(make, kernel, view=None, **kw):
    """A plan of the kind `make` for the kernel asked for by name, then one multiply (with one array misaligned)."""
    def run(b, torch, D):
        cfg = b.Config(kernel=getattr(b, kernel), **kw)
        if make == "offsets":
            plan = b.Plan(b.FORMAT_CSR, D.tdt, D.n, D.n, D.nnz, D.Ap, cfg)
        elif make == "columns":
            plan = b.Plan.csr(D.tdt, D.n, D.n, D.Ap, D.Aj, cfg=cfg)
        else:
            plan = b.Plan.csr_values(D.n, D.n, D.Ap, D.Aj, D.Ax, cfg=cfg)
        a = {"Aj": D.Aj, "Ax": D.Ax, "x": D.x}
        if view:
            a[view] = misaligned(torch, a[view])
        b.spmv_csr_plan(plan, D.Ap, a["Aj"], a["Ax"], a["x"], D.y())
        return {"kernel": plan.config().kernel}
    return run


def pitch_short(fmt):
    def run(b, torch, D):
        if fmt == "ell":
            (width, pitch, eAj, eAx), _ = D.ell()
            b.spmv_ell(D.n, D.n, width, pitch - 1, eAj, eAx, D.x, D.y(), cfg=b.Config(kernel=b.ELL_ROW, threads_per_row=1))
        elif fmt == "dia":
            off = D.up(np.array((-1, 0, 1), np.int32))
            vals = D.torch.zeros(3 * D.n, dtype=D.tdt, device="cuda")
            b.spmv_dia(D.n, D.n, 3, D.n - 1, off, vals, D.x, D.y(), cfg=b.Config(kernel=b.DIA_ROW))
        else:  # the one-launch HYB kernel; the binding's own length check is stepped over: the library's is the one asserted
            (width, pitch, eAj, eAx), (cAi, cAj, cAx) = D.ell(2)
            plan = b.Plan.hyb(D.tdt, D.n, D.n, width, cAi, cfg_ell=b.Config(kernel=b.ELL_ROW, threads_per_row=1))
            args = b.hyb_plan_args(plan, pitch, eAj, eAx, cAi, cAj, cAx)
            b.spmv_hyb_plan_args(args[:2] + (pitch - 1,) + args[3:], D.x, D.y())
            return {"launches": plan.hyb_launches()}
    return run


def wrong_format(call):
    def run(b, torch, D):
        (width, pitch, eAj, eAx), _ = D.ell()
        Ai = D.up(np.repeat(np.arange(D.n, dtype=np.int32), np.diff(D.hAp)))
        if call == "csr":
            b.spmv_csr(D.n, D.n, D.Ap, D.Aj, D.Ax, D.x, D.y(), cfg=b.Config(kernel=b.ELL_ROW))
        elif call == "ell":
            b.spmv_ell(D.n, D.n, width, pitch, eAj, eAx, D.x, D.y(), cfg=b.Config(kernel=b.CSR_SCALAR))
        elif call == "dia":
            b.spmv_dia(D.n, D.n, 1, D.n, D.up(np.zeros(1, np.int32)), D.torch.ones(D.n, dtype=D.tdt, device="cuda"), D.x, D.y(), cfg=b.Config(kernel=b.CSR_SCALAR))
        else:
            b.spmv_coo(D.n, D.n, Ai, D.Aj, D.Ax, D.x, D.y(), cfg=b.Config(kernel=b.CSR_SCALAR))
    return run


REFUSALS = {
    "csr_vector threads_per_row 3": planless("CSR_VECTOR", threads_per_row=3),
    "csr_stream threads_per_row 3": planless("CSR_STREAM", threads_per_row=3),
    "csr_stream rows_per_block beyond 4 block / tpr": planless("CSR_STREAM", block_size=64, threads_per_row=1, rows_per_block=257),
    "csr_stream rows_per_block beyond 4 block / tpr, 4 lanes": planless("CSR_STREAM", block_size=64, threads_per_row=4, rows_per_block=65),
    "csr_stream items_per_thread 3": planless("CSR_STREAM", threads_per_row=1, items_per_thread=3),
    "csr_wave K 1": planless("CSR_STREAM_WAVE", block_size=256, rows_per_block=256, items_per_thread=1),
    "csr_wave K 11": planless("CSR_STREAM_WAVE", block_size=256, rows_per_block=256, items_per_thread=11),
    "csr_wave rows_per_block not whole waves": planless("CSR_STREAM_WAVE", block_size=256, rows_per_block=6, items_per_thread=3),
    "csr_wave rows_per_block beyond 64 per wave": planless("CSR_STREAM_WAVE", block_size=64, rows_per_block=65, items_per_thread=3),
    "csr_wave 1024 lanes x 10 entries": planless("CSR_STREAM_WAVE", block_size=1024, rows_per_block=1024, items_per_thread=10),
    "WAVEV without a plan": planless("CSR_STREAM_WAVEV"),
    "WAVEX without a plan": planless("CSR_STREAM_WAVEX"),
    "WAVER without a plan": planless("CSR_STREAM_WAVER"),
    "PACKED without a plan": planless("CSR_STREAM_PACKED"),
    "C16 without a plan": planless("CSR_STREAM_C16"),
    "csr_stream_pipe rows_per_block = block_size": planless("CSR_STREAM_PIPE", block_size=64, rows_per_block=64),
    "csr_stream_pipe misaligned Aj": lambda b, torch, D: planless("CSR_STREAM_PIPE")(b, torch, D, "Aj"),
    "csr_stream_pipe misaligned Ax": lambda b, torch, D: planless("CSR_STREAM_PIPE")(b, torch, D, "Ax"),
    "cmi_spmv_csr with an ELL kernel": wrong_format("csr"),
    "cmi_spmv_ell with a CSR kernel": wrong_format("ell"),
    "cmi_spmv_dia with a CSR kernel": wrong_format("dia"),
    "cmi_spmv_coo with a CSR kernel": wrong_format("coo"),
    "plan WAVEV items_per_thread 3": planned("offsets", "CSR_STREAM_WAVEV", items_per_thread=3),
    "plan WAVEX items_per_thread 1": planned("offsets", "CSR_STREAM_WAVEX", items_per_thread=1),
    "plan WAVER items_per_thread 3": planned("columns", "CSR_STREAM_WAVER", items_per_thread=3),
    "plan WAVEV misaligned Aj": planned("offsets", "CSR_STREAM_WAVEV", "Aj", items_per_thread=1),
    "plan WAVEV misaligned Ax": planned("offsets", "CSR_STREAM_WAVEV", "Ax", items_per_thread=1),
    "plan WAVEX misaligned Aj": planned("offsets", "CSR_STREAM_WAVEX", "Aj", items_per_thread=2),
    "plan WAVEX misaligned Ax": planned("offsets", "CSR_STREAM_WAVEX", "Ax", items_per_thread=2),
    "plan WAVEX misaligned x": planned("offsets", "CSR_STREAM_WAVEX", "x", items_per_thread=2),
    "plan WAVER misaligned Ax": planned("columns", "CSR_STREAM_WAVER", "Ax", items_per_thread=1),
    "plan C16 misaligned Ax": planned("columns", "CSR_STREAM_C16", "Ax"),
    "plan PACKED from the row offsets alone": planned("offsets", "CSR_STREAM_PACKED"),
    "plan PACKED without the values": planned("columns", "CSR_STREAM_PACKED"),
    "cmi_spmv_ell pitch < rows": pitch_short("ell"),
    "cmi_spmv_dia pitch < rows": pitch_short("dia"),
    "cmi_spmv_hyb_plan pitch < rows": pitch_short("hyb"),
}


def run_refusal(b, torch, name):
    D = dev(b, torch, "tri", "f64")
    return outcome(b, lambda: REFUSALS[name](b, torch, D))


# ------------------------------------------------------------------------------------------------
# part 2: partial counts and the folded scalar
# ------------------------------------------------------------------------------------------------
# name: (how the plan is made, matrix, kernel, config fields besides the XCD dealing)
CSR_ROUTES = {
    "csr_stream": ("offsets", "penta", "CSR_STREAM", dict(block_size=256, threads_per_row=1, rows_per_block=256, items_per_thread=2)),
    "csr_wave 64-row tiles": ("offsets", "penta", "CSR_STREAM_WAVE", dict(block_size=256, rows_per_block=256, items_per_thread=5)),
    "csr_wave partition": ("offsets", "thin", "CSR_STREAM_WAVE", dict(rows_per_block=-1, items_per_thread=5)),
    "csr_wavev 32-bit columns": ("offsets", "penta", "CSR_STREAM_WAVEV", dict(items_per_thread=1)),
    "csr_wavev 16-bit copy": ("columns", "thin", "CSR_STREAM_WAVEV", dict(items_per_thread=1, nontemporal=8)),
    "csr_wavev shift tiles": ("columns", "penta", "CSR_STREAM_WAVEV", dict(items_per_thread=1, nontemporal=8)),
    "csr_wavex": ("offsets", "penta", "CSR_STREAM_WAVEX", dict(items_per_thread=2, rows_per_block=2048)),
    "csr_waver": ("columns", "penta", "CSR_STREAM_WAVER", dict(items_per_thread=1)),
    "packed runs": ("values", "thin", "CSR_STREAM_PACKED", dict(items_per_thread=1)),
    "packed 16-bit tiles": ("values", "penta", "CSR_STREAM_PACKED", dict()),
    "c16 stream": ("columns", "penta", "CSR_STREAM_C16", dict(block_size=256, rows_per_block=256, items_per_thread=2)),
    "c16 wave": ("columns", "penta", "CSR_STREAM_C16", dict()),
}
OTHER_ROUTES = ("ell", "dia", "hyb", "coo")


def run_csr_route(b, torch, name, tag, swz):
    make, matrix, kernel, kw = CSR_ROUTES[name]
    D = dev(b, torch, matrix, tag)

    def go():
        cfg = b.Config(kernel=getattr(b, kernel), xcd_swizzle=swz if swz else -1, **kw)  # (0 in a config: "the table's"; < 0: launch order)
        if make == "offsets":
            plan = b.Plan(b.FORMAT_CSR, D.tdt, D.n, D.n, D.nnz, D.Ap, cfg)
        elif make == "columns":
            plan = b.Plan.csr(D.tdt, D.n, D.n, D.Ap, D.Aj, cfg=cfg)
        else:
            plan = b.Plan.csr_values(D.n, D.n, D.Ap, D.Aj, D.Ax, cfg=cfg)
        count = b.spmv_csr_dot_partials(plan, D.Ap, D.Aj, D.Ax, D.x, D.y(), D.w, D.ws)
        res = D.res()
        b.spmv_csr_dot(D.n, D.n, D.Ap, D.Aj, D.Ax, D.x, D.y(), D.w, res, D.ws, plan=plan)
        return {"config": plan.config().as_dict(), "shift_tiles": plan.shifted_tiles(), "count": count, "dot": bits(res)}
    return outcome(b, go)


def run_other_route(b, torch, name, tag, swz):
    D = dev(b, torch, "penta", tag)
    s = swz if swz else -1

    def go():
        res, out = D.res(), {}
        if name == "ell":
            (width, pitch, eAj, eAx), _ = D.ell()
            cfg = b.Config(kernel=b.ELL_ROW, block_size=256, threads_per_row=1, items_per_thread=1, xcd_swizzle=s)
            b.spmv_ell_dot(D.n, D.n, width, pitch, eAj, eAx, D.x, D.y(), D.w, res, D.ws, cfg=cfg)
        elif name == "dia":
            off, vals = D.dia()
            cfg = b.Config(kernel=b.DIA_ROW, block_size=256, items_per_thread=1, xcd_swizzle=s)
            b.spmv_dia_dot(D.n, D.n, off.numel(), D.n, off, vals, D.x, D.y(), D.w, res, D.ws, cfg=cfg)
        elif name == "hyb":
            (width, pitch, eAj, eAx), (cAi, cAj, cAx) = D.ell(3)
            plan = b.Plan.hyb(D.tdt, D.n, D.n, width, cAi, cfg_ell=b.Config(kernel=b.ELL_ROW, threads_per_row=1, xcd_swizzle=s))
            out = {"launches": plan.hyb_launches()}
            b.spmv_hyb_dot_plan_args(b.hyb_plan_args(plan, pitch, eAj, eAx, cAi, cAj, cAx), D.x, D.y(), D.w, res, D.ws)
        else:  # sorted COO: the plan's row offsets and the CSR kernels (the table's dealing: nothing to ask for)
            Ai = D.up(np.repeat(np.arange(D.n, dtype=np.int32), np.diff(D.hAp)))
            plan = b.Plan.coo(D.tdt, D.n, D.n, Ai, D.Aj)
            out = {"config": plan.config().as_dict()}
            b.spmv_coo_dot_plan(plan, Ai, D.Aj, D.Ax, D.x, D.y(), D.w, res, D.ws)
        return dict(out, dot=bits(res))
    return outcome(b, go)


# ------------------------------------------------------------------------------------------------
# part 3: one tile more than the workspace holds partials
# ------------------------------------------------------------------------------------------------
def run_fallback(b, torch, kernel, tag):
    D = dev(b, torch, "big", tag)
    kw = dict(block_size=64, rows_per_block=8, items_per_thread=3) if kernel == "CSR_STREAM_WAVE" else \
        dict(block_size=64, rows_per_block=8, threads_per_row=1, items_per_thread=1)
    cfg = b.Config(kernel=getattr(b, kernel), **kw)

    def go():
        plan = b.Plan(b.FORMAT_CSR, D.tdt, D.n, D.n, D.nnz, D.Ap, cfg)
        out = {"plan_count": b.spmv_csr_dot_partials(plan, D.Ap, D.Aj, D.Ax, D.x, D.y(), D.w, D.ws)}
        res, y = D.res(), D.y()
        if kernel == "CSR_STREAM_WAVE":
            b.spmv_csr_dot(D.n, D.n, D.Ap, D.Aj, D.Ax, D.x, y, D.w, res, D.ws, plan=plan)
        else:
            b.spmv_csr_dot(D.n, D.n, D.Ap, D.Aj, D.Ax, D.x, y, D.w, res, D.ws, cfg=cfg)
        plain = D.res()
        b.blas_dotd(y, D.w, plain, D.ws)
        return dict(out, dot=bits(res), blas_dot=bits(plain))
    return outcome(b, go)


# ------------------------------------------------------------------------------------------------
# the recorder (by hand, with the library of the commit it names) and the tests
# ------------------------------------------------------------------------------------------------
def record(commit, path=GOLDEN_FILE):
    import torch
    import cusp_autotuned_amd as cmi
    b = cmi.binding
    gold = {"commit": commit, "refusals": {n: run_refusal(b, torch, n) for n in REFUSALS}, "partials": {}, "fallback": {}}
    for tag in TAGS:
        for swz in SWIZZLES:
            for n in CSR_ROUTES:
                gold["partials"][f"{n} {tag} swizzle {swz}"] = run_csr_route(b, torch, n, tag, swz)
            for n in OTHER_ROUTES:
                gold["partials"][f"{n} {tag} swizzle {swz}"] = run_other_route(b, torch, n, tag, swz)
        for k in ("CSR_STREAM", "CSR_STREAM_WAVE"):
            gold["fallback"][f"{k} {tag}"] = run_fallback(b, torch, k, tag)
    with open(path, "w") as f:
        json.dump(gold, f, indent=1, sort_keys=True)
        f.write("\n")
    return gold


@pytest.fixture(scope="module")
def gold():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def gpu(cmi):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return cmi.binding, torch


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(REFUSALS), ids=[n.replace(" ", "_") for n in REFUSALS])
def test_refusal(gpu, gold, name):
    got = run_refusal(*gpu, name)
    print(name, got)
    assert got == gold["refusals"][name]


@pytest.mark.gpu
@pytest.mark.parametrize("swz", SWIZZLES)
@pytest.mark.parametrize("tag", list(TAGS))
@pytest.mark.parametrize("name", list(CSR_ROUTES) + list(OTHER_ROUTES), ids=lambda n: n.replace(" ", "_"))
def test_partial_count_and_folded_scalar(gpu, gold, name, tag, swz):
    got = (run_csr_route if name in CSR_ROUTES else run_other_route)(*gpu, name, tag, swz)
    print(name, tag, swz, got)
    want = gold["partials"][f"{name} {tag} swizzle {swz}"]
    assert got == want
    if name in CSR_ROUTES:  # (what the golden file itself must say: these routes fuse the dot)
        assert want["status"] == 0 and want["count"] > 0 and want["config"]["kernel"] == getattr(gpu[0], CSR_ROUTES[name][2])


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(TAGS))
@pytest.mark.parametrize("kernel", ["CSR_STREAM", "CSR_STREAM_WAVE"])
def test_one_tile_too_many_falls_back_to_the_plain_dot(gpu, gold, kernel, tag):
    got = run_fallback(*gpu, kernel, tag)
    print(kernel, tag, got)
    assert got == gold["fallback"][f"{kernel} {tag}"]
    assert got["status"] == 0 and got["dot"] == got["blas_dot"]
    if kernel == "CSR_STREAM_WAVE":
        assert got["plan_count"] == 0  # (csr_stream's count is not exposed without a plan; through one the launcher re-tiles)

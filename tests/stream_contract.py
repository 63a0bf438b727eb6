"""The inventory behind tests/test_stream_contract_gpu.py: one row per family of include/cusp_mi355x.h that takes a `void *stream`
(the _f64 / _f32 / _i32 suffix dropped), each in exactly one class.

  ASYNC  the header promises "no allocation, no synchronisation" (or says nothing about synchronising) and the call returns no
         host value that was read from the device: its work is ordered on the given stream and it records into a stream capture.
  SYNC   a set-up call: it returns a host value read from the device, or owns scratch, and synchronises the given stream.
  OUT    out of scope, with the reason in the row: the collectives and communicator calls (they need more than one rank),
         cmi_copy_ranges and the runtime helpers (thin wrappers over the HIP runtime, no kernel of the library's).

A row of ASYNC or SYNC carries a builder.  `builder(ctx, T)` returns a list of Case objects (usually one; the Gauss-Seidel colour
call has its one-launch and its parked two-launch form): device inputs in two value sets, the output buffers, `call(stream)` and
`check(k, returned)`, which compares what the call left behind with the reference of value set k.  Every expected value comes
from the restatements the family's own kernel-level suite uses (tests/*_refs.py, the oracle), compared by that suite's rule: bit
equality for fixed chains, the rounding bound of rounding_refs.py for row sums in any order, 1e-12 sum|terms| against math.fsum for
the reductions accumulated in double.  Nothing here is a new tolerance and nothing expected comes from a call of the library.

Importable without a GPU: torch and the library are touched only inside the builders."""
import ctypes
import functools
import math
import re

import numpy as np

ASYNC, SYNC, OUT = "a", "b", "c"
TYPES = {"f64": np.float64, "f32": np.float32, "i32": np.int32}
SENTINEL = -777.25          # outputs hold it before every call (integers: -7)
N1 = 5 * 1024 + 3           # BLAS-1: 1024 elements per workgroup -> 6 partials (the fold runs) and a ragged tail
NX, NY = 83, 61             # the matrix of test_multiply_inside_hip_graph_capture: 5063 rows, 20 workgroups of 256 rows

# class OUT may hold these families and no others
OUT_OF_SCOPE = {
    "cmi_allgather": "collective: needs more than one rank", "cmi_allgatherv": "collective: needs more than one rank",
    "cmi_allreduce": "collective: needs more than one rank", "cmi_halo_exchange": "collective: needs more than one rank",
    "cmi_comm_barrier": "communicator call: needs more than one rank", "cmi_comm_allgather_host": "communicator call: needs more than one rank",
    "cmi_copy_ranges": "the one-sided halo pull of cusp/distributed: raw addresses of peer memory",
    "cmi_memcpy_h2d": "runtime helper: hipMemcpy", "cmi_memcpy_d2h": "runtime helper: hipMemcpy", "cmi_memcpy_d2d": "runtime helper: hipMemcpy",
    "cmi_memcpy_d2h_async": "runtime helper: hipMemcpyAsync", "cmi_memset": "runtime helper: hipMemset",
    "cmi_event_record": "runtime helper: hipEventRecord", "cmi_stream_destroy": "runtime helper: hipStreamDestroy",
    "cmi_stream_synchronize": "runtime helper: hipStreamSynchronize", "cmi_stream_wait_event": "runtime helper: hipStreamWaitEvent",
}


def header_families(text):
    """{family: [suffixes]} of every declaration of the header that has a `void *stream` parameter, comments stripped;
    a family without a typed suffix has ['']."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = {}
    for name, args in re.findall(r"\b(cmi_\w+)\s*\(([^;{}()]*)\)\s*;", text, flags=re.S):
        if not re.search(r"\bvoid\s*\*\s*stream\b", args):
            continue
        m = re.match(r"(.*)_(f64|f32|i32)$", name)
        family, suffix = (m.group(1), m.group(2)) if m else (name, "")
        out.setdefault(family, []).append(suffix)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# comparison rules (each is the rule of the suite named with it)
# ------------------------------------------------------------------------------------------------------------------------------
def host(t):
    return t.cpu().numpy()


def same_bits(got, want, what):
    """Bit equality (NaN patterns included), dtype and shape included."""
    got, want = np.ascontiguousarray(host(got) if hasattr(got, "cpu") else got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype}{got.shape} against {want.dtype}{want.shape}"
    if got.tobytes() != want.tobytes():
        diff = np.flatnonzero(~((got == want) | ((got != got) & (want != want))).ravel())
        raise AssertionError(f"{what}: differs from the reference at {diff[:5].tolist()} ({len(diff)} of {got.size}): got {got.ravel()[diff[:3]]}, want {want.ravel()[diff[:3]]}")


def sum_close(dev_value, a, b, what, extra=0.0):
    """A reduction accumulated in double against math.fsum of the products: 1e-12 sum|terms| (test_blas_extra_gpu.check_sums);
    `extra`: what a final rounding of the result to float adds."""
    import blas_extra_refs as R
    exact, absolute = R.exact_sum(a, b)
    got = float(dev_value)
    assert abs(got - exact) <= 1e-12 * absolute + extra * abs(exact), f"{what}: {got!r}, exact {exact!r}, sum|terms| {absolute!r}"


def rows_close(got, exact, what):
    """Row sums formed in any order: the bound of rounding_refs.within_rounding_bound (test_rounding_gpu)."""
    import rounding_refs as RR
    got = host(got) if hasattr(got, "cpu") else got
    bad = RR.within_rounding_bound(got, *exact, got.dtype)
    assert not bad, f"{what}: {RR.describe(bad)}"


# ------------------------------------------------------------------------------------------------------------------------------
# a case
# ------------------------------------------------------------------------------------------------------------------------------
class Case:
    """One call of one entry point.  Inputs are registered with two host value sets (k = 0, 1); the tensors handed to the entry point
    (`live`) are separate from the spare device copies the GPU module stages the real values in."""

    def __init__(self, ctx, label=""):
        self.ctx, self.label = ctx, label
        self.inputs = []     # [live tensor, (host set 0, host set 1), is also an output]
        self.outputs = []    # [tensor, sentinel]
        self.mirror = None   # a HostScalar the call also writes
        self.call = None     # call(stream) -> whatever the entry point returned on the host
        self.check = None    # check(k, returned): asserts against the reference of value set k
        self.keep = []       # plans and other objects that must outlive the case

    def inp(self, a0, a1=None, output=False):
        """An input that can hold the all-zero placeholder: returns the live tensor (it holds value set 0)."""
        torch = self.ctx.torch
        a0 = np.ascontiguousarray(a0)
        a1 = a0 if a1 is None else np.ascontiguousarray(a1)
        assert a0.dtype == a1.dtype and a0.shape == a1.shape
        live = torch.from_numpy(a0.copy()).to(self.ctx.dev)
        self.inputs.append([live, (a0, a1), output])
        return live

    def inout(self, a0, a1=None):
        return self.inp(a0, a1, output=True)

    def scalar(self, v0, v1=None):
        """A 1-element float64 device scalar."""
        return self.inp(np.array([v0], np.float64), np.array([v0 if v1 is None else v1], np.float64))

    def fixed(self, a):
        """Structure a plan was made from: stays in place (a plan and its arrays must agree)."""
        t = self.ctx.torch.from_numpy(np.ascontiguousarray(a).copy()).to(self.ctx.dev)
        self.keep.append(t)   # a call may hold its bare address (hyb_plan_args): it lives as long as the case
        return t

    def out(self, n, dtype):
        torch = self.ctx.torch
        tdt = {np.float64: torch.float64, np.float32: torch.float32, np.int32: torch.int32, np.int64: torch.int64}[np.dtype(dtype).type]
        s = SENTINEL if np.dtype(dtype).kind == "f" else -7
        t = torch.full((n,) if isinstance(n, int) else tuple(n), s, dtype=tdt, device=self.ctx.dev)
        self.outputs.append([t, s])
        return t

    def host_mirror(self):
        self.mirror = self.ctx.cmi.HostScalar()
        return self.mirror

    # ---- what the GPU module drives --------------------------------------------------------------------------------------
    def mirror_value(self):
        return ctypes.c_double.from_address(self.mirror.ptr).value

    def reset_outputs(self):
        for t, s in self.outputs:
            t.fill_(s)
        if self.mirror is not None:
            ctypes.c_double.from_address(self.mirror.ptr).value = SENTINEL

    def load(self, k):
        torch = self.ctx.torch
        for live, sets, _ in self.inputs:
            live.copy_(torch.from_numpy(sets[k]))

    def placeholders(self):
        for live, _, _ in self.inputs:
            live.zero_()

    def spares(self, k=0):
        torch = self.ctx.torch
        return [torch.from_numpy(sets[k]).to(self.ctx.dev) for _, sets, _ in self.inputs]

    def queue_inputs(self, spares):
        for (live, _, _), spare in zip(self.inputs, spares):
            live.copy_(spare, non_blocking=True)

    def assert_untouched(self, k, what):
        """Nothing ran: every output holds the sentinel, every in-place operand its input, the mirror the sentinel."""
        for i, (t, s) in enumerate(self.outputs):
            assert bool((t == s).all()), f"{what}: output {i} was written"
        for i, (live, sets, output) in enumerate(self.inputs):
            if output:
                assert host(live).tobytes() == sets[k].tobytes(), f"{what}: in-place operand {i} was written"
        if self.mirror is not None:
            assert self.mirror_value() == SENTINEL, f"{what}: the host mirror was written"

    def close(self):
        if self.mirror is not None:
            self.mirror.close()
        self.keep.clear()


class Ctx:
    """What the builders share: the library, the oracle, torch, one BLAS workspace, and cached host data."""

    def __init__(self, cmi, orc, torch):
        self.cmi, self.orc, self.torch = cmi, orc, torch
        self.dev = torch.device("cuda")
        self.ws = cmi.blas_workspace()
        self._cache = {}

    def cached(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def vec(self, T, n, tag, k):
        """Value set k of a vector: cached, read-only."""
        def make():
            a = np.random.default_rng([n, k, sum(map(ord, tag))]).standard_normal(n).astype(T)
            a.setflags(write=False)
            return a
        return self.cached(("vec", T, n, tag, k), make)

    def vecs(self, T, n, tag):
        return self.vec(T, n, tag, 0), self.vec(T, n, tag, 1)

    def poisson(self, T, k, nx=NX, ny=NY):
        """poisson5pt(nx, ny)'s structure with value set k: dict(n, Ap, Aj, Ax, x, exact) -- exact: rounding_refs.exact_rows."""
        def make():
            import rounding_refs as RR
            Ap, Aj, _ = self.orc.poisson5pt_csr(nx, ny, T)
            n = nx * ny
            Ax = (np.random.default_rng([7, k, nx]).uniform(0.5, 1.5, len(Aj)) * np.where(Aj == np.repeat(np.arange(n), np.diff(Ap)), 4.0, -1.0)).astype(T)
            x = self.vec(T, n, "x", k)
            return dict(n=n, Ap=Ap, Aj=Aj, Ax=Ax, x=x, exact=RR.exact_rows(Ap, Aj, Ax, x))
        return self.cached(("poisson", T, k, nx, ny), make)

    def formats(self, T, k):
        """The same matrix in ELL (width 5), HYB (width 3: a non-empty COO part), DIA and COO, from the oracle's conversions."""
        def make():
            P, orc = self.poisson(T, k), self.orc
            pitch, eAj, eAx = orc.csr_to_ell(P["Ap"], P["Aj"], P["Ax"], 5)
            hp, hAj, hAx, cAi, cAj, cAx = orc.csr_to_hyb(P["Ap"], P["Aj"], P["Ax"], 3)
            dp, off, vals = orc.csr_to_dia(P["n"], P["n"], P["Ap"], P["Aj"], P["Ax"])
            return dict(ell=(5, pitch, eAj, eAx), hyb=(3, hp, hAj, hAx, cAi, cAj, cAx), dia=(dp, off, vals), Ai=orc.csr_row_indices(P["Ap"]))
        return self.cached(("formats", T, k), make)

    def irregular(self, T):
        """Rows of 0..9 entries and five of 100, columns unsorted: (n, Ap, Aj, Ax)."""
        def make():
            rng = np.random.default_rng(31)
            n = 3001
            lens = rng.integers(0, 10, n)
            lens[rng.choice(n, 5, replace=False)] = 100
            Ap = np.r_[0, np.cumsum(lens)].astype(np.int32)
            Aj = rng.integers(0, n, int(Ap[-1])).astype(np.int32)
            Ax = rng.standard_normal(int(Ap[-1])).astype(T)
            return n, Ap, Aj, Ax
        return self.cached(("irregular", T), make)


def _tdt(torch, T):
    return {np.float64: torch.float64, np.float32: torch.float32, np.int32: torch.int32}[T]


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _sp(stream):
    return ctypes.c_void_p(stream.cuda_stream)


# ------------------------------------------------------------------------------------------------------------------------------
# builders: the multiplies
# ------------------------------------------------------------------------------------------------------------------------------
def _csr_inputs(c, ctx, T, planned):
    """(n, Ap, Aj, Ax, x) as device tensors of the case; a planned call keeps its structure in place."""
    P0, P1 = ctx.poisson(T, 0), ctx.poisson(T, 1)
    put = c.fixed if planned else c.inp
    return P0["n"], put(P0["Ap"]), put(P0["Aj"]), c.inp(P0["Ax"], P1["Ax"]), c.inp(P0["x"], P1["x"])


def _check_y(ctx, T, y, what):
    return lambda k: rows_close(y, ctx.poisson(T, k)["exact"], f"{what}: y (value set {k})")


def b_spmv_csr(ctx, T):
    c = Case(ctx)
    n, Ap, Aj, Ax, x = _csr_inputs(c, ctx, T, False)
    y = c.out(n, T)
    c.call = lambda s: ctx.cmi.spmv_csr(n, n, Ap, Aj, Ax, x, y, stream=s)
    chk = _check_y(ctx, T, y, "spmv_csr")
    c.check = lambda k, ret: chk(k)
    return [c]


def _csr_plan(c, ctx, T, Ap, Aj, n):
    plan = ctx.cmi.Plan.csr(_tdt(ctx.torch, T), n, n, Ap, Aj)
    c.keep.append(plan)
    return plan


def b_spmv_csr_plan(ctx, T):
    c = Case(ctx)
    n, Ap, Aj, Ax, x = _csr_inputs(c, ctx, T, True)
    plan = _csr_plan(c, ctx, T, Ap, Aj, n)
    y = c.out(n, T)
    c.call = lambda s: ctx.cmi.spmv_csr_plan(plan, Ap, Aj, Ax, x, y, stream=s)
    chk = _check_y(ctx, T, y, "spmv_csr_plan")
    c.check = lambda k, ret: chk(k)
    return [c]


def b_spmm_csr(ctx, T):
    """k = 3 columns: column c has the bits of the multiply on column c, so each is held to the row bound of its own x."""
    import rounding_refs as RR
    c = Case(ctx)
    P = [ctx.poisson(T, 0), ctx.poisson(T, 1)]
    n = P[0]["n"]
    Ap, Aj, Ax = c.inp(P[0]["Ap"]), c.inp(P[0]["Aj"]), c.inp(P[0]["Ax"], P[1]["Ax"])
    Xh = [np.stack([ctx.vec(T, n, f"X{j}", k) for j in range(3)], 1) for k in (0, 1)]
    X = c.inp(Xh[0], Xh[1])
    Y = c.out((n, 3), T)
    c.call = lambda s: ctx.cmi.spmm_csr(n, n, Ap, Aj, Ax, X, Y, stream=s)

    def check(k, ret):
        got = host(Y)
        for j in range(3):
            exact = ctx.cached(("spmm exact", T, k, j), lambda: RR.exact_rows(P[k]["Ap"], P[k]["Aj"], P[k]["Ax"], Xh[k][:, j]))
            rows_close(np.ascontiguousarray(got[:, j]), exact, f"spmm_csr column {j} (value set {k})")
    c.check = check
    return [c]


def _dot_check(ctx, T, y, w_sets, res, what):
    chk = _check_y(ctx, T, y, what)

    def check(k, ret):
        chk(k)
        sum_close(res[0], host(y), w_sets[k], f"{what}: <y, w> (value set {k})")  # of the y the kernel returned, as test_spmv_gpu does
    return check


def b_spmv_csr_dot(ctx, T, planned=False):
    c = Case(ctx)
    n, Ap, Aj, Ax, x = _csr_inputs(c, ctx, T, planned)
    plan = _csr_plan(c, ctx, T, Ap, Aj, n) if planned else None
    ws_ = ctx.vecs(T, n, "w")
    w, y, res = c.inp(*ws_), c.out(n, T), c.out(1, np.float64)
    c.call = lambda s: ctx.cmi.spmv_csr_dot(n, n, Ap, Aj, Ax, x, y, w, res, ctx.ws, stream=s, plan=plan)
    c.check = _dot_check(ctx, T, y, ws_, res, "spmv_csr_dot_plan" if planned else "spmv_csr_dot")
    return [c]


def b_spmv_csr_dot_plan(ctx, T):
    return b_spmv_csr_dot(ctx, T, planned=True)


def _ell_inputs(c, ctx, T):
    F = [ctx.formats(T, 0), ctx.formats(T, 1)]
    width, pitch, eAj, eAx = F[0]["ell"]
    return width, pitch, c.inp(eAj), c.inp(eAx, F[1]["ell"][3])


def b_spmv_ell(ctx, T):
    c = Case(ctx)
    n = ctx.poisson(T, 0)["n"]
    width, pitch, eAj, eAx = _ell_inputs(c, ctx, T)
    x, y = c.inp(*ctx.vecs(T, n, "x")), c.out(n, T)
    c.call = lambda s: ctx.cmi.spmv_ell(n, n, width, pitch, eAj, eAx, x, y, stream=s)
    chk = _check_y(ctx, T, y, "spmv_ell")
    c.check = lambda k, ret: chk(k)
    return [c]


def b_spmv_ell_dot(ctx, T):
    c = Case(ctx)
    n = ctx.poisson(T, 0)["n"]
    width, pitch, eAj, eAx = _ell_inputs(c, ctx, T)
    ws_ = ctx.vecs(T, n, "w")
    x, w, y, res = c.inp(*ctx.vecs(T, n, "x")), c.inp(*ws_), c.out(n, T), c.out(1, np.float64)
    c.call = lambda s: ctx.cmi.spmv_ell_dot(n, n, width, pitch, eAj, eAx, x, y, w, res, ctx.ws, stream=s)
    c.check = _dot_check(ctx, T, y, ws_, res, "spmv_ell_dot")
    return [c]


def _dia_inputs(c, ctx, T):
    F = [ctx.formats(T, 0), ctx.formats(T, 1)]
    pitch, off, vals = F[0]["dia"]
    return len(off), pitch, c.inp(off), c.inp(vals, F[1]["dia"][2])


def b_spmv_dia(ctx, T):
    c = Case(ctx)
    n = ctx.poisson(T, 0)["n"]
    nd, pitch, off, vals = _dia_inputs(c, ctx, T)
    x, y = c.inp(*ctx.vecs(T, n, "x")), c.out(n, T)
    c.call = lambda s: ctx.cmi.spmv_dia(n, n, nd, pitch, off, vals, x, y, stream=s)
    chk = _check_y(ctx, T, y, "spmv_dia")
    c.check = lambda k, ret: chk(k)
    return [c]


def b_spmv_dia_dot(ctx, T):
    c = Case(ctx)
    n = ctx.poisson(T, 0)["n"]
    nd, pitch, off, vals = _dia_inputs(c, ctx, T)
    ws_ = ctx.vecs(T, n, "w")
    x, w, y, res = c.inp(*ctx.vecs(T, n, "x")), c.inp(*ws_), c.out(n, T), c.out(1, np.float64)
    c.call = lambda s: ctx.cmi.spmv_dia_dot(n, n, nd, pitch, off, vals, x, y, w, res, ctx.ws, stream=s)
    c.check = _dot_check(ctx, T, y, ws_, res, "spmv_dia_dot")
    return [c]


def _coo_inputs(c, ctx, T, planned):
    P0, P1 = ctx.poisson(T, 0), ctx.poisson(T, 1)
    put = c.fixed if planned else c.inp
    return P0["n"], put(ctx.formats(T, 0)["Ai"]), put(P0["Aj"]), c.inp(P0["Ax"], P1["Ax"]), c.inp(P0["x"], P1["x"])


def b_spmv_coo(ctx, T):
    c = Case(ctx)
    n, Ai, Aj, Ax, x = _coo_inputs(c, ctx, T, False)
    y = c.out(n, T)
    c.call = lambda s: ctx.cmi.spmv_coo(n, n, Ai, Aj, Ax, x, y, stream=s)
    chk = _check_y(ctx, T, y, "spmv_coo")
    c.check = lambda k, ret: chk(k)
    return [c]


def _coo_plan(c, ctx, T, n, Ai, Aj):
    plan = ctx.cmi.Plan.coo(_tdt(ctx.torch, T), n, n, Ai, Aj)
    c.keep.append(plan)
    return plan


def b_spmv_coo_plan(ctx, T):
    c = Case(ctx)
    n, Ai, Aj, Ax, x = _coo_inputs(c, ctx, T, True)
    plan = _coo_plan(c, ctx, T, n, Ai, Aj)
    y = c.out(n, T)
    c.call = lambda s: ctx.cmi.spmv_coo_plan(plan, Ai, Aj, Ax, x, y, stream=s)
    chk = _check_y(ctx, T, y, "spmv_coo_plan")
    c.check = lambda k, ret: chk(k)
    return [c]


def b_spmv_coo_dot_plan(ctx, T):
    c = Case(ctx)
    n, Ai, Aj, Ax, x = _coo_inputs(c, ctx, T, True)
    plan = _coo_plan(c, ctx, T, n, Ai, Aj)
    ws_ = ctx.vecs(T, n, "w")
    w, y, res = c.inp(*ws_), c.out(n, T), c.out(1, np.float64)
    c.call = lambda s: ctx.cmi.binding.spmv_coo_dot_plan(plan, Ai, Aj, Ax, x, y, w, res, ctx.ws, stream=s)
    c.check = _dot_check(ctx, T, y, ws_, res, "spmv_coo_dot_plan")
    return [c]


def _hyb_inputs(c, ctx, T, planned, reverse=False):
    """reverse: the COO part in descending row order (unsorted: a plan then takes the two-launch form)."""
    F = [ctx.formats(T, 0), ctx.formats(T, 1)]
    width, pitch, hAj, hAx, cAi, cAj, cAx = F[0]["hyb"]
    assert len(cAi) > 0, "the COO part must not be empty"
    put = c.fixed if planned else c.inp
    o = slice(None, None, -1) if reverse else slice(None)
    return width, pitch, put(hAj), c.inp(hAx, F[1]["hyb"][3]), put(cAi[o]), put(cAj[o]), c.inp(cAx[o], F[1]["hyb"][6][o])


def b_spmv_hyb(ctx, T):
    """Plan-less HYB is two launches: the ELL kernel, then the COO kernel accumulating."""
    c = Case(ctx)
    n = ctx.poisson(T, 0)["n"]
    width, pitch, hAj, hAx, cAi, cAj, cAx = _hyb_inputs(c, ctx, T, False)
    x, y = c.inp(*ctx.vecs(T, n, "x")), c.out(n, T)
    c.call = lambda s: ctx.cmi.spmv_hyb(n, n, width, pitch, hAj, hAx, cAi, cAj, cAx, x, y, stream=s)
    chk = _check_y(ctx, T, y, "spmv_hyb")
    c.check = lambda k, ret: chk(k)
    return [c]


def _hyb_plan(c, ctx, T, n, width, cAi, launches):
    """A plan that runs `launches` launches: 1 for the sorted, light COO part, 2 for the same part in descending row order."""
    plan = ctx.cmi.Plan.hyb(_tdt(ctx.torch, T), n, n, width, cAi)
    c.keep.append(plan)
    assert plan.hyb_launches() == launches, f"the HYB plan runs {plan.hyb_launches()} launches, the case is about {launches}"
    return plan


def b_spmv_hyb_plan(ctx, T):
    out = []
    for which in (0, 1):
        c = Case(ctx, ("one launch", "two launches")[which])
        n = ctx.poisson(T, 0)["n"]
        width, pitch, hAj, hAx, cAi, cAj, cAx = _hyb_inputs(c, ctx, T, True, reverse=bool(which))
        plan = _hyb_plan(c, ctx, T, n, width, cAi, which + 1)
        x, y = c.inp(*ctx.vecs(T, n, "x")), c.out(n, T)
        c.call = lambda s, plan=plan, a=(pitch, hAj, hAx, cAi, cAj, cAx), x=x, y=y: ctx.cmi.spmv_hyb_plan(plan, *a, x, y, stream=s)
        chk = _check_y(ctx, T, y, "spmv_hyb_plan")
        c.check = lambda k, ret, chk=chk: chk(k)
        out.append(c)
    return out


def b_spmv_hyb_dot_plan(ctx, T):
    out = []
    for which in (0, 1):
        c = Case(ctx, ("one launch", "two launches")[which])
        n = ctx.poisson(T, 0)["n"]
        width, pitch, hAj, hAx, cAi, cAj, cAx = _hyb_inputs(c, ctx, T, True, reverse=bool(which))
        plan = _hyb_plan(c, ctx, T, n, width, cAi, which + 1)
        args = ctx.cmi.binding.hyb_plan_args(plan, pitch, hAj, hAx, cAi, cAj, cAx)
        ws_ = ctx.vecs(T, n, "w")
        x, w, y, res = c.inp(*ctx.vecs(T, n, "x")), c.inp(*ws_), c.out(n, T), c.out(1, np.float64)
        c.call = lambda s, args=args, x=x, y=y, w=w, res=res: ctx.cmi.binding.spmv_hyb_dot_plan_args(args, x, y, w, res, ctx.ws, stream=s)
        c.check = _dot_check(ctx, T, y, ws_, res, "spmv_hyb_dot_plan")
        out.append(c)
    return out


# ---- the semiring multiplies: (plus, minimum) -- min-plus, nothing a plain multiply could stand in for -------------------------------
def _semiring(ctx, T, fmt):
    import semiring_refs as S
    c = Case(ctx)
    P = [ctx.poisson(T, 0, 29, 23), ctx.poisson(T, 1, 29, 23)]   # the loops of semiring_refs are plain Python: 667 rows, 3 workgroups
    n = P[0]["n"]
    orc, cmi = ctx.orc, ctx.cmi
    y0s = ctx.vecs(T, n, "y0")
    x, y0, y = c.inp(P[0]["x"], P[1]["x"]), c.inp(*y0s), c.out(n, T)
    if fmt == "csr":
        Ap, Aj, Ax = c.inp(P[0]["Ap"]), c.inp(P[0]["Aj"]), c.inp(P[0]["Ax"], P[1]["Ax"])
        c.call = lambda s: cmi.spmv_csr_semiring(n, n, Ap, Aj, Ax, x, y, "plus", "minimum", y0=y0, stream=s)
        ref = lambda k: S.semiring_csr(P[k]["Ap"], P[k]["Aj"], P[k]["Ax"], P[k]["x"], "plus", "minimum", y0=y0s[k])  # noqa: E731
    elif fmt == "coo":
        Aih = orc.csr_row_indices(P[0]["Ap"])
        Ai, Aj, Ax = c.inp(Aih), c.inp(P[0]["Aj"]), c.inp(P[0]["Ax"], P[1]["Ax"])
        c.call = lambda s: cmi.spmv_coo_semiring(n, n, Ai, Aj, Ax, x, y, "plus", "minimum", y0=y0, stream=s)
        ref = lambda k: S.semiring_coo(n, Aih, P[k]["Aj"], P[k]["Ax"], P[k]["x"], "plus", "minimum", y0=y0s[k])  # noqa: E731
    elif fmt == "ell":
        E = [orc.csr_to_ell(P[k]["Ap"], P[k]["Aj"], P[k]["Ax"], 5) for k in (0, 1)]
        pitch = E[0][0]
        eAj, eAx = c.inp(E[0][1]), c.inp(E[0][2], E[1][2])
        c.call = lambda s: cmi.spmv_ell_semiring(n, n, 5, pitch, eAj, eAx, x, y, "plus", "minimum", y0=y0, stream=s)
        ref = lambda k: S.semiring_ell(n, 5, pitch, E[k][1], E[k][2], P[k]["x"], "plus", "minimum", y0=y0s[k])  # noqa: E731
    else:
        D = [orc.csr_to_dia(n, n, P[k]["Ap"], P[k]["Aj"], P[k]["Ax"]) for k in (0, 1)]
        pitch, offh = D[0][0], D[0][1]
        off, vals = c.inp(offh), c.inp(D[0][2], D[1][2])
        c.call = lambda s: cmi.spmv_dia_semiring(n, n, len(offh), pitch, off, vals, x, y, "plus", "minimum", y0=y0, stream=s)
        ref = lambda k: S.semiring_dia(n, n, pitch, offh, D[k][2], P[k]["x"], "plus", "minimum", y0=y0s[k])  # noqa: E731
    c.check = lambda k, ret: same_bits(y, ctx.cached(("semiring", fmt, T, k), lambda: ref(k)), f"spmv_{fmt}_semiring (value set {k})")
    return [c]


b_spmv_csr_semiring = functools.partial(_semiring, fmt="csr")
b_spmv_coo_semiring = functools.partial(_semiring, fmt="coo")
b_spmv_ell_semiring = functools.partial(_semiring, fmt="ell")
b_spmv_dia_semiring = functools.partial(_semiring, fmt="dia")


# ---- the epilogue sweeps and the Gauss-Seidel colour call ------------------------------------------------------------------------------
def _small(ctx, T, k):
    return ctx.poisson(T, k, 29, 23)      # relaxation_refs.row_sums and gauss_seidel_refs are plain Python loops


def b_spmv_csr_axpby(ctx, T):
    import relaxation_refs as X
    c = Case(ctx)
    P = [_small(ctx, T, 0), _small(ctx, T, 1)]
    n = P[0]["n"]
    Ap, Aj, Ax, x = c.inp(P[0]["Ap"]), c.inp(P[0]["Aj"]), c.inp(P[0]["Ax"], P[1]["Ax"]), c.inp(P[0]["x"], P[1]["x"])
    zs = ctx.vecs(T, n, "z")
    z, out = c.inp(*zs), c.out(n, T)
    alpha, beta = float(T(-1.75 / 0.6)), float(T(0.7 / 1.3))
    c.call = lambda s: ctx.cmi.spmv_csr_axpby(n, n, Ap, Aj, Ax, x, alpha, beta, z, out, stream=s)
    c.check = lambda k, ret: same_bits(out, X.spmv_axpby(P[k]["Ap"], P[k]["Aj"], P[k]["Ax"], P[k]["x"], alpha, beta, zs[k]), f"spmv_csr_axpby (value set {k})")
    return [c]


def b_csr_jacobi_sweep(ctx, T):
    import relaxation_refs as X
    c = Case(ctx)
    P = [_small(ctx, T, 0), _small(ctx, T, 1)]
    n = P[0]["n"]
    Ap, Aj, Ax, x = c.inp(P[0]["Ap"]), c.inp(P[0]["Aj"]), c.inp(P[0]["Ax"], P[1]["Ax"]), c.inp(P[0]["x"], P[1]["x"])
    ds = [X.extract_diagonal(P[k]["Ap"], P[k]["Aj"], P[k]["Ax"]) for k in (0, 1)]
    bs = ctx.vecs(T, n, "b")
    diag, b, out = c.inp(*ds), c.inp(*bs), c.out(n, T)
    omega = float(T(2.0 / 3.0))
    c.call = lambda s: ctx.cmi.csr_jacobi_sweep(n, Ap, Aj, Ax, diag, b, x, omega, out, stream=s)
    c.check = lambda k, ret: same_bits(out, X.jacobi_sweep(P[k]["Ap"], P[k]["Aj"], P[k]["Ax"], ds[k], bs[k], P[k]["x"], omega), f"csr_jacobi_sweep (value set {k})")
    return [c]


def b_relax_jacobi_update(ctx, T):
    import relaxation_refs as X
    c = Case(ctx)
    ds = tuple((np.abs(ctx.vec(T, N1, "d", k)) + T(1)).astype(T) for k in (0, 1))
    bs, ys, xs = ctx.vecs(T, N1, "b"), ctx.vecs(T, N1, "y"), ctx.vecs(T, N1, "x")
    diag, b, y, x = c.inp(*ds), c.inp(*bs), c.inp(*ys), c.inout(*xs)
    omega = float(T(2.0 / 3.0))
    c.call = lambda s: ctx.cmi.relax_jacobi_update(diag, b, y, omega, x, stream=s)
    c.check = lambda k, ret: same_bits(x, X.epilogue_jacobi(ys[k], xs[k], bs[k], ds[k], omega), f"relax_jacobi_update (value set {k})")
    return [c]


def b_csr_gauss_seidel_colour(ctx, T):
    """Both forms on the first colour of the greedy colouring: one launch, and -- on a slot range that spans two colours, so that rows of
    the range do hold columns of the range -- the parked two-launch form."""
    import gauss_seidel_refs as G
    P = [_small(ctx, T, 0), _small(ctx, T, 1)]
    n = P[0]["n"]
    colors, num_colors = G.vertex_coloring(P[0]["Ap"], P[0]["Aj"])
    ordering, offsets = G.schedule(colors, num_colors)
    out = []
    for parked in (False, True):
        c = Case(ctx, "parked two-launch" if parked else "one launch")
        s0, s1 = (int(offsets[0]), int(offsets[2])) if parked else (int(offsets[0]), int(offsets[1]))
        Ap, Aj, Ax = c.inp(P[0]["Ap"]), c.inp(P[0]["Aj"]), c.inp(P[0]["Ax"], P[1]["Ax"])
        bs, xs = ctx.vecs(T, n, "b"), (P[0]["x"], P[1]["x"])
        b, x, order = c.inp(*bs), c.inout(*xs), c.inp(ordering)
        scratch = c.out(s1 - s0, T) if parked else None
        c.outputs = [o for o in c.outputs if o[0] is not scratch]   # scratch is scratch: what it holds afterwards is not specified
        c.call = lambda s, a=(Ap, Aj, Ax, b, x, order, s0, s1, scratch): ctx.cmi.csr_gauss_seidel_colour(n, *a[:7], a[7], scratch=a[8], stream=s)
        c.check = lambda k, ret, x=x, r=(s0, s1, parked), bs=bs, xs=xs: same_bits(
            x, G.relax_slots(P[k]["Ap"], P[k]["Aj"], P[k]["Ax"], bs[k], np.array(xs[k]), ordering, r[0], r[1], parked=r[2]),
            f"csr_gauss_seidel_colour {'parked' if r[2] else 'one launch'} (value set {k})")
        out.append(c)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# builders: BLAS-1 and the fused solver steps
# ------------------------------------------------------------------------------------------------------------------------------
def _vec_case(ctx, T, names, outputs):
    c = Case(ctx)
    sets = {nm: ctx.vecs(T, N1, nm) for nm in names}
    dev = {nm: (c.inout if nm in outputs else c.inp)(*sets[nm]) for nm in names}
    return c, sets, dev


def b_blas_axpy(ctx, T):
    c, v, d = _vec_case(ctx, T, ("x", "y"), ("y",))
    c.call = lambda s: ctx.cmi.blas_axpy(0.75, d["x"], d["y"], stream=s)
    c.check = lambda k, ret: same_bits(d["y"], T(0.75) * v["x"][k] + v["y"][k], f"blas_axpy (value set {k})")   # test_blas1
    return [c]


def b_blas_axpby(ctx, T):
    c, v, d = _vec_case(ctx, T, ("x", "y"), ())
    z = c.out(N1, T)
    c.call = lambda s: ctx.cmi.blas_axpby(2.0, d["x"], -0.5, d["y"], z, stream=s)
    c.check = lambda k, ret: same_bits(z, T(2.0) * v["x"][k] + T(-0.5) * v["y"][k], f"blas_axpby (value set {k})")
    return [c]


def b_blas_copy(ctx, T):
    c, v, d = _vec_case(ctx, T, ("x",), ())
    y = c.out(N1, T)
    c.call = lambda s: ctx.cmi.blas_copy(d["x"], y, stream=s)
    c.check = lambda k, ret: same_bits(y, v["x"][k], f"blas_copy (value set {k})")
    return [c]


def b_blas_fill(ctx, T):
    c = Case(ctx)
    y = c.out(N1, T)
    c.call = lambda s: ctx.cmi.blas_fill(3.25, y, stream=s)
    c.check = lambda k, ret: same_bits(y, np.full(N1, 3.25, T), "blas_fill")
    return [c]


def b_blas_dot(ctx, T):
    c, v, d = _vec_case(ctx, T, ("x", "y"), ())
    res = c.out(1, T)
    c.call = lambda s: ctx.cmi.blas_dot(d["x"], d["y"], res, ctx.ws, stream=s)

    def check(k, ret):
        x, y = v["x"][k].astype(np.float64), v["y"][k].astype(np.float64)
        tol = 1e-12 if T is np.float64 else 1e-6   # test_blas1's bars
        assert abs(float(res[0]) - float(np.dot(x, y))) <= tol * float(np.abs(x * y).sum()), f"blas_dot (value set {k}): {float(res[0])!r}"
    c.check = check
    return [c]


def b_blas_nrm2(ctx, T):
    c, v, d = _vec_case(ctx, T, ("x",), ())
    res = c.out(1, T)
    c.call = lambda s: ctx.cmi.blas_nrm2(d["x"], res, ctx.ws, stream=s)

    def check(k, ret):
        want = float(np.linalg.norm(v["x"][k].astype(np.float64)))
        assert abs(float(res[0]) - want) <= (1e-12 if T is np.float64 else 1e-6) * want, f"blas_nrm2 (value set {k}): {float(res[0])!r} against {want!r}"
    c.check = check
    return [c]


def b_blas_dotd(ctx, T):
    c, v, d = _vec_case(ctx, T, ("x", "y"), ())
    res = c.out(1, np.float64)
    c.call = lambda s: ctx.cmi.blas_dotd(d["x"], d["y"], res, ctx.ws, stream=s)
    c.check = lambda k, ret: sum_close(res[0], v["x"][k], v["y"][k], f"blas_dotd (value set {k})")
    return [c]


def b_blas_asum(ctx, T):
    c, v, d = _vec_case(ctx, T, ("x",), ())
    res = c.out(1, T)
    c.call = lambda s: ctx.cmi.blas_asum(d["x"], res, ctx.ws, stream=s)
    c.check = lambda k, ret: sum_close(res[0], np.abs(v["x"][k]), np.ones(N1), f"blas_asum (value set {k})", extra=0.0 if T is np.float64 else 2.0 ** -24)
    return [c]


def b_blas_amax(ctx, T):
    import blas_extra_refs as R
    c, v, d = _vec_case(ctx, T, ("x",), ())
    value, index = c.out(1, T), c.out(1, np.int64)
    c.call = lambda s: ctx.cmi.blas_amax(d["x"], value, index, ctx.ws, stream=s)

    def check(k, ret):
        best, at = R.amax_ref_fast(v["x"][k])
        assert (float(value[0]), int(index[0])) == (best, at), f"blas_amax (value set {k}): {(float(value[0]), int(index[0]))} against {(best, at)}"
    c.check = check
    return [c]


# the twelve kernels of blas_extra_refs.KERNELS: name -> (header family, adapter(cmi, scalars, operands, results, ws, mirror, stream))
_EXTRA = {
    "scal": ("cmi_blas_scal", lambda cmi, s, o, r, ws, m, st: cmi.blas_scal(s["a"], o["x"], stream=st)),
    "xmy": ("cmi_blas_xmy", lambda cmi, s, o, r, ws, m, st: cmi.blas_xmy(o["x"], o["y"], o["z"], stream=st)),
    "axpbypcz": ("cmi_blas_axpbypcz", lambda cmi, s, o, r, ws, m, st: cmi.blas_axpbypcz(s["a"], o["x"], s["b"], o["y"], s["c"], o["z"], o["out"], stream=st)),
    "pcg_update": ("cmi_pcg_update_jacobi", lambda cmi, s, o, r, ws, m, st: cmi.pcg_update_jacobi(s["rz"], s["yp"], o["y"], o["r"], o["dinv"], r["rz_new"], r["rr"], ws, stream=st, mirror=m)),
    "pcg_direction": ("cmi_pcg_direction_x_jacobi", lambda cmi, s, o, r, ws, m, st: cmi.pcg_direction_x_jacobi(s["rz_new"], s["rz_old"], s["yp"], o["r"], o["dinv"], o["p"], o["x"], stream=st)),
    "bicg_s": ("cmi_bicgstab_s", lambda cmi, s, o, r, ws, m, st: cmi.bicgstab_s(s["rho"], s["d1"], o["r"], o["AMp"], o["s"], r["ss"], ws, stream=st, mirror=m)),
    "bicg_xr": ("cmi_bicgstab_xr", lambda cmi, s, o, r, ws, m, st: cmi.bicgstab_xr(s["rho"], s["d1"], s["d2"], s["d3"], o["p"], o["s"], o["AMs"], o["r_star"], o["x"], o["r"], r["rho_new"], r["rr"], ws, stream=st, mirror=m)),
    "bicg_p": ("cmi_bicgstab_p", lambda cmi, s, o, r, ws, m, st: cmi.bicgstab_p(s["rho_new"], s["rho"], s["d1"], s["d2"], s["d3"], o["r"], o["AMp"], o["p"], stream=st)),
    "cr_xr": ("cmi_cr_xr", lambda cmi, s, o, r, ws, m, st: cmi.cr_xr(s["rz"], s["yy"], o["p"], o["y"], o["x"], o["r"], r["rr"], ws, stream=st, mirror=m)),
    "cr_py": ("cmi_cr_py", lambda cmi, s, o, r, ws, m, st: cmi.cr_py(s["rz_new"], s["rz"], o["r"], o["Ar"], o["p"], o["y"], r["yy_new"], ws, stream=st)),
    "axpy_dot": ("cmi_blas_axpy_dot", lambda cmi, s, o, r, ws, m, st: cmi.blas_axpy_dot(s["h"], o["v"], o["w"], o["u"], r["out"], ws, stream=st)),
    "axpy_ratio": ("cmi_blas_axpy_ratio", lambda cmi, s, o, r, ws, m, st: cmi.blas_axpy_ratio(s["num"], s["den"], o["x"], o["y"], stream=st)),
}
_EXTRA_RESULTS = {"pcg_update": ("rz_new", "rr"), "bicg_s": ("ss",), "bicg_xr": ("rho_new", "rr"), "cr_xr": ("rr",), "cr_py": ("yy_new",), "axpy_dot": ("out",)}
_EXTRA_MIRRORED = {"pcg_update": "rr", "bicg_s": "ss", "bicg_xr": "rr", "cr_xr": "rr"}


def _table_case(ctx, T, kernel, adapter, scalar_sets, results, mirrored, what):
    """A kernel described by a blas_extra_refs.Kernel: the restatement bit for bit, the reductions against math.fsum of the vectors the
    kernel returned, the host mirror equal to its device scalar."""
    c = Case(ctx)
    sets = {nm: ctx.vecs(T, N1, nm) for nm in kernel.vecs}
    if "dinv" in sets:
        sets["dinv"] = tuple((T(1) / (np.abs(a) + T(1))).astype(T) for a in sets["dinv"])
    o = {nm: (c.inout if nm in kernel.outputs else c.inp)(*sets[nm]) for nm in kernel.vecs}
    if kernel.by_value:
        sdev = scalar_sets[0]          # by value: fixed at the call (a capture records them, as it records every by-value argument)
        scalar_sets = (scalar_sets[0], scalar_sets[0])
    else:
        sdev = {nm: c.scalar(scalar_sets[0][nm], scalar_sets[1][nm]) for nm in kernel.scalars}
    res = {nm: c.out(1, np.float64) for nm in results}
    m = c.host_mirror() if mirrored else None
    c.call = lambda st: adapter(ctx.cmi, sdev, o, res, ctx.ws, m, st)

    def check(k, ret):
        v = {nm: sets[nm][k] for nm in kernel.vecs}
        want = kernel.restate(T, scalar_sets[k], v)
        got = {nm: host(o[nm]) for nm in kernel.outputs}
        for nm in kernel.outputs:
            same_bits(got[nm], want[nm], f"{what}: {nm} (value set {k})")
        for rn, (a, b) in kernel.sums(T, got, v).items():
            if rn in res:
                sum_close(res[rn][0], a, b, f"{what}: {rn} (value set {k})")
        if m is not None:
            assert c.mirror_value() == float(res[mirrored][0]), f"{what}: the host mirror {c.mirror_value()!r} differs from the device scalar"
    c.check = check
    return [c]


def _extra(ctx, T, name):
    import blas_extra_refs as R
    kernel = R.KERNELS[name]
    return _table_case(ctx, T, kernel, _EXTRA[name][1], (R.scalars_for(kernel, "inexact", T), R.scalars_for(kernel, "exact", T)),
                       _EXTRA_RESULTS.get(name, ()), _EXTRA_MIRRORED.get(name), name)


_LOBPCG = {
    "residual": lambda cmi, s, o, r, ws, m, st: cmi.lobpcg_residual(s["lambda"], o["x"], o["ax"], o["r"], r["rr"], ws, stream=st, mirror=m),
    "gram": lambda cmi, s, o, r, ws, m, st: cmi.lobpcg_gram(s["pp"], o["x"], o["w"], o["aw"], o["p"], o["ap"], r["gram"], ws, stream=st),
    "update": lambda cmi, s, o, r, ws, m, st: cmi.lobpcg_update(s["cx"], s["cr"], s["cp"], False, s["lambda_new"], o["w"], o["aw"], o["p"], o["ap"], o["x"], o["ax"], o["r"],
                                                                 r["scalars"], ws, stream=st, mirror=m),
}


def _lobpcg(ctx, T, name):
    """The three kernels of csrc/lobpcg.hip through lobpcg_refs.KERNELS; gram's eight sums and update's two live in one result tensor."""
    import lobpcg_refs as L
    kernel = L.KERNELS[name]
    c = Case(ctx)
    sets = {nm: ctx.vecs(T, N1, nm) for nm in kernel.vecs}
    o = {nm: (c.inout if nm in kernel.outputs else c.inp)(*sets[nm]) for nm in kernel.vecs}
    ssets = (L.scalars_for(kernel, "inexact", T), L.scalars_for(kernel, "exact", T))
    if kernel.by_value:
        ssets = (ssets[0], ssets[0])
        sdev = ssets[0]
    else:
        sdev = {nm: c.scalar(ssets[0][nm], ssets[1][nm]) for nm in kernel.scalars}
    layout = {"residual": ("rr",), "gram": L.GRAM_SUMS, "update": ("rr", "pp")}[name]
    block = c.out(len(layout), np.float64)
    res = {"rr": block, "gram": block, "scalars": block}
    m = c.host_mirror() if name in ("residual", "update") else None
    c.call = lambda st: _LOBPCG[name](ctx.cmi, sdev, o, res, ctx.ws, m, st)

    def check(k, ret):
        v = {nm: sets[nm][k] for nm in kernel.vecs}
        want = kernel.restate(T, ssets[k], v)
        got = {nm: host(o[nm]) for nm in kernel.outputs}
        for nm in kernel.outputs:
            same_bits(got[nm], want[nm], f"lobpcg_{name}: {nm} (value set {k})")
        sums = kernel.sums(T, got, v)
        values = host(block)
        for i, rn in enumerate(layout):
            sum_close(values[i], *sums[rn], f"lobpcg_{name}: {rn} (value set {k})")
        if m is not None:
            assert c.mirror_value() == float(values[0]), f"lobpcg_{name}: the host mirror differs from the device scalar"
    c.check = check
    return [c]


def _cg_scalars(c):
    return c.scalar(1.75, 3.0), c.scalar(0.6, -1.5)   # rz, yp: an inexact and an exact quotient


def _q(T, num, den):
    return T(np.float64(num) / np.float64(den))


def b_cg_update(ctx, T):
    """x += alpha p; r = (-alpha) y + r; rr = <r, r>, also to the host mirror (test_cg_update_long_partial_list's expressions)."""
    c, v, d = _vec_case(ctx, T, ("p", "y", "x", "r"), ("x", "r"))
    rz, yp = _cg_scalars(c)
    rr, m = c.out(1, np.float64), c.host_mirror()
    c.call = lambda s: ctx.cmi.cg_update(rz, yp, d["p"], d["y"], d["x"], d["r"], rr, ctx.ws, stream=s, mirror=m)

    def check(k, ret):
        alpha = _q(T, *((1.75, 0.6), (3.0, -1.5))[k])
        r_new = (-alpha) * v["y"][k] + v["r"][k]
        same_bits(d["x"], alpha * v["p"][k] + v["x"][k], f"cg_update: x (value set {k})")
        same_bits(d["r"], r_new, f"cg_update: r (value set {k})")
        sum_close(rr[0], r_new, r_new, f"cg_update: rr (value set {k})")
        assert c.mirror_value() == float(rr[0]), "cg_update: the host mirror differs from the device scalar"
    c.check = check
    return [c]


def b_cg_direction(ctx, T, with_x=False):
    names = ("r", "p", "x") if with_x else ("r", "p")
    c, v, d = _vec_case(ctx, T, names, names[1:])
    rr_new, rr_old, yp = c.scalar(0.9, 0.75), c.scalar(1.75, 3.0), c.scalar(0.6, -1.5)
    if with_x:
        c.call = lambda s: ctx.cmi.cg_direction_x(rr_new, rr_old, yp, d["r"], d["p"], d["x"], stream=s)
    else:
        c.call = lambda s: ctx.cmi.cg_direction(rr_new, rr_old, d["r"], d["p"], stream=s)

    def check(k, ret):
        new, old, ypv = ((0.9, 1.75, 0.6), (0.75, 3.0, -1.5))[k]
        beta, alpha = _q(T, new, old), _q(T, old, ypv)
        what = "cg_direction_x" if with_x else "cg_direction"
        if with_x:
            same_bits(d["x"], alpha * v["p"][k] + v["x"][k], f"{what}: x (value set {k})")
        same_bits(d["p"], T(1) * v["r"][k] + beta * v["p"][k], f"{what}: p (value set {k})")
    c.check = check
    return [c]


def b_cg_direction_x(ctx, T):
    return b_cg_direction(ctx, T, with_x=True)


# ---- the fold-ahead forms: each consumes the partial list its producer left in the workspace, so the workspace is an input.  Its contents
# are prepared by running the producers once per value set while the case is built; the references are the sums of THOSE partials. ---------
def _fold_chain(ctx, T):
    """Per value set: the workspace after the partials call (ws1) and after the update fold (ws2), with the vectors in between."""
    def make():
        cmi, torch = ctx.cmi, ctx.torch
        sets = []
        P0 = ctx.poisson(T, 0)
        n = P0["n"]
        Ap, Aj = (torch.from_numpy(P0[a].copy()).to(ctx.dev) for a in ("Ap", "Aj"))
        plan = cmi.Plan.csr(_tdt(torch, T), n, n, Ap, Aj)
        for k in (0, 1):
            P = ctx.poisson(T, k)
            to = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to(ctx.dev)  # noqa: E731
            ws = cmi.blas_workspace()
            ws.zero_()
            y = torch.empty(n, dtype=_tdt(torch, T), device=ctx.dev)
            w = ctx.vec(T, n, "w", k)
            np_yp = cmi.binding.spmv_csr_dot_partials(plan, Ap, Aj, to(P["Ax"]), to(P["x"]), y, to(w), ws)
            assert np_yp > 0, "the plan's kernel cannot fuse the dot: no partial list to fold"
            torch.cuda.synchronize()
            ws1, yh = host(ws).copy(), host(y).copy()
            r0 = ctx.vec(T, n, "r", k)
            r, yp = to(r0), torch.zeros(1, dtype=torch.float64, device=ctx.dev)
            rz = (1.75, 3.0)[k]
            np_rr = cmi.binding.cg_update_fold(to(np.array([rz])), yp, np_yp, y, r, ws)
            torch.cuda.synchronize()
            sets.append(dict(ws1=ws1, y=yh, w=w, np_yp=np_yp, r0=r0, rz=rz, ws2=host(ws).copy(), r1=host(r).copy(), yp=float(yp[0]), np_rr=np_rr))
        assert sets[0]["np_yp"] == sets[1]["np_yp"] and sets[0]["np_rr"] == sets[1]["np_rr"]
        return n, sets
    return ctx.cached(("fold chain", T), make)


def b_spmv_csr_dot_plan_partials(ctx, T):
    c = Case(ctx)
    n, Ap, Aj, Ax, x = _csr_inputs(c, ctx, T, True)
    plan = _csr_plan(c, ctx, T, Ap, Aj, n)
    ws_ = ctx.vecs(T, n, "w")
    w, y = c.inp(*ws_), c.out(n, T)
    ws = ctx.cmi.blas_workspace()
    c.keep.append(ws)
    c.call = lambda s: ctx.cmi.binding.spmv_csr_dot_partials(plan, Ap, Aj, Ax, x, y, w, ws, stream=s)
    chk = _check_y(ctx, T, y, "spmv_csr_dot_plan_partials")

    def check(k, ret):
        assert ret > 0, "no partials: the plan's kernel cannot fuse the dot"   # (a word of the plan, not a device read)
        chk(k)
        partials = host(ws)[:ret]
        exact, absolute = __import__("blas_extra_refs").exact_sum(host(y), ws_[k])
        assert abs(math.fsum(partials.tolist()) - exact) <= 1e-12 * absolute, f"spmv_csr_dot_plan_partials: the {ret} partials do not add up to <y, w> (value set {k})"
    c.check = check
    return [c]


def b_cg_update_fold(ctx, T):
    n, S = _fold_chain(ctx, T)
    c = Case(ctx)
    ws = c.inout(S[0]["ws1"], S[1]["ws1"])
    rz, y, r = c.scalar(S[0]["rz"], S[1]["rz"]), c.inp(S[0]["y"], S[1]["y"]), c.inout(S[0]["r0"], S[1]["r0"])
    yp = c.out(1, np.float64)
    np_yp = S[0]["np_yp"]
    c.call = lambda s: ctx.cmi.binding.cg_update_fold(rz, yp, np_yp, y, r, ws, stream=s)

    def check(k, ret):
        partials = S[k]["ws1"][:np_yp].tolist()
        got_yp = float(yp[0])
        assert abs(got_yp - math.fsum(partials)) <= 1e-12 * math.fsum(map(abs, partials)), f"cg_update_fold: yp {got_yp!r} is not the sum of the partials (value set {k})"
        alpha = _q(T, S[k]["rz"], got_yp)
        r_new = (-alpha) * S[k]["y"] + S[k]["r0"]
        same_bits(r, r_new, f"cg_update_fold: r (value set {k})")
        assert ret == S[k]["np_rr"] and ret > 0
        area2 = host(ws)[len(S[k]["ws1"]) // 2:][:ret].tolist()
        exact, absolute = __import__("blas_extra_refs").exact_sum(r_new, r_new)
        assert abs(math.fsum(area2) - exact) <= 1e-12 * absolute, f"cg_update_fold: the {ret} partials do not add up to <r, r> (value set {k})"
    c.check = check
    return [c]


def b_cg_direction_x_fold(ctx, T):
    n, S = _fold_chain(ctx, T)
    c = Case(ctx)
    ws = c.inout(S[0]["ws2"], S[1]["ws2"])
    rr_old, yp = c.scalar(S[0]["rz"], S[1]["rz"]), c.scalar(S[0]["yp"], S[1]["yp"])
    ps, xs = ctx.vecs(T, n, "p"), ctx.vecs(T, n, "x")
    r, p, x = c.inp(S[0]["r1"], S[1]["r1"]), c.inout(*ps), c.inout(*xs)
    rr_new, m = c.out(1, np.float64), c.host_mirror()
    np_rr = S[0]["np_rr"]
    c.call = lambda s: ctx.cmi.binding.cg_direction_x_fold(rr_new, np_rr, rr_old, yp, r, p, x, ws, stream=s, mirror=m)

    def check(k, ret):
        area2 = S[k]["ws2"][len(S[k]["ws2"]) // 2:][:np_rr].tolist()
        got = float(rr_new[0])
        assert abs(got - math.fsum(area2)) <= 1e-12 * math.fsum(map(abs, area2)), f"cg_direction_x_fold: rr_new {got!r} is not the sum of the partials (value set {k})"
        assert c.mirror_value() == got, "cg_direction_x_fold: the host mirror differs from the device scalar"
        alpha, beta = _q(T, S[k]["rz"], S[k]["yp"]), _q(T, got, S[k]["rz"])
        same_bits(x, alpha * ps[k] + xs[k], f"cg_direction_x_fold: x (value set {k})")
        same_bits(p, T(1) * S[k]["r1"] + beta * ps[k], f"cg_direction_x_fold: p (value set {k})")
    c.check = check
    return [c]


# ---- multi-shift steps (multishift_refs) ---------------------------------------------------------------------------------------------
SHIFTS = 3


def _shift_sets(ctx, T, names, lo=0.5, hi=1.5):
    return {nm: tuple(np.random.default_rng([k, sum(map(ord, nm))]).uniform(lo, hi, SHIFTS).astype(T) for k in (0, 1)) for nm in names}


def b_cg_m_coefficients(ctx, T):
    import multishift_refs as M
    c = Case(ctx)
    s = _shift_sets(ctx, T, ("sigma", "zeta_m1", "zeta_0"))
    st = tuple(np.array(a, T) for a in ((1.0, 0.0), (-0.6, 0.4)))
    rsq_old, pAp, rsq_new = c.scalar(1.75, 3.0), c.scalar(0.6, -1.5), c.scalar(0.9, 0.75)
    state, sigma, zm1, z0 = c.inout(*st), c.inp(*s["sigma"]), c.inout(*s["zeta_m1"]), c.inout(*s["zeta_0"])
    beta_s, alpha_s = c.out(SHIFTS, T), c.out(SHIFTS, T)
    c.call = lambda stream: ctx.cmi.cg_m_coefficients(rsq_old, pAp, rsq_new, state, sigma, zm1, z0, beta_s, alpha_s, stream=stream)

    def check(k, ret):
        a, b, d = ((1.75, 0.6, 0.9), (3.0, -1.5, 0.75))[k]
        want = M.cg_m_coefficients(T, a, b, d, st[k], s["sigma"][k], s["zeta_m1"][k], s["zeta_0"][k])
        for got, w, nm in zip((state, zm1, z0, beta_s, alpha_s), want, ("state", "zeta_m1", "zeta_0", "beta_s", "alpha_s")):
            same_bits(got, np.asarray(w, T), f"cg_m_coefficients: {nm} (value set {k})")
    c.check = check
    return [c]


def b_cg_m_update_xp(ctx, T):
    import multishift_refs as M
    c = Case(ctx)
    n, ld = N1, N1 + 5
    s = _shift_sets(ctx, T, ("beta_s", "alpha_s", "zeta_0"))
    st = tuple(np.array(a, T) for a in ((-0.6, 0.4), (0.5, -0.25)))
    rs, p0s = ctx.vecs(T, n, "r"), ctx.vecs(T, n, "p0")
    xs, pss = ctx.vecs(T, SHIFTS * ld, "xs"), ctx.vecs(T, SHIFTS * ld, "ps")
    state, beta_s, alpha_s, z0 = c.inp(*st), c.inp(*s["beta_s"]), c.inp(*s["alpha_s"]), c.inp(*s["zeta_0"])
    r, p0, x, ps = c.inp(*rs), c.inout(*p0s), c.inout(*xs), c.inout(*pss)
    c.call = lambda stream: ctx.cmi.cg_m_update_xp(n, ld, state, beta_s, alpha_s, z0, r, p0, x, ps, stream=stream)

    def check(k, ret):
        want = M.cg_m_update_xp(T, n, SHIFTS, ld, st[k], s["beta_s"][k], s["alpha_s"][k], s["zeta_0"][k], rs[k], np.array(p0s[k]), np.array(xs[k]), np.array(pss[k]))
        for got, w, nm in zip((p0, x, ps), want, ("p0", "x", "p_s")):
            same_bits(got, w, f"cg_m_update_xp: {nm} (value set {k})")
    c.check = check
    return [c]


def b_bicgstab_m_s(ctx, T):
    import multishift_refs as M
    c, v, d = _vec_case(ctx, T, ("r_1", "As", "s_0"), ("s_0",))
    a1, chi = float(T(1.75 / 0.6)), float(T(-0.7 / 1.3))
    c.call = lambda s: ctx.cmi.bicgstab_m_s(a1, chi, d["r_1"], d["As"], d["s_0"], stream=s)
    c.check = lambda k, ret: same_bits(d["s_0"], M.bicgstab_m_s(T, a1, chi, v["r_1"][k], v["As"][k], v["s_0"][k]), f"bicgstab_m_s (value set {k})")
    return [c]


def b_bicgstab_m_coefficients(ctx, T):
    import multishift_refs as M
    c = Case(ctx)
    s = _shift_sets(ctx, T, ("sigma", "zeta_m1", "zeta_0", "rho_0"))
    by_value = tuple(float(T(v)) for v in (-0.6, 0.45, 0.4, 0.35, 0.8))   # beta_m1, beta_0, alpha_old, alpha_new, chi_0
    ins = [c.inp(*s[nm]) for nm in ("sigma", "zeta_m1", "zeta_0", "rho_0")]
    outs = [c.out(SHIFTS, T) for _ in range(5)]
    c.call = lambda stream: ctx.cmi.bicgstab_m_coefficients(*by_value, *ins, *outs, stream=stream)

    def check(k, ret):
        want = M.bicgstab_m_coefficients(T, *by_value, s["sigma"][k], s["zeta_m1"][k], s["zeta_0"][k], s["rho_0"][k])
        for got, w, nm in zip(outs, want, ("zeta_1", "beta_s", "chi_s", "rho_1", "alpha_s")):
            same_bits(got, np.asarray(w, T), f"bicgstab_m_coefficients: {nm} (value set {k})")
    c.check = check
    return [c]


def b_bicgstab_m_update_xs(ctx, T):
    """Two launches: the update, and the rotation of zeta and rho queued behind it."""
    import multishift_refs as M
    c = Case(ctx)
    n, ld = N1, N1 + 5
    names = ("beta_s", "chi_s", "rho_0", "zeta_m1", "zeta_0", "alpha_s", "rho_1", "zeta_1")
    s = _shift_sets(ctx, T, names)
    rotated = ("rho_0", "zeta_m1", "zeta_0")
    dev = {nm: (c.inout if nm in rotated else c.inp)(*s[nm]) for nm in names}
    r0s, r1s, w1s = ctx.vecs(T, n, "r_0"), ctx.vecs(T, n, "r_1"), ctx.vecs(T, n, "w_1")
    xs, sss = ctx.vecs(T, SHIFTS * ld, "xs"), ctx.vecs(T, SHIFTS * ld, "ss")
    r0, r1, w1, x, ss = c.inp(*r0s), c.inp(*r1s), c.inp(*w1s), c.inout(*xs), c.inout(*sss)
    c.call = lambda stream: ctx.cmi.bicgstab_m_update_xs(n, ld, *[dev[nm] for nm in names], r0, r1, w1, x, ss, stream=stream)

    def check(k, ret):
        want = M.bicgstab_m_update_xs(T, n, SHIFTS, ld, *[s[nm][k] for nm in names], r0s[k], r1s[k], w1s[k], np.array(xs[k]), np.array(sss[k]))
        for got, w, nm in zip((x, ss, dev["zeta_m1"], dev["zeta_0"], dev["rho_0"]), want, ("x", "s_s", "zeta_m1", "zeta_0", "rho_0")):
            same_bits(got, np.asarray(w, T), f"bicgstab_m_update_xs: {nm} (value set {k})")
    c.check = check
    return [c]


def b_dense_gemm(ctx, T):
    """n = 9: two column groups, two launches."""
    import lanczos_refs as Z
    c = Case(ctx)
    m, n, k_ = 1027, 9, 5
    As, Bs = ctx.vecs(T, m * k_, "A"), ctx.vecs(T, k_ * n, "B")
    A, B, C = c.inp(*As), c.inp(*Bs), c.out(m * n, T)
    c.call = lambda s: ctx.cmi.dense_gemm(m, n, k_, A, m, B, k_, C, m, stream=s)
    c.check = lambda k, ret: same_bits(C, Z.gemm_ref(As[k].reshape(k_, m).T, Bs[k].reshape(n, k_).T).T.reshape(-1), f"dense_gemm (value set {k})")
    return [c]


# ---- cusp::eigen's kernels (eigen_refs) and the rest -------------------------------------------------------------------------------------
def _abs_bound(got, S, lengths, dtype, what):
    """test_eigen_gpu.within_bound: |got - S| <= len u S per row, exact for rows of length <= 1."""
    u = 2.0 ** -53 if np.dtype(dtype) == np.float64 else 2.0 ** -24
    g = host(got).astype(np.float64)
    ok = np.where(np.asarray(lengths) <= 1, g == S.astype(dtype).astype(np.float64), np.abs(g - S) <= np.asarray(lengths) * u * S)
    assert ok.all(), f"{what}: rows {np.flatnonzero(~ok)[:5].tolist()} outside len u S"


def b_csr_abs_row_sums(ctx, T):
    import eigen_refs as E
    c = Case(ctx)
    P = [_small(ctx, T, 0), _small(ctx, T, 1)]
    n = P[0]["n"]
    Ap, Ax, out = c.inp(P[0]["Ap"]), c.inp(P[0]["Ax"], P[1]["Ax"]), c.out(n, T)
    c.call = lambda s: ctx.cmi.csr_abs_row_sums(n, Ap, Ax, out, stream=s)
    c.check = lambda k, ret: _abs_bound(out, E.csr_abs_row_sums(P[k]["Ap"], P[k]["Ax"]), np.diff(P[k]["Ap"]), T, f"csr_abs_row_sums (value set {k})")
    return [c]


def b_ell_abs_row_sums(ctx, T):
    import eigen_refs as E
    c = Case(ctx)
    P = [_small(ctx, T, 0), _small(ctx, T, 1)]
    n = P[0]["n"]
    Es = [ctx.orc.csr_to_ell(P[k]["Ap"], P[k]["Aj"], P[k]["Ax"], 5) for k in (0, 1)]
    pitch = Es[0][0]
    eAx, out = c.inp(Es[0][2], Es[1][2]), c.out(n, T)
    c.call = lambda s: ctx.cmi.ell_abs_row_sums(n, n, 5, pitch, eAx, out, stream=s)
    c.check = lambda k, ret: _abs_bound(out, E.ell_abs_row_sums(n, 5, pitch, Es[k][2]), np.full(n, 5), T, f"ell_abs_row_sums (value set {k})")
    return [c]


def b_dia_abs_row_sums(ctx, T):
    import eigen_refs as E
    c = Case(ctx)
    P = [_small(ctx, T, 0), _small(ctx, T, 1)]
    n = P[0]["n"]
    D = [ctx.orc.csr_to_dia(n, n, P[k]["Ap"], P[k]["Aj"], P[k]["Ax"]) for k in (0, 1)]
    pitch, offh = D[0][0], D[0][1]
    off, vals, out = c.inp(offh), c.inp(D[0][2], D[1][2]), c.out(n, T)
    lengths = np.array([sum(0 <= i + int(o) < n for o in offh) for i in range(n)])
    c.call = lambda s: ctx.cmi.dia_abs_row_sums(n, n, len(offh), pitch, off, vals, out, stream=s)
    c.check = lambda k, ret: _abs_bound(out, E.dia_abs_row_sums(n, n, pitch, offh, D[k][2]), lengths, T, f"dia_abs_row_sums (value set {k})")
    return [c]


def b_random_fill(ctx, T):
    import eigen_refs as E
    c = Case(ctx)
    x = c.out(N1, T)
    c.call = lambda s: ctx.cmi.random_fill(x, 12345, stream=s)
    c.check = lambda k, ret: same_bits(x, E.random_fill(N1, 12345, T), "random_fill")
    return [c]


def b_blas_scal_recip(ctx, T):
    import eigen_refs as E
    c = Case(ctx)
    xs = ctx.vecs(T, N1, "x")
    ss = (6.25, 3.0)          # a norm's square in a device double: s = T(sqrt(.))
    s_dev, x, s_out = c.scalar(*ss), c.inout(*xs), c.out(1, np.float64)
    c.call = lambda s: ctx.cmi.blas_scal_recip(s_dev, x, squared_norm=True, s_out=s_out, stream=s)

    def check(k, ret):
        same_bits(x, E.scal_recip(np.array(xs[k]), ss[k], True), f"blas_scal_recip: x (value set {k})")
        assert float(s_out[0]) == float(T(np.sqrt(np.float64(ss[k])))), f"blas_scal_recip: s_out (value set {k})"
    c.check = check
    return [c]


def b_csr_diagonal(ctx, T):
    import blas_extra_refs as R
    c = Case(ctx)
    P = [ctx.poisson(T, 0), ctx.poisson(T, 1)]
    n = P[0]["n"]
    Ap, Aj, Ax, diag = c.inp(P[0]["Ap"]), c.inp(P[0]["Aj"]), c.inp(P[0]["Ax"], P[1]["Ax"]), c.out(n, T)
    c.call = lambda s: ctx.cmi.csr_diagonal(n, Ap, Aj, Ax, diag, reciprocal=True, stream=s)
    c.check = lambda k, ret: same_bits(diag, R.csr_diagonal_ref_fast(T, n, P[k]["Ap"], P[k]["Aj"], P[k]["Ax"], True), f"csr_diagonal (value set {k})")
    return [c]


def b_csr_scale_rows(ctx, T):
    import amg_refs as A
    c = Case(ctx)
    P = [ctx.poisson(T, 0), ctx.poisson(T, 1)]
    n = P[0]["n"]
    ds = tuple((np.abs(ctx.vec(T, n, "d", k)) + T(1)).astype(T) for k in (0, 1))
    Ap, Ax, d, out = c.inp(P[0]["Ap"]), c.inp(P[0]["Ax"], P[1]["Ax"]), c.inp(*ds), c.out(len(P[0]["Ax"]), T)
    lam = float(T(4.0 / 3.0))
    c.call = lambda s: ctx.cmi.csr_scale_rows(n, Ap, Ax, d, lam, out=out, stream=s)
    c.check = lambda k, ret: same_bits(out, A.scale_rows(P[k]["Ap"], P[k]["Ax"], ds[k], lam), f"csr_scale_rows (value set {k})")
    return [c]


def b_relax_jacobi_presmooth(ctx, T):
    import amg_refs as A
    c = Case(ctx)
    ds = tuple((np.abs(ctx.vec(T, N1, "d", k)) + T(1)).astype(T) for k in (0, 1))
    bs = ctx.vecs(T, N1, "b")
    d, b, x = c.inp(*ds), c.inp(*bs), c.out(N1, T)
    omega = float(T(2.0 / 3.0))
    c.call = lambda s: ctx.cmi.relax_jacobi_presmooth(d, b, omega, x, stream=s)
    c.check = lambda k, ret: same_bits(x, A.presmooth(ds[k], bs[k], omega), f"relax_jacobi_presmooth (value set {k})")
    return [c]


def b_csr_ring_max_u64(ctx, T):
    import mis_refs as Q
    c = Case(ctx)
    P = ctx.poisson(np.float64, 0)
    n = P["n"]
    keys = tuple(np.random.default_rng(k).integers(0, 2 ** 62, n, dtype=np.int64) for k in (0, 1))
    Ap, Aj, x, z = c.inp(P["Ap"]), c.inp(P["Aj"]), c.inp(*keys), c.out(n, np.int64)
    c.call = lambda s: ctx.cmi.csr_ring_max(n, Ap, Aj, x, z=z, stream=s)
    c.check = lambda k, ret: same_bits(z, Q.ringmax(P["Ap"], P["Aj"], keys[k].astype(np.uint64)).astype(np.int64), f"csr_ring_max_u64 (value set {k})")
    return [c]


# ---- the builders and conversions that only launch ---------------------------------------------------------------------------------------
def b_poisson5pt_csr(ctx, T):
    c = Case(ctx)
    Ap_w, Aj_w, Ax_w = ctx.orc.poisson5pt_csr(NX, NY, T)
    n = NX * NY
    Ap, Aj, Ax = c.out(n + 1, np.int32), c.out(len(Aj_w), np.int32), c.out(len(Aj_w), T)
    c.call = lambda s: ctx.cmi.poisson5pt_csr(NX, NY, Ap, Aj, Ax, stream=s)

    def check(k, ret):
        same_bits(Ap, Ap_w, "poisson5pt_csr: Ap"), same_bits(Aj, Aj_w, "poisson5pt_csr: Aj"), same_bits(Ax, Ax_w, "poisson5pt_csr: Ax")
    c.check = check
    return [c]


def b_poisson5pt_dia(ctx, T):
    c = Case(ctx)
    off_w, vals_w, _ = ctx.orc.poisson5pt_dia(NX, NY, T)
    n = NX * NY
    off, vals = c.out(5, np.int32), c.out(5 * n, T)
    c.call = lambda s: ctx.cmi.poisson5pt_dia(NX, NY, n, off, vals, stream=s)

    def check(k, ret):
        same_bits(off, off_w, "poisson5pt_dia: offsets"), same_bits(vals, vals_w, "poisson5pt_dia: values")
    c.check = check
    return [c]


def b_csr_to_ell(ctx, T):
    c = Case(ctx)
    n, Ap_h, Aj_h, Ax_h = ctx.irregular(T)
    Ax1 = ctx.vec(T, len(Ax_h), "irr", 1)
    width = 4
    pitch, eAj_w, _ = ctx.orc.csr_to_ell(Ap_h, Aj_h, Ax_h, width)
    Ap, Aj, Ax = c.inp(Ap_h), c.inp(Aj_h), c.inp(Ax_h, Ax1)
    eAj, eAx = c.out(width * pitch, np.int32), c.out(width * pitch, T)
    c.call = lambda s: ctx.cmi.csr_to_ell(n, Ap, Aj, Ax, width, pitch, eAj, eAx, stream=s)

    def check(k, ret):
        _, wj, wx = ctx.orc.csr_to_ell(Ap_h, Aj_h, (Ax_h, Ax1)[k], width)
        rows = np.arange(width * pitch) % pitch < n        # the pitch rows beyond num_rows are not the call's to write
        same_bits(host(eAj)[rows], wj[rows], f"csr_to_ell: columns (value set {k})")
        same_bits(host(eAx)[rows], wx[rows], f"csr_to_ell: values (value set {k})")
    c.check = check
    return [c]


def b_csr_to_hyb_coo(ctx, T):
    c = Case(ctx)
    n, Ap_h, Aj_h, Ax_h = ctx.irregular(T)
    Ax1 = ctx.vec(T, len(Ax_h), "irr", 1)
    width = 4
    over = np.maximum(np.diff(Ap_h) - width, 0)
    offs = (np.cumsum(over) - over).astype(np.int32)
    ncoo = int(over.sum())
    Ap, Aj, Ax, off = c.inp(Ap_h), c.inp(Aj_h), c.inp(Ax_h, Ax1), c.inp(offs)
    cAi, cAj, cAx = c.out(ncoo, np.int32), c.out(ncoo, np.int32), c.out(ncoo, T)
    c.call = lambda s: ctx.cmi.csr_to_hyb_coo(n, Ap, Aj, Ax, width, off, cAi, cAj, cAx, stream=s)

    def check(k, ret):
        w = ctx.orc.csr_to_hyb(Ap_h, Aj_h, (Ax_h, Ax1)[k], width)
        same_bits(cAi, w[3], f"csr_to_hyb_coo: rows (value set {k})"), same_bits(cAj, w[4], "csr_to_hyb_coo: columns"), same_bits(cAx, w[5], "csr_to_hyb_coo: values")
    c.check = check
    return [c]


def b_csr_to_dia(ctx, T):
    """Three launches: the zero fill, the slot table, the scatter."""
    c = Case(ctx)
    P = [ctx.poisson(T, 0), ctx.poisson(T, 1)]
    n = P[0]["n"]
    D = [ctx.formats(T, k)["dia"] for k in (0, 1)]
    pitch, offh = D[0][0], D[0][1]
    Ap, Aj, Ax, off = c.inp(P[0]["Ap"]), c.inp(P[0]["Aj"]), c.inp(P[0]["Ax"], P[1]["Ax"]), c.inp(offh)
    slot_map = c.inp(np.zeros(2 * n, np.int32))      # scratch the call fills from `offsets`; zeros keep every slot in range
    vals = c.out(len(offh) * pitch, T)
    c.call = lambda s: ctx.cmi.binding.csr_to_dia(n, n, Ap, Aj, Ax, off, pitch, slot_map, vals, stream=s)

    def check(k, ret):
        rows = np.arange(len(offh) * pitch) % pitch < n
        same_bits(host(vals)[rows], D[k][2][rows], f"csr_to_dia (value set {k})")
    c.check = check
    return [c]


def b_csr_rebase_offsets(ctx, T):
    c = Case(ctx)
    n, Ap_h, _, _ = ctx.irregular(np.float64)
    block = Ap_h[1000:2001].copy()
    Ap, out = c.inp(block), c.out(1001, np.int32)
    base = int(block[0])
    L = ctx.cmi.lib()
    c.call = lambda s: ctx.cmi.check(L.cmi_csr_rebase_offsets(1000, _ptr(Ap), base, _ptr(out), _sp(s)))
    c.check = lambda k, ret: same_bits(out, block - np.int32(base), "csr_rebase_offsets")
    return [c]


def b_csr_row_indices(ctx, T):
    c = Case(ctx)
    n, Ap_h, Aj_h, _ = ctx.irregular(np.float64)
    Ap, Ai = c.inp(Ap_h), c.out(len(Aj_h), np.int32)
    c.call = lambda s: ctx.cmi.csr_row_indices(n, Ap, Ai, stream=s)
    c.check = lambda k, ret: same_bits(Ai, ctx.orc.csr_row_indices(Ap_h), "csr_row_indices")
    return [c]


def b_ell_row_lengths(ctx, T):
    c = Case(ctx)
    n, Ap_h, Aj_h, Ax_h = ctx.irregular(np.float64)
    width = 4
    pitch, eAj_h, _ = ctx.orc.csr_to_ell(Ap_h, Aj_h, Ax_h, width)
    eAj_h = np.where(np.arange(width * pitch) % pitch < n, eAj_h, -1).astype(np.int32)
    eAj, lengths = c.inp(eAj_h), c.out(n, np.int32)
    c.call = lambda s: ctx.cmi.ell_row_lengths(n, width, pitch, eAj, lengths, stream=s)
    c.check = lambda k, ret: same_bits(lengths, np.minimum(np.diff(Ap_h), width).astype(np.int32), "ell_row_lengths")
    return [c]


# ------------------------------------------------------------------------------------------------------------------------------
# builders: the synchronising set-up calls.  Their host values are compared as soon as the call returns.
# ------------------------------------------------------------------------------------------------------------------------------
def b_hyb_entries_per_row(ctx, T):
    c = Case(ctx)
    n, Ap_h, _, _ = ctx.irregular(np.float64)
    Ap = c.inp(Ap_h)
    c.call = lambda s: ctx.cmi.hyb_entries_per_row(ctx.cmi.F64, n, Ap, kind=ctx.cmi.HYB_RULE_REFERENCE, relative_speed=3.0, threshold=1000, stream=s)
    want = ctx.orc.optimal_entries_per_row(Ap_h, 3.0, 1000)
    assert want > 0, "the width must differ from the placeholder's (0)"

    def check(k, ret):
        assert ret == want, f"hyb_entries_per_row: {ret} against the oracle's {want}"
    c.check = check
    return [c]


def _plan_case(ctx, make, want, what):
    c = Case(ctx)
    c.call = lambda s: make(c, s)

    def check(k, ret):
        c.keep.append(ret)
        got = want[0](ret)
        assert got == want[1], f"{what}: {got} against {want[1]}"
    c.check = check
    return c


def b_plan_create(ctx, T):
    n, Ap_h, Aj_h, _ = ctx.irregular(np.float64)
    c = Case(ctx)
    Ap = c.inp(Ap_h)
    cmi = ctx.cmi
    c.call = lambda s: cmi.Plan(cmi.FORMAT_CSR, cmi.F64, n, n, len(Aj_h), Ap, stream=s)
    c.check = lambda k, plan: _expect(plan.info()["max_row_length"], int(np.diff(Ap_h).max()), "plan_create: max_row_length")
    return [c]


def _expect(got, want, what):
    assert got == want, f"{what}: {got} against {want}"


def b_plan_create_csr(ctx, T):
    n, Ap_h, Aj_h, _ = ctx.irregular(np.float64)
    c = Case(ctx)
    Ap, Aj = c.inp(Ap_h), c.inp(Aj_h)
    cmi = ctx.cmi
    c.call = lambda s: cmi.Plan.csr(cmi.F64, n, n, Ap, Aj, stream=s)
    c.check = lambda k, plan: _expect(plan.info()["max_row_length"], int(np.diff(Ap_h).max()), "plan_create_csr: max_row_length")
    return [c]


def b_plan_create_coo(ctx, T):
    """Unsorted row indices: the plan must find them unsorted (the all-zero placeholder is sorted)."""
    n, Ap_h, Aj_h, _ = ctx.irregular(np.float64)
    Ai_h = ctx.orc.csr_row_indices(Ap_h)[::-1].copy()
    c = Case(ctx)
    Ai, Aj = c.inp(Ai_h), c.inp(Aj_h)
    cmi = ctx.cmi
    c.call = lambda s: cmi.Plan.coo(cmi.F64, n, n, Ai, Aj, stream=s)
    c.check = lambda k, plan: _expect(plan.info()["coo_sorted"], False, "plan_create_coo: coo_sorted")
    return [c]


def b_plan_create_csr_values(ctx, T):
    """The packed plan copies the values: a plan made from the placeholder would not validate against the real ones."""
    P = ctx.poisson(np.float64, 0)
    n = P["n"]
    c = Case(ctx)
    Ap, Aj, Ax = c.inp(P["Ap"]), c.inp(P["Aj"]), c.inp(P["Ax"])
    cmi = ctx.cmi
    c.call = lambda s: cmi.Plan.csr_values(n, n, Ap, Aj, Ax, cfg=cmi.Config(kernel=cmi.CSR_STREAM_PACKED), stream=s)

    def check(k, plan):
        _expect(plan.config().kernel, cmi.CSR_STREAM_PACKED, "plan_create_csr_values: kernel")
        _expect(plan.info()["max_row_length"], 5, "plan_create_csr_values: max_row_length")
        real = ctx.torch.from_numpy(P["Ax"].copy()).to(ctx.dev)
        _expect(plan.validate_values(real), True, "plan_create_csr_values: the plan's copy of the values")
    c.check = check
    return [c]


def b_plan_validate_values(ctx, T):
    P = ctx.poisson(np.float64, 0)
    n = P["n"]
    c = Case(ctx)
    cmi = ctx.cmi
    Ap, Aj = c.fixed(P["Ap"]), c.fixed(P["Aj"])
    plan = cmi.Plan.csr_values(n, n, Ap, Aj, c.fixed(P["Ax"]), cfg=cmi.Config(kernel=cmi.CSR_STREAM_PACKED))
    c.keep.append(plan)
    Ax = c.inp(P["Ax"])
    c.call = lambda s: plan.validate_values(Ax, stream=s)
    c.check = lambda k, ret: _expect(ret, True, "plan_validate_values")
    return [c]


def b_plan_create_hyb(ctx, T):
    """Row indices in descending order: an unsorted COO part takes the two-launch form (the all-zero placeholder is sorted and light)."""
    F = ctx.formats(np.float64, 0)
    n = ctx.poisson(np.float64, 0)["n"]
    cAi_h = F["hyb"][4][::-1].copy()
    c = Case(ctx)
    cAi = c.inp(cAi_h)
    cmi = ctx.cmi
    c.call = lambda s: cmi.Plan.hyb(cmi.F64, n, n, 3, cAi, stream=s)
    c.check = lambda k, plan: _expect(plan.hyb_launches(), 2, "plan_create_hyb: launches")
    return [c]


def b_plan_validate(ctx, T):
    n, Ap_h, Aj_h, _ = ctx.irregular(np.float64)
    c = Case(ctx)
    cmi = ctx.cmi
    plan = cmi.Plan(cmi.FORMAT_CSR, cmi.F64, n, n, len(Aj_h), c.fixed(Ap_h))
    c.keep.append(plan)
    Ap = c.inp(Ap_h)
    c.call = lambda s: plan.validate(Ap, stream=s)
    c.check = lambda k, ret: _expect(ret, True, "plan_validate")
    return [c]


def _spgemm_operands(ctx, T):
    import spgemm_refs as G
    def make():
        rng = np.random.default_rng(17)
        return G.random_pair(rng, 301, 257, 283, 0.02, 0.03, T)
    return ctx.cached(("spgemm", T), make)


def b_spgemm_csr(ctx, T):
    import spgemm_refs as G
    m, k_, n, Ap_h, Aj_h, Ax_h, Bp_h, Bj_h, Bx_h = _spgemm_operands(ctx, T)
    c = Case(ctx)
    dev = [c.inp(a) for a in (Ap_h, Aj_h, Ax_h, Bp_h, Bj_h, Bx_h)]
    c.call = lambda s: ctx.cmi.spgemm_csr(m, k_, n, *dev, stream=s)

    def check(k, ret):
        want = G.spgemm(m, k_, n, Ap_h, Aj_h, Ax_h, Bp_h, Bj_h, Bx_h)
        for got, w, nm in zip(ret[:3], want, ("Cp", "Cj", "Cx")):
            same_bits(got, w, f"spgemm_csr: {nm}")
    c.check = check
    return [c]


def b_spgemm_take(ctx, T):
    """The handle is made from the real operands while the case is built; the copy out of it is the call under test.  It has no
    device input of the caller's: check A shows that the copies are queued on the given stream and complete, check B that they record.
    Two forms: a product with entries (copies out of the handle), and an empty one (A has no entries: the handle holds nothing on
    the device and the call zero-fills Cp itself, its one launch)."""
    import spgemm_refs as G
    m, k_, n, Ap_h, Aj_h, Ax_h, Bp_h, Bj_h, Bx_h = _spgemm_operands(ctx, T)
    L, cmi = ctx.cmi.lib(), ctx.cmi
    suf = "f64" if T is np.float64 else "f32"

    def one(label, Ap_h, Aj_h, Ax_h):
        want = G.spgemm(m, k_, n, Ap_h, Aj_h, Ax_h, Bp_h, Bj_h, Bx_h)
        c = Case(ctx, label)
        dev = [c.fixed(a) for a in (Ap_h, Aj_h, Ax_h, Bp_h, Bj_h, Bx_h)]
        h = ctypes.c_void_p()
        cmi.check(getattr(L, "cmi_spgemm_csr_" + suf)(m, k_, n, len(Aj_h), *map(_ptr, dev[:3]), len(Bj_h), *map(_ptr, dev[3:]), ctypes.byref(h), None))

        class Handle:
            def __del__(self):
                L.cmi_spgemm_destroy(h)
        c.keep.append(Handle())
        nnz = len(want[1])
        Cp, Cj, Cx = c.out(m + 1, np.int32), c.out(nnz, np.int32), c.out(nnz, T)
        c.call = lambda s: cmi.check(getattr(L, "cmi_spgemm_take_" + suf)(h, _ptr(Cp), _ptr(Cj), _ptr(Cx), nnz, _sp(s)))

        def check(k, ret):
            for got, w, nm in zip((Cp, Cj, Cx), want, ("Cp", "Cj", "Cx")):
                same_bits(got, w, f"spgemm_take {label}: {nm}")
        c.check = check
        return c, want

    full, _ = one("with entries", Ap_h, Aj_h, Ax_h)
    empty, want = one("empty product", np.zeros(m + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, T))
    assert len(want[1]) == 0 and not want[0].any()
    return [full, empty]


def b_csr_strength_symmetric(ctx, T):
    import amg_refs as A
    P = _small(ctx, T, 0)
    n = P["n"]
    c = Case(ctx)
    Ap, Aj, Ax = c.inp(P["Ap"]), c.inp(P["Aj"]), c.inp(P["Ax"])
    c.call = lambda s: ctx.cmi.csr_strength_symmetric(n, Ap, Aj, Ax, theta=0.25, stream=s)

    def check(k, ret):
        want = A.strength(n, P["Ap"], P["Aj"], P["Ax"], 0.25)
        assert len(want[1]) < len(P["Aj"]), "the threshold must drop something"
        for got, w, nm in zip(ret, want, ("Sp", "Sj", "Sx")):
            same_bits(got, w, f"csr_strength_symmetric: {nm}")
    c.check = check
    return [c]


def b_aggregates_fit(ctx, T):
    import amg_refs as A
    n, na = 3001, 400
    agg_h = np.random.default_rng(5).integers(-1, na, n).astype(np.int32)
    B_h = ctx.vec(T, n, "B", 0)
    c = Case(ctx)
    agg, B = c.inp(agg_h), c.inp(B_h)
    c.call = lambda s: ctx.cmi.aggregates_fit(agg, B, na, stream=s)

    def check(k, ret):
        for got, w, nm in zip(ret, A.fit(agg_h, np.array(B_h), na), ("Tp", "Tj", "Tx", "R")):
            same_bits(got, w, f"aggregates_fit: {nm}")
    c.check = check
    return [c]


def b_csr_elementwise(ctx, T):
    import amg_refs as A
    rng = np.random.default_rng(23)
    m, n = 301, 257
    (Ap_h, Aj_h, Ax_h), (Bp_h, Bj_h, Bx_h) = A.random_sorted_csr(rng, m, n, 0.03, T), A.random_sorted_csr(rng, m, n, 0.03, T)
    c = Case(ctx)
    dev = [c.inp(a) for a in (Ap_h, Aj_h, Ax_h, Bp_h, Bj_h, Bx_h)]
    c.call = lambda s: ctx.cmi.csr_elementwise(m, n, *dev, op="subtract", stream=s)

    def check(k, ret):
        assert ret is not None, "csr_elementwise: the operands were reported unsorted"
        for got, w, nm in zip(ret, A.elementwise(m, n, Ap_h, Aj_h, Ax_h, Bp_h, Bj_h, Bx_h, "subtract"), ("Cp", "Cj", "Cx")):
            same_bits(got, w, f"csr_elementwise: {nm}")
    c.check = check
    return [c]


def b_csr_transpose_positions(ctx, T):
    import evolution_refs as V
    P = _small(ctx, np.float64, 0)
    n = P["n"]
    c = Case(ctx)
    Ap, Aj = c.inp(P["Ap"]), c.inp(P["Aj"])
    c.call = lambda s: ctx.cmi.csr_transpose_positions(n, Ap, Aj, stream=s)

    def check(k, ret):
        assert ret is not None, "csr_transpose_positions: the pattern was reported as not conforming"
        same_bits(ret, V.transpose_positions(n, P["Ap"], P["Aj"])[0], "csr_transpose_positions")
    c.check = check
    return [c]


def b_csr_masked_product(ctx, T):
    import evolution_refs as V
    P = _small(ctx, T, 0)
    n, nnz = P["n"], len(P["Aj"])
    V_h, W_h = ctx.vec(T, nnz, "V", 0), ctx.vec(T, nnz, "W", 0)
    c = Case(ctx)
    Ap, Aj, Vx, Wx, out = c.inp(P["Ap"]), c.inp(P["Aj"]), c.inp(V_h), c.inp(W_h), c.out(nnz, T)
    c.call = lambda s: ctx.cmi.csr_masked_product(n, Ap, Aj, Vx, Wx, out=out, stream=s)
    c.check = lambda k, ret: same_bits(out, V.masked_product(n, P["Ap"], P["Aj"], V_h, W_h), "csr_masked_product")
    return [c]


def b_csr_evolution_strength(ctx, T):
    import evolution_refs as V
    n, Ap_h, Aj_h, Ax_h = __import__("multishift_refs").poisson5pt(29, 23, T)
    B_h = (np.abs(ctx.vec(T, n, "B", 0)) + T(0.5)).astype(T)
    c = Case(ctx)
    Ap, Aj, Ax, B = c.inp(Ap_h), c.inp(Aj_h), c.inp(Ax_h), c.inp(B_h)
    c.call = lambda s: ctx.cmi.csr_evolution_strength(n, Ap, Aj, Ax, B, 2.0, epsilon=4.0, stream=s)

    def check(k, ret):
        assert ret is not None, "csr_evolution_strength: the pattern was reported as not conforming"
        for got, w, nm in zip(ret, V.evolution_strength(n, Ap_h, Aj_h, Ax_h, B_h, 2.0, 4.0)["S"], ("Sp", "Sj", "Sx")):
            same_bits(got, w, f"csr_evolution_strength: {nm}")
    c.check = check
    return [c]


def _pattern(ctx):
    P = ctx.poisson(np.float64, 0)
    return P["n"], P["Ap"], P["Aj"]


def b_csr_maximal_independent_set(ctx, T):
    import mis_refs as Q
    n, Ap_h, Aj_h = _pattern(ctx)
    c = Case(ctx)
    Ap, Aj = c.inp(Ap_h), c.inp(Aj_h)
    c.call = lambda s: ctx.cmi.maximal_independent_set((n, Ap, Aj), k=1, seed=3, stream=s)

    def check(k, ret):
        stencil, rounds = Q.mis(n, Ap_h, Aj_h, 1, seed=3)
        same_bits(ret[0], stencil, "csr_maximal_independent_set: stencil")
        _expect((ret[1], ret[2]), (int(stencil.sum()), rounds), "csr_maximal_independent_set: (set size, rounds)")
    c.check = check
    return [c]


def b_csr_mis_aggregate(ctx, T):
    import mis_refs as Q
    n, Ap_h, Aj_h = _pattern(ctx)
    c = Case(ctx)
    Ap, Aj = c.inp(Ap_h), c.inp(Aj_h)
    c.call = lambda s: ctx.cmi.mis_aggregate((n, Ap, Aj), seed=3, stream=s)

    def check(k, ret):
        agg, m, count = Q.mis_aggregate(n, Ap_h, Aj_h, seed=3)
        same_bits(ret[0], agg, "csr_mis_aggregate: aggregates"), same_bits(ret[1], m, "csr_mis_aggregate: mis")
        _expect(ret[2], count, "csr_mis_aggregate: count")
    c.check = check
    return [c]


def b_csr_breadth_first_search(ctx, T):
    import graph_refs as H
    n, Ap_h, Aj_h = _pattern(ctx)
    c = Case(ctx)
    Ap, Aj = c.inp(Ap_h), c.inp(Aj_h)
    c.call = lambda s: ctx.cmi.breadth_first_search(n, Ap, Aj, 17, mark_levels=False, stream=s)

    def check(k, ret):
        labels, reached, depth = H.bfs(n, Ap_h, Aj_h, 17, mark_levels=False)
        same_bits(ret[0], labels, "csr_breadth_first_search: predecessors")
        _expect((ret[1], ret[2]), (reached, depth), "csr_breadth_first_search: (reached, depth)")
    c.check = check
    return [c]


def b_csr_pseudo_peripheral_vertex(ctx, T):
    import graph_refs as H
    n, Ap_h, Aj_h = _pattern(ctx)
    c = Case(ctx)
    Ap, Aj = c.inp(Ap_h), c.inp(Aj_h)
    c.call = lambda s: ctx.cmi.pseudo_peripheral_vertex(n, Ap, Aj, start=2500, stream=s)

    def check(k, ret):
        vertex, levels, searches = H.pseudo_peripheral(n, Ap_h, Aj_h, 2500)
        _expect((ret[0], ret[2]), (vertex, searches), "csr_pseudo_peripheral_vertex: (vertex, searches)")
        same_bits(ret[1], levels, "csr_pseudo_peripheral_vertex: levels")
    c.check = check
    return [c]


def b_csr_symmetric_rcm(ctx, T):
    import graph_refs as H
    n, Ap_h, Aj_h = _pattern(ctx)
    c = Case(ctx)
    Ap, Aj = c.inp(Ap_h), c.inp(Aj_h)
    c.call = lambda s: ctx.cmi.symmetric_rcm(n, Ap, Aj, start=2500, stream=s)

    def check(k, ret):
        permutation, vertex = H.symmetric_rcm(n, Ap_h, Aj_h, 2500)
        _expect(ret[1], vertex, "csr_symmetric_rcm: vertex")
        same_bits(ret[0], permutation, "csr_symmetric_rcm: permutation")
    c.check = check
    return [c]


def _map_values(ctx, T, n):
    return np.arange(n, dtype=np.int32) * 3 - 1000 if T is np.int32 else ctx.vec(T, n, "g", 0)


def b_gather(ctx, T):
    import graph_refs as H
    m, n = 4001, N1
    map_h = np.random.default_rng(3).integers(0, m, n).astype(np.int32)
    x_h = _map_values(ctx, T, m)
    c = Case(ctx)
    mp, x = c.inp(map_h), c.inp(x_h)
    c.call = lambda s: ctx.cmi.gather(mp, x, m, stream=s)
    c.check = lambda k, ret: same_bits(ret, H.gather(map_h, x_h), "gather")
    return [c]


def b_scatter(ctx, T):
    import graph_refs as H
    n = N1
    map_h = np.random.default_rng(4).permutation(n).astype(np.int32)
    x_h = _map_values(ctx, T, n)
    c = Case(ctx)
    mp, x = c.inp(map_h), c.inp(x_h)
    c.call = lambda s: ctx.cmi.scatter(mp, x, n, stream=s)
    c.check = lambda k, ret: same_bits(ret, H.scatter(map_h, x_h, n), "scatter")
    return [c]


def b_csr_max_row_length(ctx, T):
    n, Ap_h, _, _ = ctx.irregular(np.float64)
    c = Case(ctx)
    Ap = c.inp(Ap_h)
    L = ctx.cmi.lib()

    def call(s):
        got = ctypes.c_int64(-1)
        ctx.cmi.check(L.cmi_csr_max_row_length(n, _ptr(Ap), ctypes.byref(got), _sp(s)))
        return got.value
    c.call = call
    c.check = lambda k, ret: _expect(ret, int(np.diff(Ap_h).max()), "csr_max_row_length")
    return [c]


def b_count_zeros(ctx, T):
    v = np.array(ctx.vec(T, N1, "z", 0))
    v[::7] = 0
    v[5] = -0.0
    c = Case(ctx)
    values = c.inp(v)
    c.call = lambda s: ctx.cmi.count_zeros(values, stream=s)
    c.check = lambda k, ret: _expect(ret, int(np.count_nonzero(v == 0)), "count_zeros")
    return [c]


def b_csr_diagonals(ctx, T):
    P = ctx.poisson(np.float64, 0)
    n = P["n"]
    c = Case(ctx)
    Ap, Aj = c.inp(P["Ap"]), c.inp(P["Aj"])
    slot_map, diag_list = c.out(2 * n, np.int32), c.out(16, np.int32)
    c.outputs = c.outputs[1:]       # slot_map is scratch kept for cmi_csr_to_dia_*: its contents are not specified
    c.call = lambda s: ctx.cmi.binding.csr_diagonals(n, n, Ap, Aj, slot_map, diag_list, stream=s)

    def check(k, ret):
        want = ctx.formats(np.float64, 0)["dia"][1]
        _expect(ret, len(want), "csr_diagonals: count")
        same_bits(np.sort(host(diag_list)[:ret]), np.sort(want), "csr_diagonals: offsets")
    c.check = check
    return [c]


def b_csr_interior_rows(ctx, T):
    """The numpy restatement of test_interior_rows_of_a_row_block on rows [1000, 3000) of the matrix."""
    P = ctx.poisson(np.float64, 0)
    r0, r1 = 1000, 3000
    rows = r1 - r0
    Ap_h = (P["Ap"][r0:r1 + 1] - P["Ap"][r0]).astype(np.int32)
    Aj_h = P["Aj"][P["Ap"][r0]:P["Ap"][r1]].copy()
    c = Case(ctx)
    Ap, Aj = c.inp(Ap_h), c.inp(Aj_h)
    c.call = lambda s: ctx.cmi.csr_interior_rows(rows, Ap, Aj, r0, r1, stream=s)

    def check(k, ret):
        outside = np.array([np.any((Aj_h[Ap_h[i]:Ap_h[i + 1]] < r0) | (Aj_h[Ap_h[i]:Ap_h[i + 1]] >= r1)) for i in range(rows)])
        below, above = np.nonzero(outside[:rows // 2])[0], np.nonzero(outside[rows // 2:])[0]
        want = (int(below[-1]) + 1 if below.size else 0, int(above[0]) + rows // 2 if above.size else rows)
        assert want == (NX, rows - NX)
        _expect(ret, want, "csr_interior_rows")
    c.check = check
    return [c]


def b_csr_column_span(ctx, T):
    P = ctx.poisson(np.float64, 0)
    Aj_h = P["Aj"][P["Ap"][1000]:P["Ap"][3000]].copy()
    c = Case(ctx)
    Aj = c.inp(Aj_h)
    c.call = lambda s: ctx.cmi.csr_column_span(Aj, stream=s)
    c.check = lambda k, ret: _expect(ret, (int(Aj_h.min()), int(Aj_h.max())), "csr_column_span")
    return [c]


def b_coo_row_offsets(ctx, T):
    n, Ap_h, _, _ = ctx.irregular(np.float64)
    Ai_h = ctx.orc.csr_row_indices(Ap_h)
    c = Case(ctx)
    Ai, Ap = c.inp(Ai_h), c.out(n + 1, np.int32)
    c.call = lambda s: ctx.cmi.coo_row_offsets(n, Ai, Ap, stream=s)

    def check(k, ret):
        _expect(ret, True, "coo_row_offsets: sorted")
        same_bits(Ap, Ap_h, "coo_row_offsets: Ap")
    c.check = check
    return [c]


def b_coo_sort_by_row(ctx, T):
    n, Ap_h, Aj_h, Ax_h = ctx.irregular(T)
    shuffle = np.random.default_rng(8).permutation(len(Aj_h))
    Ai_s, Aj_s, Ax_s = ctx.orc.csr_row_indices(Ap_h)[shuffle], Aj_h[shuffle], Ax_h[shuffle]
    c = Case(ctx)
    Ai, Aj, Ax = c.inout(Ai_s), c.inout(Aj_s), c.inout(Ax_s)
    c.call = lambda s: ctx.cmi.coo_sort_by_row(n, n, Ai, Aj, Ax, stream=s)

    def check(k, ret):
        order = np.argsort(Ai_s, kind="stable")        # entries of a row keep their storage order
        same_bits(Ai, Ai_s[order], "coo_sort_by_row: rows"), same_bits(Aj, Aj_s[order], "coo_sort_by_row: columns"), same_bits(Ax, Ax_s[order], "coo_sort_by_row: values")
    c.check = check
    return [c]


def b_coo_is_sorted(ctx, T):
    """Unsorted entries: the answer False cannot come from the all-zero placeholder, which is sorted."""
    n, Ap_h, _, _ = ctx.irregular(np.float64)
    Ai_h = ctx.orc.csr_row_indices(Ap_h)[::-1].copy()
    c = Case(ctx)
    Ai = c.inp(Ai_h)
    c.call = lambda s: ctx.cmi.coo_is_sorted(n, Ai, stream=s)
    c.check = lambda k, ret: _expect(ret, False, "coo_is_sorted")
    return [c]


def _to_csr_check(ret, want, what):
    for got, w, nm in zip(ret, want, ("Ap", "Aj", "Ax")):
        same_bits(got, w, f"{what}: {nm}")


def b_ell_to_csr(ctx, T):
    P, F = ctx.poisson(T, 0), ctx.formats(T, 0)
    width, pitch, eAj_h, eAx_h = F["ell"]
    live = np.arange(width * pitch) % pitch < P["n"]
    c = Case(ctx)
    eAj, eAx = c.inp(np.where(live, eAj_h, -1).astype(np.int32)), c.inp(np.where(live, eAx_h, 0).astype(T))
    c.call = lambda s: ctx.cmi.ell_to_csr(P["n"], width, pitch, eAj, eAx, stream=s)
    c.check = lambda k, ret: _to_csr_check(ret, (P["Ap"], P["Aj"], P["Ax"]), "ell_to_csr")
    return [c]


def b_dia_to_csr(ctx, T):
    P, F = ctx.poisson(T, 0), ctx.formats(T, 0)
    pitch, off_h, vals_h = F["dia"]
    live = np.arange(len(off_h) * pitch) % pitch < P["n"]
    c = Case(ctx)
    off, vals = c.inp(off_h), c.inp(np.where(live, vals_h, 0).astype(T))
    c.call = lambda s: ctx.cmi.dia_to_csr(P["n"], P["n"], len(off_h), pitch, off, vals, stream=s)
    c.check = lambda k, ret: _to_csr_check(ret, (P["Ap"], P["Aj"], P["Ax"]), "dia_to_csr")
    return [c]


def b_hyb_to_csr(ctx, T):
    P, F = ctx.poisson(T, 0), ctx.formats(T, 0)
    width, pitch, hAj_h, hAx_h, cAi_h, cAj_h, cAx_h = F["hyb"]
    live = np.arange(width * pitch) % pitch < P["n"]
    c = Case(ctx)
    dev = [c.inp(a) for a in (np.where(live, hAj_h, -1).astype(np.int32), np.where(live, hAx_h, 0).astype(T), cAi_h, cAj_h, cAx_h)]
    c.call = lambda s: ctx.cmi.hyb_to_csr(P["n"], width, pitch, *dev, stream=s)
    c.check = lambda k, ret: _to_csr_check(ret, (P["Ap"], P["Aj"], P["Ax"]), "hyb_to_csr")
    return [c]


# ------------------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------------------
class Row:
    def __init__(self, family, cls, types, builder=None, reason=None):
        self.family, self.cls, self.types, self.builder, self.reason = family, cls, tuple(types), builder, reason


FF = ("f64", "f32")
ONE = ("",)


def _a(family, builder, types=FF):
    return Row(family, ASYNC, types, builder)


def _b(family, builder, types=FF):
    return Row(family, SYNC, types, builder)


ROWS = [
    # ---- asynchronous: launches only -------------------------------------------------------------------------------------
    _a("cmi_spmv_csr", b_spmv_csr), _a("cmi_spmv_csr_plan", b_spmv_csr_plan), _a("cmi_spmm_csr", b_spmm_csr),
    _a("cmi_spmv_csr_dot", b_spmv_csr_dot), _a("cmi_spmv_csr_dot_plan", b_spmv_csr_dot_plan),
    _a("cmi_spmv_csr_dot_plan_partials", b_spmv_csr_dot_plan_partials),
    _a("cmi_spmv_ell", b_spmv_ell), _a("cmi_spmv_ell_dot", b_spmv_ell_dot), _a("cmi_spmv_dia", b_spmv_dia), _a("cmi_spmv_dia_dot", b_spmv_dia_dot),
    _a("cmi_spmv_coo", b_spmv_coo), _a("cmi_spmv_coo_plan", b_spmv_coo_plan), _a("cmi_spmv_coo_dot_plan", b_spmv_coo_dot_plan),
    _a("cmi_spmv_hyb", b_spmv_hyb), _a("cmi_spmv_hyb_plan", b_spmv_hyb_plan), _a("cmi_spmv_hyb_dot_plan", b_spmv_hyb_dot_plan),
    _a("cmi_spmv_csr_semiring", b_spmv_csr_semiring), _a("cmi_spmv_coo_semiring", b_spmv_coo_semiring),
    _a("cmi_spmv_ell_semiring", b_spmv_ell_semiring), _a("cmi_spmv_dia_semiring", b_spmv_dia_semiring),
    _a("cmi_spmv_csr_axpby", b_spmv_csr_axpby), _a("cmi_csr_jacobi_sweep", b_csr_jacobi_sweep), _a("cmi_relax_jacobi_update", b_relax_jacobi_update),
    _a("cmi_csr_gauss_seidel_colour", b_csr_gauss_seidel_colour),
    _a("cmi_blas_axpy", b_blas_axpy), _a("cmi_blas_axpby", b_blas_axpby), _a("cmi_blas_copy", b_blas_copy), _a("cmi_blas_fill", b_blas_fill),
    _a("cmi_blas_dot", b_blas_dot), _a("cmi_blas_nrm2", b_blas_nrm2), _a("cmi_blas_dotd", b_blas_dotd, ("f32",)),
    _a("cmi_blas_asum", b_blas_asum), _a("cmi_blas_amax", b_blas_amax),
    *[_a(family, functools.partial(_extra, name=name)) for name, (family, _) in _EXTRA.items()],
    _a("cmi_cg_update", b_cg_update), _a("cmi_cg_direction", b_cg_direction), _a("cmi_cg_direction_x", b_cg_direction_x),
    _a("cmi_cg_update_fold", b_cg_update_fold), _a("cmi_cg_direction_x_fold", b_cg_direction_x_fold),
    _a("cmi_cg_m_coefficients", b_cg_m_coefficients), _a("cmi_cg_m_update_xp", b_cg_m_update_xp),
    _a("cmi_bicgstab_m_s", b_bicgstab_m_s), _a("cmi_bicgstab_m_coefficients", b_bicgstab_m_coefficients), _a("cmi_bicgstab_m_update_xs", b_bicgstab_m_update_xs),
    *[_a("cmi_lobpcg_" + name, functools.partial(_lobpcg, name=name)) for name in _LOBPCG],
    _a("cmi_dense_gemm", b_dense_gemm),
    _a("cmi_csr_abs_row_sums", b_csr_abs_row_sums), _a("cmi_ell_abs_row_sums", b_ell_abs_row_sums), _a("cmi_dia_abs_row_sums", b_dia_abs_row_sums),
    _a("cmi_random_fill", b_random_fill), _a("cmi_blas_scal_recip", b_blas_scal_recip), _a("cmi_csr_diagonal", b_csr_diagonal),
    _a("cmi_csr_scale_rows", b_csr_scale_rows), _a("cmi_relax_jacobi_presmooth", b_relax_jacobi_presmooth), _a("cmi_csr_ring_max_u64", b_csr_ring_max_u64, ONE),
    _a("cmi_spgemm_take", b_spgemm_take),      # copies out of the handle, queued on the stream: asynchronous (the header says so now)
    _a("cmi_poisson5pt_csr", b_poisson5pt_csr), _a("cmi_poisson5pt_dia", b_poisson5pt_dia),
    _a("cmi_csr_to_ell", b_csr_to_ell), _a("cmi_csr_to_hyb_coo", b_csr_to_hyb_coo), _a("cmi_csr_to_dia", b_csr_to_dia),
    _a("cmi_csr_rebase_offsets", b_csr_rebase_offsets, ONE), _a("cmi_csr_row_indices", b_csr_row_indices, ONE), _a("cmi_ell_row_lengths", b_ell_row_lengths, ONE),
    # ---- synchronising set-up calls -------------------------------------------------------------------------------------------
    _b("cmi_hyb_entries_per_row", b_hyb_entries_per_row, ONE),
    _b("cmi_plan_create", b_plan_create, ONE), _b("cmi_plan_create_csr", b_plan_create_csr, ONE), _b("cmi_plan_create_coo", b_plan_create_coo, ONE),
    _b("cmi_plan_create_csr_values", b_plan_create_csr_values, ONE), _b("cmi_plan_validate_values", b_plan_validate_values, ONE),
    _b("cmi_plan_create_hyb", b_plan_create_hyb, ONE), _b("cmi_plan_validate", b_plan_validate, ONE),
    _b("cmi_spgemm_csr", b_spgemm_csr),
    _b("cmi_csr_strength_symmetric", b_csr_strength_symmetric), _b("cmi_aggregates_fit", b_aggregates_fit), _b("cmi_csr_elementwise", b_csr_elementwise),
    _b("cmi_csr_transpose_positions", b_csr_transpose_positions, ONE), _b("cmi_csr_masked_product", b_csr_masked_product),
    _b("cmi_csr_evolution_strength", b_csr_evolution_strength),
    _b("cmi_csr_maximal_independent_set", b_csr_maximal_independent_set, ONE), _b("cmi_csr_mis_aggregate", b_csr_mis_aggregate, ONE),
    _b("cmi_csr_breadth_first_search", b_csr_breadth_first_search, ONE), _b("cmi_csr_pseudo_peripheral_vertex", b_csr_pseudo_peripheral_vertex, ONE),
    _b("cmi_csr_symmetric_rcm", b_csr_symmetric_rcm, ONE),
    _b("cmi_gather", b_gather, ("i32", "f32", "f64")), _b("cmi_scatter", b_scatter, ("i32", "f32", "f64")),
    _b("cmi_csr_max_row_length", b_csr_max_row_length, ONE), _b("cmi_count_zeros", b_count_zeros),
    _b("cmi_csr_diagonals", b_csr_diagonals, ONE), _b("cmi_csr_interior_rows", b_csr_interior_rows, ONE), _b("cmi_csr_column_span", b_csr_column_span, ONE),
    _b("cmi_coo_row_offsets", b_coo_row_offsets, ONE), _b("cmi_coo_sort_by_row", b_coo_sort_by_row), _b("cmi_coo_is_sorted", b_coo_is_sorted, ONE),
    _b("cmi_ell_to_csr", b_ell_to_csr), _b("cmi_dia_to_csr", b_dia_to_csr), _b("cmi_hyb_to_csr", b_hyb_to_csr),
    # ---- out of scope -------------------------------------------------------------------------------------------------------------
    *[Row(family, OUT, {"cmi_allgather": FF, "cmi_allgatherv": FF, "cmi_halo_exchange": FF, "cmi_allreduce": ("f64",)}.get(family, ONE), reason=reason)
      for family, reason in OUT_OF_SCOPE.items()],
]
BY_FAMILY = {r.family: r for r in ROWS}


def cases(cls):
    """(family, suffix) of every case of one class, in table order."""
    return [(r.family, t) for r in ROWS if r.cls == cls for t in r.types]


def build(ctx, family, suffix):
    row = BY_FAMILY[family]
    return row.builder(ctx, TYPES.get(suffix, np.float64))

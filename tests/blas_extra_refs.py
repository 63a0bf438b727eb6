"""References for the kernels of csrc/blas1_extra.hip (test infrastructure shared by test_blas_extra_refs.py, which checks
these references against exact rational arithmetic on the CPU, and test_blas_extra_gpu.py, which checks the kernels against them).

Every element-wise kernel has two references:
  (a) `restate(T, s, v)`: numpy in type T, operation by operation in the order the kernel's comment documents.  The library is
      built with -ffp-contract=off, so the kernel's result is this fixed sequence of IEEE operations: compared BIT FOR BIT.
  (b) `formula(s, v)`: the mathematical formula of the header, written once over any arithmetic (np.longdouble, np.float64
      or fractions.Fraction in object arrays).  It returns, per output vector, (value, sum of |terms|); a result in T must lie
      within k * u * sum|terms| of it, u the unit roundoff of T and k (`KERNELS[name].k[output]`) the number of roundings on the longest
      path to the output: each scalar rounded to T counts one, each multiply one, each add one.
`s` maps the names of the device scalars (Python floats, i.e. doubles) and `v` the operand names to arrays.
`sums(T, got, v)` names, per reduction result, the two factor arrays whose products the kernel sums in double, taken from the
vectors the kernel RETURNED (`got`)."""
import math
from fractions import Fraction

import numpy as np

U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
HIGHER = {np.float32: np.float64, np.float64: np.longdouble}


class Kernel:
    def __init__(self, name, scalars, vecs, outputs, k, restate, formula, sums=None, by_value=False):
        self.name, self.scalars, self.vecs, self.outputs, self.k = name, scalars, vecs, outputs, k
        self.restate, self.formula, self.sums = restate, formula, sums or (lambda T, got, v: {})
        self.by_value = by_value  # scalars are passed by value in T (and must be representable in T), not as device doubles

    @property
    def const(self):
        return tuple(n for n in self.vecs if n not in self.outputs)


def _q(T, num, den):
    """The device's scalar: the double quotient of two device doubles, rounded to T once."""
    return T(np.float64(num) / np.float64(den))


# ---- scal / xmy / axpbypcz: scalars by value ---------------------------------------------------------------------------------
def _r_scal(T, s, v):
    return {"x": T(s["a"]) * v["x"]}


def _f_scal(s, v):
    t = s["a"] * v["x"]
    return {"x": (t, abs(t))}


def _r_xmy(T, s, v):
    return {"z": v["x"] * v["y"]}


def _f_xmy(s, v):
    t = v["x"] * v["y"]
    return {"z": (t, abs(t))}


def _r_axpbypcz(T, s, v):
    return {"out": (T(s["a"]) * v["x"] + T(s["b"]) * v["y"]) + T(s["c"]) * v["z"]}


def _f_axpbypcz(s, v):
    t1, t2, t3 = s["a"] * v["x"], s["b"] * v["y"], s["c"] * v["z"]
    return {"out": (t1 + t2 + t3, abs(t1) + abs(t2) + abs(t3))}


# ---- Jacobi-preconditioned cg ---------------------------------------------------------------------------------------------------
def _r_pcg_update(T, s, v):
    alpha = _q(T, s["rz"], s["yp"])
    return {"r": v["r"] - alpha * v["y"]}


def _f_pcg_update(s, v):
    t = (s["rz"] / s["yp"]) * v["y"]
    return {"r": (v["r"] - t, abs(v["r"]) + abs(t))}


def _s_pcg_update(T, got, v):
    r = got["r"]
    return {"rz_new": (r, v["dinv"] * r), "rr": (r, r)}  # <r, D^-1 r> with D^-1 r rounded to T, as the kernel forms it


def _r_pcg_direction(T, s, v):
    alpha, beta = _q(T, s["rz_old"], s["yp"]), _q(T, s["rz_new"], s["rz_old"])
    return {"x": v["x"] + alpha * v["p"], "p": v["dinv"] * v["r"] + beta * v["p"]}


def _f_pcg_direction(s, v):
    t1, t2, t3 = (s["rz_old"] / s["yp"]) * v["p"], v["dinv"] * v["r"], (s["rz_new"] / s["rz_old"]) * v["p"]
    return {"x": (v["x"] + t1, abs(v["x"]) + abs(t1)), "p": (t2 + t3, abs(t2) + abs(t3))}


# ---- BiCGstab ---------------------------------------------------------------------------------------------------------------------
def _r_bicg_s(T, s, v):
    alpha = _q(T, s["rho"], s["d1"])
    return {"s": v["r"] - alpha * v["AMp"]}


def _f_bicg_s(s, v):
    t = (s["rho"] / s["d1"]) * v["AMp"]
    return {"s": (v["r"] - t, abs(v["r"]) + abs(t))}


def _s_bicg_s(T, got, v):
    return {"ss": (got["s"], got["s"])}


def _r_bicg_xr(T, s, v):
    alpha, omega = _q(T, s["rho"], s["d1"]), _q(T, s["d2"], s["d3"])
    return {"x": (v["x"] + alpha * v["p"]) + omega * v["s"], "r": v["s"] - omega * v["AMs"]}


def _f_bicg_xr(s, v):
    alpha, omega = s["rho"] / s["d1"], s["d2"] / s["d3"]
    t1, t2, t3 = alpha * v["p"], omega * v["s"], omega * v["AMs"]
    return {"x": (v["x"] + t1 + t2, abs(v["x"]) + abs(t1) + abs(t2)), "r": (v["s"] - t3, abs(v["s"]) + abs(t3))}


def _s_bicg_xr(T, got, v):
    return {"rho_new": (v["r_star"], got["r"]), "rr": (got["r"], got["r"])}


def _r_bicg_p(T, s, v):
    f = np.float64
    alpha, omega = f(s["rho"]) / f(s["d1"]), f(s["d2"]) / f(s["d3"])  # both kept in double here
    beta = T((f(s["rho_new"]) / f(s["rho"])) * (alpha / omega))
    bo = T(-f(beta) * omega)
    return {"p": (v["r"] + beta * v["p"]) + bo * v["AMp"]}


def _f_bicg_p(s, v):
    alpha, omega = s["rho"] / s["d1"], s["d2"] / s["d3"]
    beta = (s["rho_new"] / s["rho"]) * (alpha / omega)
    t1, t2 = beta * v["p"], beta * omega * v["AMp"]
    return {"p": (v["r"] + t1 - t2, abs(v["r"]) + abs(t1) + abs(t2))}


# ---- conjugate residuals ----------------------------------------------------------------------------------------------------------
def _r_cr_xr(T, s, v):
    alpha = _q(T, s["rz"], s["yy"])
    return {"x": v["x"] + alpha * v["p"], "r": v["r"] - alpha * v["y"]}


def _f_cr_xr(s, v):
    alpha = s["rz"] / s["yy"]
    t1, t2 = alpha * v["p"], alpha * v["y"]
    return {"x": (v["x"] + t1, abs(v["x"]) + abs(t1)), "r": (v["r"] - t2, abs(v["r"]) + abs(t2))}


def _s_cr_xr(T, got, v):
    return {"rr": (got["r"], got["r"])}


def _r_cr_py(T, s, v):
    beta = _q(T, s["rz_new"], s["rz"])
    return {"p": v["r"] + beta * v["p"], "y": v["Ar"] + beta * v["y"]}


def _f_cr_py(s, v):
    beta = s["rz_new"] / s["rz"]
    t1, t2 = beta * v["p"], beta * v["y"]
    return {"p": (v["r"] + t1, abs(v["r"]) + abs(t1)), "y": (v["Ar"] + t2, abs(v["Ar"]) + abs(t2))}


def _s_cr_py(T, got, v):
    return {"yy_new": (got["y"], got["y"])}


# ---- GMRES's Gram-Schmidt step, bicgstab's last x update ------------------------------------------------------------------------------
def _r_axpy_dot(T, s, v):
    return {"w": v["w"] - T(s["h"]) * v["v"]}


def _f_axpy_dot(s, v):
    t = s["h"] * v["v"]
    return {"w": (v["w"] - t, abs(v["w"]) + abs(t))}


def _s_axpy_dot(T, got, v):
    return {"out": (got["w"], v["u"])}


def _r_axpy_ratio(T, s, v):
    return {"y": v["y"] + _q(T, s["num"], s["den"]) * v["x"]}


def _f_axpy_ratio(s, v):
    t = (s["num"] / s["den"]) * v["x"]
    return {"y": (v["y"] + t, abs(v["y"]) + abs(t))}


# k per output: the roundings on the longest path (scalar -> T, multiply, add count one each)
KERNELS = {k.name: k for k in (
    Kernel("scal", ("a",), ("x",), ("x",), {"x": 1}, _r_scal, _f_scal, by_value=True),                        # a x: 1 multiply
    Kernel("xmy", (), ("x", "y", "z"), ("z",), {"z": 1}, _r_xmy, _f_xmy),                                    # x y: 1 multiply
    Kernel("axpbypcz", ("a", "b", "c"), ("x", "y", "z", "out"), ("out",), {"out": 3}, _r_axpbypcz, _f_axpbypcz, by_value=True),  # a x: multiply, add, add
    Kernel("pcg_update", ("rz", "yp"), ("y", "r", "dinv"), ("r",), {"r": 3}, _r_pcg_update, _f_pcg_update, _s_pcg_update),  # alpha -> T, alpha y, r - .
    Kernel("pcg_direction", ("rz_new", "rz_old", "yp"), ("r", "dinv", "p", "x"), ("p", "x"), {"x": 3, "p": 3},  # x: alpha -> T, alpha p, add; p: beta -> T, beta p, add
           _r_pcg_direction, _f_pcg_direction),
    Kernel("bicg_s", ("rho", "d1"), ("r", "AMp", "s"), ("s",), {"s": 3}, _r_bicg_s, _f_bicg_s, _s_bicg_s),    # alpha -> T, alpha AMp, r - .
    Kernel("bicg_xr", ("rho", "d1", "d2", "d3"), ("p", "s", "AMs", "r_star", "x", "r"), ("x", "r"), {"x": 4, "r": 3},  # x: alpha -> T, alpha p, add, add; r: omega -> T, omega AMs, s - .
           _r_bicg_xr, _f_bicg_xr, _s_bicg_xr),
    # p: the AMp term: alpha, omega (2 double quotients), rho_new / rho, alpha / omega, their product, beta -> T, beta omega, bo -> T, bo AMp, the last add
    Kernel("bicg_p", ("rho_new", "rho", "d1", "d2", "d3"), ("r", "AMp", "p"), ("p",), {"p": 10}, _r_bicg_p, _f_bicg_p),
    Kernel("cr_xr", ("rz", "yy"), ("p", "y", "x", "r"), ("x", "r"), {"x": 3, "r": 3}, _r_cr_xr, _f_cr_xr, _s_cr_xr),  # alpha -> T, multiply, add
    Kernel("cr_py", ("rz_new", "rz"), ("r", "Ar", "p", "y"), ("p", "y"), {"p": 3, "y": 3}, _r_cr_py, _f_cr_py, _s_cr_py),  # beta -> T, multiply, add
    Kernel("axpy_dot", ("h",), ("v", "w", "u"), ("w",), {"w": 3}, _r_axpy_dot, _f_axpy_dot, _s_axpy_dot),  # h -> T, h v, w - .
    Kernel("axpy_ratio", ("num", "den"), ("x", "y"), ("y",), {"y": 3}, _r_axpy_ratio, _f_axpy_ratio),         # a -> T, a x, add
)}

# device scalars: quotients that are NOT representable (1.75 / 0.6, ...) and, to tell a wrong scalar from wrong vector code, exact ones (3 / -1.5, ...)
SCALARS = {
    "inexact": {"rz": 1.75, "yp": 0.6, "rz_new": 0.9, "rz_old": 1.75, "rho": 1.75, "d1": 0.6, "d2": -0.7, "d3": 1.3, "rho_new": 1.1, "yy": 0.6,
                "h": 0.1, "num": 1.75, "den": 0.6},
    "exact": {"rz": 3.0, "yp": -1.5, "rz_new": 0.75, "rz_old": 3.0, "rho": 3.0, "d1": -1.5, "d2": 0.5, "d3": 2.0, "rho_new": -6.0, "yy": -1.5,
              "h": -0.5, "num": 3.0, "den": -1.5},
}


def scalars_for(kernel, kind, T):
    """The scalars of one kernel; the by-value ones (scal, axpbypcz) are made representable in T: the caller hands them over exactly."""
    if kernel.by_value:
        vals = {"inexact": {"a": 1.75 / 0.6, "b": -0.7 / 1.3, "c": 0.1}, "exact": {"a": -2.0, "b": 0.5, "c": 0.25}}[kind]
        return {n: float(T(vals[n])) for n in kernel.scalars}
    return {n: SCALARS[kind][n] for n in kernel.scalars}


def higher(T, s, v):
    """s and v in the precision above T (float64 for f32, longdouble for f64)."""
    H = HIGHER[T]
    return {n: H(x) for n, x in s.items()}, {n: a.astype(H) for n, a in v.items()}


def rational(s, v):
    """s and v as exact rationals (object arrays of Fraction)."""
    def arr(a):
        out = np.empty(len(a), dtype=object)
        out[:] = [Fraction(float(x)) for x in a]
        return out
    return {n: Fraction(float(x)) for n, x in s.items()}, {n: arr(a) for n, a in v.items()}


def exact_sum(a, b):
    """(sum of a_i b_i, sum of |a_i b_i|) with the products formed in double (exact for f32 factors) and summed exactly."""
    prod = (np.asarray(a, np.float64) * np.asarray(b, np.float64)).tolist()
    return math.fsum(prod), math.fsum(map(abs, prod))


def amax_ref(x):
    """(largest |x_i|, FIRST position holding it), NaNs skipped; empty or all-NaN: (0, 0)."""
    best, at = -1.0, 0
    for i, xi in enumerate(np.asarray(x, np.float64).tolist()):
        a = abs(xi)
        if a > best:  # false for NaN; a later equal value does not replace an earlier one
            best, at = a, i
    return (0.0, 0) if best < 0 else (best, at)


def amax_ref_fast(x):
    """amax_ref for long vectors (numpy; test_blas_extra_refs.py checks it against the loop)."""
    a = np.abs(np.asarray(x, np.float64))
    if a.size == 0 or np.all(np.isnan(a)):
        return 0.0, 0
    at = int(np.nanargmax(a))  # the first occurrence of the maximum
    return float(a[at]), at


def csr_diagonal_ref(T, num_rows, Ap, Aj, Ax, reciprocal):
    """Row i: the entries stored in column i summed in type T in storage order from 0 (none: 0), or 1 / that."""
    d = np.zeros(num_rows, T)
    for i in range(num_rows):
        acc = T(0)
        for jj in range(Ap[i], Ap[i + 1]):
            if Aj[jj] == i:
                acc = T(acc + Ax[jj])
        d[i] = acc
    return _reciprocal(T, d) if reciprocal else d


def _reciprocal(T, d):
    with np.errstate(divide="ignore"):
        return (T(1) / d).astype(T)


def csr_diagonal_ref_fast(T, num_rows, Ap, Aj, Ax, reciprocal):
    """csr_diagonal_ref for many rows: pass t adds every row's t-th stored diagonal entry, so each row still sums in storage order
    (test_blas_extra_refs.py checks it against the loop)."""
    Ap = np.asarray(Ap, np.int64)
    Aj, Ax = np.asarray(Aj, np.int64)[:Ap[-1]], np.asarray(Ax)[:Ap[-1]]  # the arrays may be longer than the rows use
    row = np.repeat(np.arange(num_rows, dtype=np.int64), np.diff(Ap))
    hit = np.nonzero(Aj == row)[0]                       # in storage order
    rows, vals = row[hit], np.asarray(Ax, T)[hit]
    first = np.searchsorted(rows, rows, side="left")     # rows is sorted: position of each row's first hit
    rank = np.arange(len(rows)) - first
    d = np.zeros(num_rows, T)
    for t in range(int(rank.max()) + 1 if len(rank) else 0):
        sel = rank == t
        d[rows[sel]] = d[rows[sel]] + vals[sel]
    return _reciprocal(T, d) if reciprocal else d


def hand_made_matrix(T):
    """6 x 4 (more rows than columns; rows 4 and 5 have no column of their own):
    row 0: diagonal first; row 1: diagonal in the middle, columns unsorted; row 2: empty; row 3: diagonal last and stored twice;
    row 4: entries but no diagonal (its column 4 does not exist); row 5: empty."""
    Ap = np.array([0, 3, 6, 6, 10, 12, 12], np.int32)
    Aj = np.array([0, 2, 1,  3, 1, 0,  3, 0, 1, 3,  0, 2], np.int32)
    Ax = np.array([0.1, 5.0, 6.0,  7.0, 0.3, 8.0,  1e8, 9.0, 10.0, 0.7,  11.0, 12.0]).astype(T)
    return 6, Ap, Aj, Ax

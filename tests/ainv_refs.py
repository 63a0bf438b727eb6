"""Plain restatement of the three AINV factorisations of cusp/precond/ainv.h (Bridson's outer-product form with a drop tolerance and the
Lin-More bound on the entries per row), one rounding per operation in the value type (numpy scalars), or exact with fractions.Fraction.

The factor row is the header's container: the entries by index and a binary min-heap on |value| whose tie rules decide which entry is dropped:
  * every comparison is a strict < on absolute values;
  * sift-down takes the second child only when it is strictly smaller than the first, and moves the node while either child is strictly smaller;
  * a value update sifts up when the new value is strictly smaller in magnitude, otherwise down;
  * removal swaps the root with the last slot, shrinks, then sifts the new root down.
`mutants` (a set of names, empty for the real rule) switches single rules to a plausible wrong form, for the tests that show each is caught:
  tol_le            a term is skipped when |term| <= tolerance
  replace_strict    a new index replaces the minimum only when strictly greater than it
  cap_after         the bound is tested as if the entry were already in: a row may hold row_count + 1 entries
  sift_second       sift-down prefers the second child on ties
  lin_nofloor       the Lin-More bound without its floor of 1
"""
import bisect
from fractions import Fraction

import numpy as np

MUTANTS = ("tol_le", "replace_strict", "cap_after", "sift_second", "lin_nofloor")


def less_abs(a, b):
    return (-a if a < 0 else a) < (-b if b < 0 else b)


class Row:
    """index -> value in index order (keys + values dict) and the heap of indices by |value| (slot_of: index -> heap slot)"""

    def __init__(self, mutants=()):
        self.keys, self.value, self.slot_of, self.heap = [], {}, {}, []
        self.mutants = mutants

    def __len__(self):
        return len(self.keys)

    def items(self):
        return [(i, self.value[i]) for i in self.keys]

    def has(self, i):
        return i in self.value

    def _exchange(self, a, b):
        h = self.heap
        h[a], h[b] = h[b], h[a]
        self.slot_of[h[a]], self.slot_of[h[b]] = a, b

    def _val(self, slot):
        return self.value[self.heap[slot]]

    def _up(self, s):
        while s != 0:
            parent = (s - 1) // 2
            if not less_abs(self._val(s), self._val(parent)):
                break
            self._exchange(s, parent)
            s = parent

    def _down(self, s):
        n = len(self.heap)
        while True:
            c0, c1 = 2 * s + 1, 2 * s + 2
            if c0 >= n:
                break
            smaller = c0
            if c1 < n:
                if "sift_second" in self.mutants:
                    if not less_abs(self._val(c0), self._val(c1)):
                        smaller = c1
                elif less_abs(self._val(c1), self._val(c0)):
                    smaller = c1
            if not (less_abs(self._val(c0), self._val(s)) or (c1 < n and less_abs(self._val(c1), self._val(s)))):
                break
            self._exchange(s, smaller)
            s = smaller

    def insert(self, i, v):
        if i not in self.value:
            bisect.insort(self.keys, i)
            self.value[i] = v
        self.heap.append(i)
        self.slot_of[i] = len(self.heap) - 1
        self._up(len(self.heap) - 1)

    def min_abs_value(self, zero):
        return self._val(0) if self.heap else zero

    def add_to_value(self, i, addend):
        before = self.value[i]
        self.value[i] = before + addend
        if less_abs(self.value[i], before):
            self._up(self.slot_of[i])
        else:
            self._down(self.slot_of[i])

    def remove_min(self):
        if not self.heap:
            return
        gone = self.heap[0]
        self._exchange(0, len(self.heap) - 1)
        self.heap.pop()
        self._down(0)
        del self.value[gone], self.slot_of[gone]
        self.keys.pop(bisect.bisect_left(self.keys, gone))

    def replace_min_if_greater(self, i, t, zero):
        m = self.min_abs_value(zero)
        refuse = (not less_abs(m, t)) if "replace_strict" in self.mutants else less_abs(t, m)
        if refuse:
            return
        self.remove_min()
        self.insert(i, t)

    def mult_by_scalar(self, s):
        for i in self.keys:
            self.value[i] = self.value[i] * s

    def validate_heap(self):
        n = len(self.heap)
        return all(less_abs(self._val(s), self._val(c)) for s in range(n) for c in (2 * s + 1, 2 * s + 2) if c < n)

    def validate_backpointers(self):
        return all(self.heap[self.slot_of[i]] == i for i in self.keys) and sorted(self.heap) == self.keys == sorted(self.value)


def add_row_dropping(result, mult, operand, tolerance, row_count, zero):
    """result += mult * operand, term by term under the drop rule"""
    mutants = result.mutants
    for i, v in operand.items():
        term = mult * v
        a = -term if term < 0 else term
        if (a <= tolerance) if "tol_le" in mutants else (a < tolerance):
            continue
        if result.has(i):
            result.add_to_value(i, term)
        elif row_count < 0 or (len(result) <= row_count if "cap_after" in mutants else len(result) < row_count):
            result.insert(i, term)
        else:
            result.replace_min_if_greater(i, term, zero)


def scatter_rows(Ap, Aj, Ax, row):
    """sum over the entries (k, x_k) of the factor row, in index order, of A's row k times x_k: index -> value (read in index order)"""
    b = {}
    for k, xk in row.items():
        for e in range(Ap[k], Ap[k + 1]):
            product = Ax[e] * xk
            c = int(Aj[e])
            b[c] = b[c] + product if c in b else product
    return b


def merge_dot(row, b, zero):
    s = zero
    for i, v in row.items():
        if i in b:
            s = s + v * b[i]
    return s


def row_count_of(Ap, i, per_row, lin, lin_param, mutants):
    if not lin:
        return per_row
    c = lin_param + int(Ap[i + 1] - Ap[i])
    return c if "lin_nofloor" in mutants else max(c, 1)


def transpose_csr(n, Ap, Aj, Ax):
    """rows of the transpose with ascending columns (a stable counting sort)"""
    Aj = np.asarray(Aj)
    rows = np.repeat(np.arange(n), np.diff(Ap))
    order = np.argsort(Aj, kind="stable")
    Tp = np.zeros(n + 1, np.int32)
    np.add.at(Tp, Aj + 1, 1)
    Tp = np.cumsum(Tp).astype(np.int32)
    Tx = [Ax[e] for e in order] if isinstance(Ax, list) else np.asarray(Ax)[order]
    return Tp, rows[order].astype(np.int32), Tx


def rows_to_csr(rows, dtype):
    Wp, Wj, Wx = [0], [], []
    for r in rows:
        for i, v in r.items():
            Wj.append(i)
            Wx.append(v)
        Wp.append(len(Wj))
    Wx = Wx if dtype is Fraction else np.array(Wx, dtype)
    return np.array(Wp, np.int32), np.array(Wj, np.int32), Wx


class PivotError(ValueError):
    pass


def factor(kind, n, Ap, Aj, Ax, dtype, tol=0.1, per_row=-1, lin=False, lin_param=1, mutants=()):
    """kind: "scaled" | "bridson" | "nonsym"; dtype: np.float32 | np.float64 | Fraction (not for "scaled": its root is not rational).
    Returns {"w": csr, "w_t": csr, "diagonals": array} ("z" instead of "w" for nonsym; no diagonals for scaled), csr = (offsets, columns, values)."""
    t = dtype
    exact = dtype is Fraction
    Ax = [Fraction(float(v)) for v in Ax] if exact else np.asarray(Ax, dtype)
    Ap = np.asarray(Ap)
    zero, one, tol = t(0), t(1), (Fraction(tol) if exact else t(tol))
    mutants = frozenset(mutants)

    def identity():
        rows = [Row(mutants) for _ in range(n)]
        for i, r in enumerate(rows):
            r.insert(i, one)
        return rows

    def update(rows, j, u, scalar_of):
        for i in sorted(k for k in u if k > j):
            add_row_dropping(rows[i], scalar_of(u[i]), rows[j], tol, row_count_of(Ap, i, per_row, lin, lin_param, mutants), zero)

    def recip(p):  # 1.0 / p formed in double, then cast
        return one / p if exact else t(1.0 / float(p))

    diag = []
    if kind == "nonsym":
        Tp, Tj, Tx = transpose_csr(n, Ap, Aj, Ax)
        wt, z = identity(), identity()
        for j in range(n):
            u = scatter_rows(Tp, Tj, Tx, wt[j])
            l = scatter_rows(Ap, Aj, Ax, z[j])
            p = merge_dot(wt[j], l, zero)
            if p == 0 or p != p:
                raise PivotError(j)
            diag.append(recip(p))
            update(z, j, u, lambda ui: -ui / p)
            update(wt, j, l, lambda li: -li / p)
        w = rows_to_csr(wt, dtype)
        return {"z": rows_to_csr(z, dtype), "w_t": transpose_csr(n, *w), "diagonals": diag if exact else np.array(diag, dtype)}
    rows = identity()
    for j in range(n):
        u = scatter_rows(Ap, Aj, Ax, rows[j])
        p = merge_dot(rows[j], u, zero)
        if kind == "scaled":
            if not p > 0:
                raise PivotError(j)
            s = t(1.0 / float(np.sqrt(p)))  # the root in the value type, the quotient in double
            u = {k: v * s for k, v in u.items()}
            rows[j].mult_by_scalar(s)
            update(rows, j, u, lambda ui: -ui)
        else:
            if p == 0 or p != p:
                raise PivotError(j)
            diag.append(recip(p))
            update(rows, j, u, lambda ui: -ui / p)
    w = rows_to_csr(rows, dtype)
    out = {"w": w, "w_t": transpose_csr(n, *w)}
    if kind == "bridson":
        out["diagonals"] = diag if exact else np.array(diag, dtype)
    return out


def poisson5pt(m, n, dtype=np.float64, corner=10.0):
    """the 5-point Laplacian on an m x n grid (m the fast direction), rows with ascending columns, values[0] = corner"""
    Ap, Aj, Ax = [0], [], []
    for y in range(n):
        for x in range(m):
            i = y * m + x
            for c, v, ok in ((i - m, -1.0, y > 0), (i - 1, -1.0, x > 0), (i, 4.0, True), (i + 1, -1.0, x < m - 1), (i + m, -1.0, y < n - 1)):
                if ok:
                    Aj.append(c)
                    Ax.append(v)
            Ap.append(len(Aj))
    Ax = np.array(Ax, dtype)
    Ax[0] = corner
    return m * n, np.array(Ap, np.int32), np.array(Aj, np.int32), Ax


def nonsymmetric(m, n, dtype=np.float64):
    """poisson5pt(m, n) with values[0] = 10 and every entry above the diagonal halved"""
    N, Ap, Aj, Ax = poisson5pt(m, n, dtype)
    rows = np.repeat(np.arange(N), np.diff(Ap))
    Ax = np.where(Aj > rows, Ax * dtype(0.5), Ax).astype(dtype)
    return N, Ap, Aj, Ax


def dense(n, csr, as_type=Fraction):
    Wp, Wj, Wx = csr
    D = [[as_type(0)] * n for _ in range(n)]
    for i in range(n):
        for e in range(Wp[i], Wp[i + 1]):
            D[i][Wj[e]] = Wx[e] if isinstance(Wx[e], Fraction) else as_type(float(Wx[e]))
    return D


# the dropping settings of the C++ dump (tests/ainv/ainv_check.h settings())
SETTINGS = [(0.1, -1, False, 1), (0.0, 10, False, 1), (0.01, 4, False, 1), (0.0, -1, True, 4), (0.0, -1, True, -10)]

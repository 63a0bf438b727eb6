"""cusp::graph::vertex_coloring, the colour schedule of cusp::relaxation::gauss_seidel, its sweeps and cusp::relaxation::sor,
restated in numpy with one rounding per operation in the matrix's own type T -- plus three deliberately wrong variants.

Plain module: no fixtures, no GPU.  tests/test_gauss_seidel_refs.py proves these restatements against the literal answers of
the reference's own tests and against exact rational arithmetic, and that every mutant is caught;
tests/test_gauss_seidel_gpu.py compares the kernel and the classes with them bit for bit.

    colouring   colors = N - 1 everywhere; vertices in index order; a vertex marks the colours its own row's columns hold, takes
                the lowest unmarked colour below the current maximum, else opens a new one
    schedule    ordering = rows sorted by colour, ascending row index inside a colour; color_offsets = exclusive scan of the sizes
    one row     rsum = T(0); over row i in storage order: column i sets diag (the last one wins) and adds nothing, any other
                entry does rsum = rsum + Ax * x[Aj]; if diag != 0: x[i] = (b[i] - rsum) / diag, else x[i] stays
    sweep       FORWARD colours 0 .. C-1, BACKWARD C-1 .. 0 (rows inside a colour ascending in both), SYMMETRIC = both in turn;
                the rows of a colour are visited in order and read what is in x at that moment
    SOR         temp = x; sweep; x = (1 - omega) * temp + omega * x
"""
from fractions import Fraction

import numpy as np

FORWARD, BACKWARD, SYMMETRIC = 0, 1, 2
MUTANTS = ("diagonal_in_sum", "backward_reverses_rows", "conflicts_read_fresh")


def vertex_coloring(Ap, Aj):
    """(colors, number of colours) by the greedy rule above."""
    n = len(Ap) - 1
    colors = np.full(n, n - 1, np.int64)
    mark = np.full(max(n, 1), -1, np.int64)
    max_color = 0
    for v in range(n):
        for jj in range(int(Ap[v]), int(Ap[v + 1])):
            mark[colors[Aj[jj]]] = v
        c = 0
        while c < max_color and mark[c] == v:
            c += 1
        if c == max_color:
            max_color += 1
        colors[v] = c
    return colors.astype(np.int32), max_color


def schedule(colors, num_colors):
    """(ordering, color_offsets)."""
    ordering = np.argsort(colors, kind="stable").astype(np.int32)
    offsets = np.r_[0, np.cumsum(np.bincount(colors, minlength=num_colors))].astype(np.int32)
    return ordering, offsets


def conflicts(Ap, Aj, colors, num_colors):
    """flag[c] = some row of colour c holds an off-diagonal column of colour c."""
    rows = np.repeat(np.arange(len(Ap) - 1), np.diff(Ap))
    bad = (Aj != rows) & (colors[Aj] == colors[rows])
    flag = np.zeros(num_colors, bool)
    flag[colors[rows[bad]]] = True
    return flag


def relax_row(Ap, Aj, Ax, b, x_read, i, mutant=None):
    """(has a new value, the value) for row i reading x_read, in T."""
    T = Ax.dtype.type
    rsum, diag = T(0), T(0)
    with np.errstate(all="ignore"):
        for jj in range(int(Ap[i]), int(Ap[i + 1])):
            j = int(Aj[jj])
            if j == i:
                diag = Ax[jj]
                if mutant == "diagonal_in_sum":
                    rsum = rsum + Ax[jj] * x_read[j]
            else:
                rsum = rsum + Ax[jj] * x_read[j]     # numpy scalars of type T: one rounding per operation
        if diag != 0:                                 # false for +0, -0 and a missing diagonal; true for NaN
            return True, (b[i] - rsum) / diag
    return False, T(0)


def relax_slots(Ap, Aj, Ax, b, x, ordering, s0, s1, parked=False, reverse=False):
    """The rows ordering[s0:s1], in place.  parked=False: in order, each row reading x as it is then (the host loop).
    parked=True: every row reads the x from before the call (the two-launch form)."""
    src = x.copy() if parked else x
    slots = range(s1 - 1, s0 - 1, -1) if reverse else range(s0, s1)
    for s in slots:
        i = int(ordering[s])
        has, v = relax_row(Ap, Aj, Ax, b, src, i)
        if has:
            x[i] = v
    return x


class GaussSeidel:
    """cusp::relaxation::gauss_seidel<T>: gauss_seidel(A, direction = SYMMETRIC); relax(b, x) and relax(b, x, direction)
    return the new x."""

    def __init__(self, Ap, Aj, Ax, direction=SYMMETRIC):
        self.A = (Ap, Aj, Ax)
        self.colors, self.num_colors = vertex_coloring(Ap, Aj)
        self.ordering, self.color_offsets = schedule(self.colors, self.num_colors)
        self.color_conflicts = conflicts(Ap, Aj, self.colors, self.num_colors)
        self.default_direction = direction

    def colour(self, b, x, c, mutant=None):
        Ap, Aj, Ax = self.A
        s0, s1 = int(self.color_offsets[c]), int(self.color_offsets[c + 1])
        if mutant == "diagonal_in_sum":
            for s in range(s0, s1):
                i = int(self.ordering[s])
                has, v = relax_row(Ap, Aj, Ax, b, x, i, mutant)
                if has:
                    x[i] = v
            return
        if mutant == "conflicts_read_fresh":      # rows in DESCENDING order: a conflicting column (the larger index) is written first
            relax_slots(Ap, Aj, Ax, b, x, self.ordering, s0, s1, reverse=True)
            return
        relax_slots(Ap, Aj, Ax, b, x, self.ordering, s0, s1)

    def __call__(self, b, x, direction=None, mutant=None):
        x = np.array(x, self.A[2].dtype)
        direction = self.default_direction if direction is None else direction
        passes = {FORWARD: (FORWARD,), BACKWARD: (BACKWARD,), SYMMETRIC: (FORWARD, BACKWARD)}[direction]
        for d in passes:
            order = range(self.num_colors) if d == FORWARD else range(self.num_colors - 1, -1, -1)
            for c in order:
                if mutant == "backward_reverses_rows" and d == BACKWARD:
                    s0, s1 = int(self.color_offsets[c]), int(self.color_offsets[c + 1])
                    relax_slots(*self.A, b, x, self.ordering, s0, s1, reverse=True)
                else:
                    self.colour(b, x, c, mutant)
        return x


class Sor:
    """cusp::relaxation::sor<T>: sor(A, omega, direction = SYMMETRIC); relax(b, x) and relax(b, x, omega, direction)."""

    def __init__(self, Ap, Aj, Ax, omega, direction=SYMMETRIC):
        self.gs = GaussSeidel(Ap, Aj, Ax, direction)
        self.default_omega = Ax.dtype.type(omega)

    def __call__(self, b, x, omega=None, direction=None):
        T = self.gs.A[2].dtype.type
        omega = self.default_omega if omega is None else T(omega)
        temp = np.array(x, self.gs.A[2].dtype)
        swept = self.gs(b, x, direction)
        with np.errstate(all="ignore"):
            return (T(1) - omega) * temp + omega * swept


def from_dense(M, dtype):
    """CSR (Ap, Aj, Ax) of the non-zero entries of a dense matrix, as cusp::convert does."""
    M = np.asarray(M, dtype)
    keep = M != 0
    Ap = np.r_[0, np.cumsum(keep.sum(1))].astype(np.int32)
    return Ap, np.nonzero(keep)[1].astype(np.int32), M[keep]


# ------------------------------------------------------------------------------------------------
# exact arithmetic (the check of the restatements above; data on which nothing rounds)
# ------------------------------------------------------------------------------------------------
def exact_sweep(Ap, Aj, Ax, b, x, ordering, color_offsets, direction):
    """The sweep in Fractions, written independently: plain Python lists, the colours as lists of rows."""
    x = [Fraction(float(v)) for v in x]
    colours = [[int(i) for i in ordering[color_offsets[c]:color_offsets[c + 1]]] for c in range(len(color_offsets) - 1)]
    passes = {FORWARD: [colours], BACKWARD: [colours[::-1]], SYMMETRIC: [colours, colours[::-1]]}[direction]
    for order in passes:
        for rows in order:
            for i in rows:
                entries = [(int(Aj[jj]), Fraction(float(Ax[jj]))) for jj in range(int(Ap[i]), int(Ap[i + 1]))]
                on = [v for j, v in entries if j == i]
                if not on or on[-1] == 0:
                    continue
                x[i] = (Fraction(float(b[i])) - sum((v * x[j] for j, v in entries if j != i), Fraction(0))) / on[-1]
    return x


def exact_sor(Ap, Aj, Ax, b, x, ordering, color_offsets, omega, direction):
    swept = exact_sweep(Ap, Aj, Ax, b, x, ordering, color_offsets, direction)
    w = Fraction(omega)
    return [(1 - w) * Fraction(float(t)) + w * s for t, s in zip(x, swept)]

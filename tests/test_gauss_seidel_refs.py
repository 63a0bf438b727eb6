"""CPU proof of tests/gauss_seidel_refs.py, the numpy restatement the GPU tests compare cusp::relaxation::gauss_seidel / sor
and cmi_csr_gauss_seidel_colour_* with: (a) the literal answers of the reference's own tests, (b) exact rational arithmetic
on small matrices on which nothing rounds, (c) three mutants, each of which must be caught."""
from fractions import Fraction

import numpy as np
import pytest

import gauss_seidel_refs as G

DTYPES = (np.float64, np.float32)
# the matrices of the reference's testing/gauss_seidel.cu
M5 = [[1, 1, 2, 0, 0], [3, 2, 0, 0, 5], [0, 0, 0.5, 0, 0], [0, 6, 7, 4, 0], [0, 8, 0, 0, 8]]
M2 = [[2, 1], [1, 3]]


def _small_matrices():
    """n <= 8, small integer values, diagonals that are powers of two (signed), patterns that are NOT symmetric, a row without a
    diagonal, a stored zero diagonal and a diagonal stored twice: with integer b and x every operation of two sweeps is exact
    in float32 already."""
    out = []
    rng = np.random.default_rng(7)
    for n in (1, 2, 5, 8):
        rows = []
        for i in range(n):
            others = [int(j) for j in rng.choice(n, size=min(n, int(rng.integers(0, 4))), replace=False) if j != i]
            ent = [(j, int(rng.integers(1, 4)) * int(rng.choice([-1, 1]))) for j in sorted(others)]
            d = float(rng.choice([1.0, 2.0, -1.0, -2.0, 4.0]))
            kind = (i + n) % 5
            if kind == 0 and n > 2:
                pass                                   # no diagonal entry: the row is left alone
            elif kind == 1 and n > 2:
                ent.append((i, 0.0))                   # a stored zero
            elif kind == 2 and n > 2:
                ent = [(i, 3.0)] + ent + [(i, d)]      # stored twice: the last wins, the first adds nothing
            else:
                ent.append((i, d))
            rows.append(ent)
        Ap = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int32)
        Aj = np.array([j for r in rows for j, _ in r], np.int32)
        Ax = np.array([v for r in rows for _, v in r], np.float64)
        out.append((n, Ap, Aj, Ax))
    return out


def test_reference_colouring_of_the_5x5_matrix():
    Ap, Aj, _ = G.from_dense(M5, np.float32)
    colors, n = G.vertex_coloring(Ap, Aj)
    assert colors.tolist() == [0, 1, 0, 2, 0] and n == 3
    ordering, offsets = G.schedule(colors, n)
    assert ordering.tolist() == [0, 2, 4, 1, 3] and offsets.tolist() == [0, 3, 4, 5]
    # rows 0 and 2 share colour 0 and row 0 holds column 2: the colour is flagged
    assert G.conflicts(Ap, Aj, colors, n).tolist() == [True, False, False]


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_reference_literal_answers(dtype):
    Ap, Aj, Ax = G.from_dense(M5, dtype)
    gs = G.GaussSeidel(Ap, Aj, Ax)
    x = gs(np.full(5, 5, dtype), np.full(5, -1, dtype))          # the default: SYMMETRIC
    assert x.dtype == dtype and x.tolist() == [-1.4375, -13.5625, 10.0, 4.09375, 14.1875]
    Ap, Aj, Ax = G.from_dense(M2, dtype)
    gs = G.GaussSeidel(Ap, Aj, Ax)
    b, x0 = np.full(2, 5, dtype), np.full(2, -1, dtype)
    fwd, bwd = gs(b, x0, G.FORWARD), gs(b, x0, G.BACKWARD)
    assert fwd[0] == 3 and fwd[1] == dtype(2) / dtype(3) and abs(float(fwd[1]) - 0.6666667) < 1e-6
    assert bwd.tolist() == [1.5, 2.0]
    assert x0.tolist() == [-1, -1]                                # the argument is not modified


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("direction", [G.FORWARD, G.BACKWARD, G.SYMMETRIC])
def test_against_exact_rational_arithmetic(dtype, direction):
    flagged = 0
    for n, Ap, Aj, Ax in _small_matrices():
        Ax = Ax.astype(dtype)
        b = np.arange(1, n + 1).astype(dtype)
        x0 = np.array([(-1) ** i * (i + 2) for i in range(n)], dtype)
        gs = G.GaussSeidel(Ap, Aj, Ax)
        flagged += int(gs.color_conflicts.sum())
        got = gs(b, x0, direction)
        want = G.exact_sweep(Ap, Aj, Ax, b, x0, gs.ordering, gs.color_offsets, direction)
        assert [Fraction(float(v)) for v in got] == want, (n, direction)
        # the parked form of a colour equals the in-order form: a conflicting column is the larger index, visited later
        for c in range(gs.num_colors):
            s0, s1 = int(gs.color_offsets[c]), int(gs.color_offsets[c + 1])
            a = G.relax_slots(Ap, Aj, Ax, b, x0.copy(), gs.ordering, s0, s1)
            p = G.relax_slots(Ap, Aj, Ax, b, x0.copy(), gs.ordering, s0, s1, parked=True)
            assert a.tolist() == p.tolist()
        sor = G.Sor(Ap, Aj, Ax, 0.5)
        got = sor(b, x0, direction=direction)
        want = G.exact_sor(Ap, Aj, Ax, b, x0, gs.ordering, gs.color_offsets, 0.5, direction)
        assert [Fraction(float(v)) for v in got] == want, (n, direction, "sor")
    assert flagged >= 1   # the set holds a colour whose rows depend on one another


def test_sor_with_omega_one_is_the_sweep():
    Ap, Aj, Ax = G.from_dense(M5, np.float64)
    b, x0 = np.full(5, 5.0), np.full(5, -1.0)
    assert G.Sor(Ap, Aj, Ax, 1.0)(b, x0).tolist() == G.GaussSeidel(Ap, Aj, Ax)(b, x0).tolist()
    half = G.Sor(Ap, Aj, Ax, 0.5)(b, x0)
    assert half.tolist() == [0.5 * -1 + 0.5 * v for v in [-1.4375, -13.5625, 10.0, 4.09375, 14.1875]]


@pytest.mark.parametrize("mutant", G.MUTANTS)
def test_every_mutant_is_caught(mutant):
    Ap, Aj, Ax = G.from_dense(M5, np.float64)
    gs = G.GaussSeidel(Ap, Aj, Ax)
    b, x0 = np.full(5, 5.0), np.full(5, -1.0)
    direction = G.BACKWARD if mutant == "backward_reverses_rows" else G.FORWARD
    good, bad = gs(b, x0, direction), gs(b, x0, direction, mutant=mutant)
    assert good.tolist() != bad.tolist(), mutant
    if mutant == "diagonal_in_sum":      # the diagonal's product is never formed: a NaN in x[i] does not reach row i's sum
        one = G.GaussSeidel(*G.from_dense([[2.0]], np.float64))
        assert one(np.array([4.0]), np.array([np.nan]), G.FORWARD).tolist() == [2.0]
        assert np.isnan(one(np.array([4.0]), np.array([np.nan]), G.FORWARD, mutant=mutant)[0])

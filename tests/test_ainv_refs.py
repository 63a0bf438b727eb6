"""CPU tests (-m "not gpu") of tests/ainv_refs.py, the plain restatement of the AINV factorisations that the C++ classes are compared with bit for
bit (tests/test_ainv_host.py): anchored in exact rational arithmetic, its tie rules pinned on hand-made rows, and every mutant of a rule caught."""
from fractions import Fraction

import numpy as np
import pytest

import ainv_refs as R

KINDS = ("scaled", "bridson", "nonsym")


def hash_unit(k):
    z = ((k + 1) * 0x9E3779B97F4A7C15) & (2**64 - 1)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
    return np.float32(((z ^ (z >> 31)) >> 40) / 16777216.0)


def test_heap_insert_update_remove_insert_keeps_both_invariants():
    """the reference's heap test as it stands (insert 100, update all, remove half, insert 100 more, then both validators), 40 trials"""
    seed = 0
    for _ in range(40):
        row = R.Row()
        for i in range(100):
            row.insert(i, hash_unit(seed)); seed += 1
        for i in range(100):
            row.add_to_value(i, hash_unit(seed) - np.float32(.5)); seed += 1
        for i in range(50):
            row.remove_min()
        for i in range(100):
            row.insert(i + 100, hash_unit(seed)); seed += 1
        assert len(row) == 150
        assert row.validate_heap()
        assert row.validate_backpointers()


def test_tie_rules_on_hand_made_rows():
    # sift-down: root 1 over the tied children b = 2, c = -2 and the leaf d = 5.  Removing the root puts d on top; it sinks below the FIRST child
    # (the second is not strictly smaller), so b is the next minimum and goes next: c and d remain.
    row = R.Row()
    for i, v in enumerate((1.0, 2.0, -2.0, 5.0)):
        row.insert(i, v)
    row.remove_min()
    assert row.min_abs_value(0.0) == 2.0 and row.heap[0] == 1
    row.remove_min()
    assert row.keys == [2, 3] and row.validate_backpointers()
    # a new index at a full row: strictly smaller than the minimum is refused, equal replaces it
    row = R.Row()
    row.insert(0, 1.0); row.insert(1, -2.0)
    R.add_row_dropping(row, 1.0, _row({5: 0.5}), 0.0, 2, 0.0)
    assert row.keys == [0, 1]
    R.add_row_dropping(row, 1.0, _row({5: -1.0}), 0.0, 2, 0.0)
    assert row.keys == [1, 5]
    # the tolerance is strict: |term| == tolerance is kept; below a full bound an index simply enters
    row = R.Row()
    R.add_row_dropping(row, 0.5, _row({3: 1.0, 4: 0.9}), 0.5, 2, 0.0)
    assert row.items() == [(3, 0.5)]
    # an update sifts up only when strictly smaller in magnitude
    row = R.Row()
    for i, v in enumerate((1.0, 2.0, 3.0)):
        row.insert(i, v)
    row.add_to_value(2, -2.5)  # 3 -> 0.5: to the root
    assert row.heap[0] == 2
    row.add_to_value(2, 1.5)   # 0.5 -> 2: down, past the first child 2? no: 2 is not strictly smaller than 2, but 1 is
    assert row.heap[0] == 0 and row.validate_backpointers()
    # the Lin-More bound: lin_param + the row's length, not below 1
    Ap = np.array([0, 3, 5])
    assert R.row_count_of(Ap, 0, 7, True, 4, ()) == 7 and R.row_count_of(Ap, 1, 7, True, -10, ()) == 1 and R.row_count_of(Ap, 1, 7, False, 4, ()) == 7


def _row(d):
    r = R.Row()
    for i, v in d.items():
        r.insert(i, v)
    return r


class Exact:
    """a matrix of rationals whose denominators are powers of two -- what floats are -- as integers over one power of two: products and sums are
    exact integer arithmetic (fractions.Fraction with the common denominator kept out of the loops)"""

    def __init__(self, ints, shift):
        self.m, self.shift = ints, shift

    @classmethod
    def of(cls, rows):
        fr = [[v if isinstance(v, Fraction) else Fraction(float(v)) for v in r] for r in rows]
        shift = max(v.denominator.bit_length() - 1 for r in fr for v in r)
        assert all((1 << shift) % v.denominator == 0 for r in fr for v in r), "not a matrix of dyadic rationals"
        return cls(np.array([[int(v * (1 << shift)) for v in r] for r in fr], dtype=object), shift)

    def __matmul__(self, o):
        return Exact(self.m.dot(o.m), self.shift + o.shift)

    def abs(self):
        return Exact(np.abs(self.m), self.shift)

    def at(self, i, j):
        return Fraction(int(self.m[i, j]), 1 << self.shift)

    def max(self, keep=lambda i, j: True):
        n = len(self.m)
        return Fraction(max(int(self.m[i, j]) for i in range(n) for j in range(n) if keep(i, j)), 1 << self.shift)


def exact_products(kind, n, Ap, Aj, Ax, f):
    """the factor's values as exact rationals: A, the first factor F (W or Z), W^T D and W^T; M = (W^T D) F"""
    A = Exact.of(R.dense(n, (Ap, Aj, Ax)))
    first = Exact.of(R.dense(n, f["z"] if kind == "nonsym" else f["w"]))
    Wt = R.dense(n, f["w_t"])
    d = [v if isinstance(v, Fraction) else Fraction(float(v)) for v in f["diagonals"]] if kind != "scaled" else [Fraction(1)] * n
    return A, first, Exact.of([[Wt[i][k] * d[k] for k in range(n)] for i in range(n)]), Exact.of(Wt)


@pytest.mark.parametrize("kind,problem", [("bridson", "poisson 4x3"), ("nonsym", "poisson 4x3"), ("nonsym", "nonsymmetric 4x3")])
def test_exact_run_inverts_the_matrix_exactly(kind, problem):
    """drop_tolerance 0 and no bound, in fractions: W A W^T (nonsym: Z A W^T) is diagonal with the pivots, and M A is the identity, exactly"""
    n, Ap, Aj, Ax = R.poisson5pt(4, 3) if problem == "poisson 4x3" else R.nonsymmetric(4, 3)
    f = R.factor(kind, n, Ap, Aj, Ax, Fraction, tol=0, per_row=-1)
    d = f["diagonals"]
    Wt = R.dense(n, f["w_t"])
    F1 = R.dense(n, f["z"] if kind == "nonsym" else f["w"])
    A = R.dense(n, (Ap, Aj, Ax))
    mul = lambda X, Y: [[sum(X[i][k] * Y[k][j] for k in range(n)) for j in range(n)] for i in range(n)]  # noqa: E731
    MA = mul([[Wt[i][k] * d[k] for k in range(n)] for i in range(n)], mul(F1, A))
    FAWt = mul(mul(F1, A), Wt)
    assert all(MA[i][j] == (1 if i == j else 0) for i in range(n) for j in range(n))
    assert all(FAWt[i][j] == (1 / d[i] if i == j else 0) for i in range(n) for j in range(n))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind,problem", [(k, p) for k in KINDS for p in ("poisson 4x3", "poisson 10x10")] + [("nonsym", "nonsymmetric 4x3")])
def test_float_run_inverts_the_matrix_to_rounding(kind, problem, dtype):
    """drop_tolerance 0 and no bound in the value type: with the factor's values taken as exact rationals, |M A - I| stays within the rounding of the
    run.  The bound: every entry of M A is a sum of at most n products of three factor entries, each of which went through at most n updates of a
    handful of roundings, so the error relative to |M| |A| is a modest multiple of n eps: 16 n eps max_i sum_j (|M| |A|)_ij; the off-diagonal of
    W A W^T is held in the same way against the largest entry of |W| |A| |W^T|."""
    m, k = (10, 10) if problem.endswith("10x10") else (4, 3)
    n, Ap, Aj, Ax = (R.nonsymmetric if problem.startswith("nonsym") else R.poisson5pt)(m, k, dtype)
    f = R.factor(kind, n, Ap, Aj, Ax, dtype, tol=0, per_row=-1)
    assert (f["z"] if kind == "nonsym" else f["w"])[2].dtype == dtype
    A, F1, WtD, Wt = exact_products(kind, n, Ap, Aj, Ax, f)
    eps = Fraction(float(np.finfo(dtype).eps))
    MA = WtD @ (F1 @ A)
    err = max(abs(MA.at(i, j) - (1 if i == j else 0)) for i in range(n) for j in range(n))
    scale = max(sum(row) for row in (WtD.abs() @ (F1.abs() @ A.abs())).m)  # the largest row sum of |W^T D| |F| |A|
    bound = 16 * n * eps * Fraction(int(scale), 1 << (WtD.shift + F1.shift + A.shift))
    print(f"{kind} {problem} {np.dtype(dtype).name}: |M A - I| = {float(err):.3e}, bound {float(bound):.3e}")
    assert err <= bound
    off = (F1 @ A @ Wt).abs().max(lambda i, j: i != j)
    bound = 16 * n * eps * (F1.abs() @ A.abs() @ Wt.abs()).max()
    print(f"    off-diagonal of F A W^T: {float(off):.3e}, bound {float(bound):.3e}")
    assert off <= bound


def cases():
    """(name, n, Ap, Aj, Ax, setting) on which the rules bite: the dump's settings on a small Poisson problem and a matrix made to tie"""
    out = []
    n, Ap, Aj, Ax = R.poisson5pt(6, 5)
    for s in R.SETTINGS:
        out.append((f"poisson 6x5 {s}", n, Ap, Aj, Ax, s))
    # [[2, -2, 0], [-2, 5, -1], [0, -1, 3]] with one entry per row: the term for row 1 at step 0 is 1 = |the row's only entry|: a tie at a full row
    # an arrow: rows 0..4 hold (d_i, -1), row 5 all of them; d = (2, 2, 2, 1, 1, 16), four entries per row: row 5 collects 1/d_j at index j, ties among
    # the halves sit side by side in its heap when the ones arrive and push them out
    d = [2., 2., 2., 1., 1., 16.]
    out.append(("arrow 6", 6, np.array([0, 2, 4, 6, 8, 10, 16]), np.array([0, 5, 1, 5, 2, 5, 3, 5, 4, 5, 0, 1, 2, 3, 4, 5]),
                np.array([d[0], -1, d[1], -1, d[2], -1, d[3], -1, d[4], -1, -1, -1, -1, -1, -1, d[5]]), (0.0, 4, False, 1)))
    out.append(("tie 3x3", 3, np.array([0, 2, 5, 7]), np.array([0, 1, 0, 1, 2, 1, 2]), np.array([2., -2., -2., 5., -1., -1., 3.]), (0.0, 1, False, 1)))
    return out


def same_factor(a, b):
    keys = sorted(a)
    return keys == sorted(b) and all(
        (np.array_equal(a[k], b[k]) if k == "diagonals" else all(np.array_equal(x, y) for x, y in zip(a[k], b[k]))) for k in keys)


def test_the_arrow_by_hand():
    """row 5 = {5: 1} takes 1/2 at 0, 1, 2 (heap slots: 0, 2, 1, 5 by index); the 1 at index 3 removes the root (index 0): the last slot (index 5,
    value 1) comes to the top and sinks below its FIRST child (index 2), the second being tied, not smaller; the 1 at index 4 then removes index 2.
    Indices 1, 3, 4, 5 remain (a sift-down that preferred the second child on ties would keep 2 instead of 1)."""
    _, n, Ap, Aj, Ax, s = cases()[-2]
    Wp, Wj, Wx = R.factor("bridson", n, Ap, Aj, Ax, np.float64, *s)["w"]
    assert Wj[Wp[5]:].tolist() == [1, 3, 4, 5] and Wx[Wp[5]:].tolist() == [0.5, 1.0, 1.0, 1.0]


def test_the_tie_matrix_by_hand():
    _, n, Ap, Aj, Ax, s = cases()[-1]
    f = R.factor("bridson", n, Ap, Aj, Ax, np.float64, *s)
    Wp, Wj, Wx = f["w"]
    # row 1 held {1: 1}; the term -(-2)/2 * 1 = 1 at index 0 ties with it and takes its place
    assert Wj[Wp[1]:Wp[2]].tolist() == [0] and Wx[Wp[1]] == 1.0
    assert f["diagonals"][0] == 0.5


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_is_caught(mutant):
    caught = []
    for name, n, Ap, Aj, Ax, s in cases():
        for kind in ("bridson", "scaled"):
            if not same_factor(R.factor(kind, n, Ap, Aj, Ax, np.float64, *s), R.factor(kind, n, Ap, Aj, Ax, np.float64, *s, mutants=(mutant,))):
                caught.append((name, kind))
    print(mutant, "caught on", caught)
    assert caught, f"no case distinguishes the mutant {mutant}"


def test_symmetric_and_nonsymmetric_class_agree_on_a_symmetric_matrix():
    n, Ap, Aj, Ax = R.poisson5pt(9, 7, np.float32)
    for s in R.SETTINGS[:4]:
        a, b = R.factor("bridson", n, Ap, Aj, Ax, np.float32, *s), R.factor("nonsym", n, Ap, Aj, Ax, np.float32, *s)
        assert same_factor({"w": a["w"], "w_t": a["w_t"], "diagonals": a["diagonals"]}, {"w": b["z"], "w_t": b["w_t"], "diagonals": b["diagonals"]})


def test_pivots_that_cannot_be_used_are_refused():
    Ap, Aj = np.array([0, 2, 4]), np.array([0, 1, 0, 1])
    for kind in KINDS:
        with pytest.raises(R.PivotError):
            R.factor(kind, 2, Ap, Aj, np.ones(4), np.float64, tol=0)
    with pytest.raises(R.PivotError):
        R.factor("scaled", 2, np.array([0, 1, 2]), np.array([0, 1]), -np.ones(2), np.float64, tol=0)

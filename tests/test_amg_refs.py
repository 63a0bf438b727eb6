"""tests/amg_refs.py against exact rational arithmetic, against scipy, and against its own mutants (CPU only).

The references are the yardstick of tests/test_amg_gpu.py, so they are checked three ways: sums against Fractions where the
inputs make every partial sum representable; structure against scipy's own filter / add / subtract / triple product; and one
deliberately wrong variant per stated order (amg_refs.MUTANTS), each of which a deck here must catch.
"""
from fractions import Fraction

import numpy as np
import pytest

import amg_refs as R
import spgemm_refs as SR
from special_values import bits_differ, same_bits

import scipy.sparse as sp
DT = list(R.DTYPES)


def scipy_csr(M):
    rows, cols, Ap, Aj, Ax = M
    return sp.csr_matrix((Ax.astype(np.float64), Aj, Ap), shape=(rows, cols))


def dense(M):
    return scipy_csr(M).toarray()


# ---- exact sums -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
def test_fit_norm_squares_are_the_exact_sums(dtype):
    rng = np.random.default_rng(1)
    n, na = 300, 23
    agg = rng.integers(-1, na, size=n).astype(np.int32)
    agg[agg == 7] = 8                                           # id 7 is unused
    B = rng.integers(-9, 10, size=n).astype(dtype)              # squares and their sums are small integers: every add is exact
    Tp, Tj, Tx, Rr = R.fit(agg, B, na)
    for a in range(na):
        want = sum(Fraction(int(b)) ** 2 for b in B[agg == a])
        assert Rr[a] == dtype(np.sqrt(dtype(float(want)))), a
    assert Rr[7] == 0 and Tp[-1] == len(Tj) == int((agg >= 0).sum())
    assert np.array_equal(np.diff(Tp), (agg >= 0).astype(np.int32)) and np.array_equal(Tj, agg[agg >= 0])
    with np.errstate(all="ignore"):
        same_bits(Tx, (B[agg >= 0] / Rr[Tj]).astype(dtype), "T")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("op", ["add", "subtract"])
def test_merged_entries_are_the_exact_sums(dtype, op):
    rng = np.random.default_rng(2)
    m, n = 40, 31
    A, B = R.random_sorted_csr(rng, m, n, 0.2, dtype), R.random_sorted_csr(rng, m, n, 0.2, dtype)
    Cp, Cj, Cx = R.elementwise(m, n, *A, *B, op)
    want = R.exact_elementwise(m, *A, *B, op)
    got = {(int(i), int(j)): Fraction(float(v)) for i, j, v in zip(R.csr_rows(Cp), Cj, Cx)}
    assert got == want and len(Cj) < len(A[1]) + len(B[1])      # duplicates merged, cancellations dropped
    rows = R.csr_rows(Cp)
    assert np.all((rows[1:] != rows[:-1]) | (Cj[1:] > Cj[:-1]))


# ---- structure against scipy ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("theta", [0.0, 0.25, 1.0])
def test_strength_pattern_is_the_scipy_filter(dtype, theta, golden_irregular):
    p = "f64" if dtype == np.float64 else "f32"
    n = int(golden_irregular["cols"])                           # the square part of the fixture
    full = sp.csr_matrix((golden_irregular[p + "_Ax"], golden_irregular[p + "_Aj"], golden_irregular[p + "_Ap"]),
                         shape=(int(golden_irregular["rows"]), n))[:n, :].tocsr()
    Ap, Aj, Ax = full.indptr.astype(np.int32), full.indices.astype(np.int32), full.data.astype(dtype)
    Sp, Sj, Sx = R.strength(n, Ap, Aj, Ax, theta)
    mine = R.strength(n, Ap, Aj, Ax, theta, return_mask=True)
    assert np.array_equal(Sj, Aj[mine]) and np.array_equal(np.diff(Sp), np.add.reduceat(np.r_[mine, False].astype(np.int64), Ap[:-1]) * (np.diff(Ap) > 0))
    d = np.abs(full.diagonal())                                 # (scipy sums a repeated diagonal entry, as the contract does)
    rows = R.csr_rows(Ap)
    # the same predicate in double on the double diagonal: the margin decides which entries may legitimately differ
    lim = theta * np.sqrt(d[rows] * d[Aj])
    mag = np.abs(Ax.astype(np.float64))
    sure_in, sure_out = mag > lim * (1 + 1e-5), mag < lim * (1 - 1e-5)
    assert mine[sure_in].all() and not mine[sure_out].any()
    if theta == 0:
        assert np.array_equal(Sp, Ap) and np.array_equal(Sj, Aj)
        same_bits(Sx, Ax, "theta 0 keeps everything")


@pytest.mark.parametrize("dtype", DT)
def test_add_and_subtract_against_scipy(dtype):
    rng = np.random.default_rng(3)
    m, n = 57, 49
    A, B = R.random_sorted_csr(rng, m, n, 0.15, dtype, duplicates=False), R.random_sorted_csr(rng, m, n, 0.15, dtype, duplicates=False)
    for op, want in (("add", scipy_csr((m, n, *A)) + scipy_csr((m, n, *B))), ("subtract", scipy_csr((m, n, *A)) - scipy_csr((m, n, *B)))):
        C = (m, n, *R.elementwise(m, n, *A, *B, op))
        want.eliminate_zeros()
        assert np.array_equal(dense(C), want.toarray()) and len(C[3]) == want.nnz


def hierarchy(dtype, nx, ny, min_level_size, rhos=None):
    """[(A, P, aggregates)] + the coarsest A, built by the references alone; rho per level from `rhos` or numpy."""
    N, Ap, Aj, Ax = SR.poisson5pt(nx, ny, dtype)
    A, B, out = (N, N, Ap, Aj, Ax), np.ones(N, dtype), []
    while A[0] > min_level_size:
        n = A[0]
        S = R.strength(n, *A[2:], 0.0)
        agg, _ = R.standard_aggregate(n, S[0], S[1])
        na = int(agg.max()) + 1
        Tp, Tj, Tx, Rr = R.fit(agg, B, na)
        if rhos is None:
            M = scipy_csr(A)
            rho = float(np.max(np.abs(np.linalg.eigvals((sp.diags(1.0 / M.diagonal()) @ M).toarray())))) if n <= 2000 else 2.0
        else:
            rho = rhos[len(out)]
        P = R.smooth_prolongator(A, (n, na, Tp, Tj, Tx), rho)
        out.append((A, P, agg))
        A, B = R.galerkin((na, n, *SR.transpose(*P)), A, P), Rr
    return out, A


def test_level_sizes_of_poisson_100x100():
    # rho(D^-1 A) of the two fine levels as scipy.sparse.linalg.eigs gives them (largest magnitude); the sizes and entry counts
    # depend on the patterns alone, so any rho in (0, 2] gives the same figures unless an entry cancels exactly
    levels, coarse = hierarchy(np.float64, 100, 100, 500, rhos=[1.9995162822919836, 1.4076716791442256])
    assert [l[0][0] for l in levels] + [coarse[0]] == [10000, 1700, 192]
    assert [len(l[0][3]) for l in levels] + [len(coarse[3])] == [49600, 14928, 1692]


@pytest.mark.parametrize("dtype", DT)
def test_galerkin_product_against_scipy_within_rounding(dtype):
    levels, coarse = hierarchy(dtype, 24, 20, 50)
    assert len(levels) >= 2
    eps = np.finfo(dtype).eps
    for (A, P, agg), Ac in zip(levels, [l[0] for l in levels[1:]] + [coarse]):
        Ps, As = scipy_csr(P), scipy_csr(A)
        want = (Ps.T @ As @ Ps).toarray()
        # |error| <= (chain length + 2 roundings) eps * sum of |products| entrywise
        bound = (abs(Ps).T @ abs(As) @ abs(Ps)).toarray() * eps * (2 * 5 * 9 + 4)
        assert np.all(np.abs(dense(Ac) - want) <= bound + np.finfo(dtype).tiny)
        assert Ac[0] == int(agg.max()) + 1 and R.is_sorted(Ac[1], Ac[2], Ac[3])


@pytest.mark.parametrize("dtype", DT)
def test_lu_against_numpy(dtype):
    rng = np.random.default_rng(4)
    M = rng.standard_normal((9, 9)).astype(dtype)
    M[0, 0] = 0                                                 # the first pivot must move
    b = rng.standard_normal(9).astype(dtype)
    LU, piv = R.lu_factor(M)
    assert piv[0] != 0
    x = R.lu_solve(LU, piv, b)
    want = np.linalg.solve(M.astype(np.float64), b.astype(np.float64))
    assert np.max(np.abs(x - want)) <= 200 * np.finfo(dtype).eps * np.linalg.cond(M.astype(np.float64)) * np.max(np.abs(want))
    with pytest.raises(ZeroDivisionError):
        R.lu_factor(np.zeros((3, 3), dtype))


def test_standard_aggregate_on_a_path_and_an_isolated_node():
    # 0 - 1 - 2 - 3 - 4, node 5 alone (its row holds only its diagonal)
    rows = [[(0, 1.0), (1, 1.0)], [(0, 1.0), (1, 1.0), (2, 1.0)], [(1, 1.0), (2, 1.0), (3, 1.0)], [(2, 1.0), (3, 1.0), (4, 1.0)],
            [(3, 1.0), (4, 1.0)], [(5, 1.0)]]
    Ap, Aj, _ = SR.csr(rows, np.float64)
    agg, roots = R.standard_aggregate(6, Ap, Aj)
    assert agg.tolist() == [0, 0, 1, 1, 1, -1] and roots.tolist() == [0, 3]   # pass 1: {0, 1} around 0, then {2, 3, 4} around 3; 5 is isolated


# ---- mutants ----------------------------------------------------------------------------------------------------------------
def differs(a, b):
    return a.shape != b.shape or bool(bits_differ(a, b).any())


@pytest.mark.parametrize("dtype", DT)
def test_mutant_sum_from_zero_and_rows_descending(dtype):
    """A square is never -0.0, so +0 + B0^2 has the bits of B0^2 for every B0 (NaN included): starting the chain at +0 cannot be
    told from starting it at the first square, and this test pins that down instead of pretending to catch it.  What the
    binade deck does catch is the ORDER of the chain."""
    agg, B = R.binade_deck(dtype)
    good = R.fit(agg, B, 1)
    assert not differs(good[3], R.fit(agg, B, 1, mutant="sum_from_zero")[3])
    for b0 in (0.0, -0.0, np.nan, np.inf, 1e-30):
        one = np.array([b0], dtype)
        assert not differs(R.fit(agg[:1], one, 1)[3], R.fit(agg[:1], one, 1, mutant="sum_from_zero")[3])
    assert differs(good[3], R.fit(agg, B, 1, mutant="rows_descending")[3])


@pytest.mark.parametrize("dtype", DT)
def test_mutant_b_before_a(dtype):
    big = dtype(2.0) ** (53 if dtype == np.float64 else 24)
    A = SR.csr([[(0, big)]], dtype)
    B = SR.csr([[(0, 1.0), (0, 1.0)]], dtype)                  # (big + 1) + 1 = big; (1 + 1) + big = big + 2
    good = R.elementwise(1, 1, *A, *B, "add")
    bad = R.elementwise(1, 1, *A, *B, "add", mutant="b_before_a")
    assert good[2][0] == big and differs(good[2], bad[2])


@pytest.mark.parametrize("dtype", DT)
def test_mutant_minus_instead_of_negate_on_a_minus_zero_case(dtype):
    T = np.dtype(dtype).type
    good = R.chain_value([], [T(0.0)], "subtract", T)
    bad = R.chain_value([], [T(0.0)], "subtract", T, mutant="minus_instead_of_negate")
    assert good == 0 and np.signbit(good) and bad == 0 and not np.signbit(bad)
    # ... and the zero test hides it: neither variant stores an entry
    A, B = SR.csr([[]], dtype), SR.csr([[(0, 0.0)]], dtype)
    for mutant in (None, "minus_instead_of_negate"):
        assert len(R.elementwise(1, 1, *A, *B, "subtract", mutant=mutant)[1]) == 0


@pytest.mark.parametrize("dtype", DT)
def test_mutants_product_and_quotient_swapped(dtype):
    rng = np.random.default_rng(5)
    n = 200
    Ap = np.arange(n + 1, dtype=np.int32)
    Ax, d, b = (rng.standard_normal(n).astype(dtype) for _ in range(3))
    lam = 4.0 / 3.0 / 1.9
    assert differs(R.scale_rows(Ap, Ax, d, lam), R.scale_rows(Ap, Ax, d, lam, mutant="scale_product_first"))
    assert differs(R.presmooth(d, b, lam), R.presmooth(d, b, lam, mutant="presmooth_quotient_first"))


@pytest.mark.parametrize("dtype", DT)
def test_mutant_zeros_kept(dtype):
    A = SR.csr([[(0, 1.0), (1, 2.0)]], dtype)
    good = R.elementwise(1, 2, *A, *A, "subtract")
    bad = R.elementwise(1, 2, *A, *A, "subtract", mutant="zeros_kept")
    assert good[0].tolist() == [0, 0] and bad[0].tolist() == [0, 2]


def test_mutant_threshold_in_value_type():
    n, Ap, Aj, Ax, theta, keep = R.value_type_threshold_case()
    good = R.strength(n, Ap, Aj, Ax, theta)
    bad = R.strength(n, Ap, Aj, Ax, theta, mutant="threshold_in_value_type")
    assert not keep and len(good[1]) == 2 and len(bad[1]) == 3


@pytest.mark.parametrize("dtype", DT)
def test_threshold_deck_keeps_and_drops_by_one_ulp(dtype):
    for n, Ap, Aj, Ax, theta, keep in R.threshold_deck(dtype):
        Sp, Sj, Sx = R.strength(n, Ap, Aj, Ax, theta)
        assert ((0, 1) in set(zip(R.csr_rows(Sp).tolist(), Sj.tolist()))) == keep

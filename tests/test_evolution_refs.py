"""CPU tests (-m "not gpu") of tests/evolution_refs.py itself: the masked product against exact arithmetic, the measure against
scipy's sparse product sampled on the pattern, the structural facts of the 7 x 5 anisotropic grid, one deck per mutant, and
cusp::gallery::diffusion's coefficients against a direct evaluation of the reference's formulas."""
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import evolution_refs as E
from special_values import same_bits

DT = [np.float64, np.float32]
FINITE = ("diffusion 7x5 FD angle 0", "diffusion 7x5 FD angle pi/4", "diffusion 7x5 FE angle 0", "diffusion 7x5 FE angle pi/4", "1x1", "diagonal 65", "arrow 70",
          "random 40", "random 40, epsilon inf", "random 40, epsilon 1")


@pytest.fixture(scope="module")
def measured():
    """Every deck's restatement, computed once."""
    return {dt: {name: (d, E.evolution_strength(*d)) for name, d in E.decks(dt).items()} for dt in DT}


@pytest.mark.parametrize("dtype", DT)
def test_masked_product_within_the_chain_bound_of_exact_arithmetic(measured, dtype):
    """|computed - exact| <= n u sum|terms| for a chain of n products added from +0: every term passes through at most n roundings (its
    own product and the n - 1 additions that follow the first, which adds to +0 and is exact), each of relative size u."""
    u = E.unit_roundoff(dtype)
    for name in FINITE:
        (n, Ap, Aj, Ax, B, rho, eps), r = measured[dtype][name]
        v, w = r["v"], r["v"][r["tpos"]]
        for e, (exact, magnitude, terms) in enumerate(E.exact_masked_product(n, Ap, Aj, v, w)):
            err = abs(Fraction(float(r["data"][e])) - exact)
            assert err <= terms * u * magnitude, (name, e, float(err), terms)


@pytest.mark.parametrize("dtype", DT)
def test_measure_against_scipys_product_sampled_on_the_pattern(measured, dtype):
    """(Atilde Atilde) formed by scipy in double and read where A stores an entry.  Both sides are rounded sums of the same terms, so
    they agree within the sum of their chain bounds, n (u + 2^-53) sum|terms| (scipy adds in double, in an order of its own); and the
    measure continued from scipy's data keeps the same pattern."""
    u = float(E.unit_roundoff(dtype))
    for name in FINITE:
        (n, Ap, Aj, Ax, B, rho, eps), r = measured[dtype][name]
        At = sp.csr_matrix((r["v"].astype(np.float64), Aj, Ap), shape=(n, n))
        sq = (At @ At).tocsr()
        rows = E.csr_rows(Ap)
        sampled = np.asarray(sq[rows, Aj]).ravel()
        mag = np.asarray((abs(At) @ abs(At)).tocsr()[rows, Aj]).ravel()
        terms = np.array([t for _, _, t in E.exact_masked_product(n, Ap, Aj, r["v"], r["v"][r["tpos"]])])
        assert np.all(np.abs(r["data"].astype(np.float64) - sampled) <= terms * (u + 2.0 ** -53) * mag), name
        again = E.evolution_strength(n, Ap, Aj, Ax, B, rho, eps, data=sampled.astype(dtype))
        assert np.array_equal(again["S"][0], r["S"][0]) and np.array_equal(again["S"][1], r["S"][1]), name


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("method", ["FD", "FE"])
@pytest.mark.parametrize("eps", [1e-3, 1e-2])
def test_seven_by_five_keeps_the_strong_direction_and_nothing_else(dtype, method, eps):
    """7 x 5 grid, angle 0: the kept diagonals are {-7, 0, 7}, 91 entries of 151 (FD) or 247 (FE).
    float32 gives the same pattern as float64.  sqrt(eps_float) = 3.45e-4 lies above the 1e-4 constant, so in float32 step 14 would also
    LOWER a value in (1e-4, 3.45e-4) to 1e-4, which float64 (sqrt(eps) = 1.5e-8) never does; but on these grids no a[e] comes near that
    interval: the smallest non-zero a after step 13 is 0.178 (FD) and 0.359 (FE) in both types, so step 14 changes nothing here."""
    N, Ap, Aj, Ax = E.diffusion(7, 5, eps, 0.0, method, dtype)
    assert len(Aj) == (151 if method == "FD" else 247)
    Sp, Sj, Sx = E.evolution_strength(N, Ap, Aj, Ax, np.ones(N, dtype), 1.9)["S"]
    assert len(Sj) == 91 and set((Sj - E.csr_rows(Sp)).tolist()) == {-7, 0, 7}
    assert np.all(Sx[Sj == E.csr_rows(Sp)] == 2) and Sx.dtype == dtype


def _catches(mutant, dtype, names):
    for name in names:
        d = E.decks(dtype)[name]
        good, bad = E.evolution_strength(*d), E.evolution_strength(*d, mutant=mutant)
        if not (np.array_equal(good["S"][1], bad["S"][1]) and np.array_equal(good["S"][0], bad["S"][0])
                and np.array_equal(good["S"][2].view(np.uint8), bad["S"][2].view(np.uint8))
                and np.array_equal(good["data"].view(np.uint8), bad["data"].view(np.uint8))):
            return name
    return None


@pytest.mark.parametrize("mutant", E.MUTANTS)
def test_every_mutant_is_caught_by_a_deck(mutant):
    assert mutant in E.MUTANTS
    dtype = np.float32 if mutant == "rho_product_in_value_type" else np.float64
    caught = _catches(mutant, dtype, E.decks(dtype).keys())
    print(mutant, "caught by", caught)
    assert caught is not None, f"no deck tells {mutant} from the contract"


def test_filter_boundary_and_zero_minimum_cases_are_in_the_decks(measured):
    """The decks hold what the filter mutants need: an entry exactly at epsilon * small (epsilon = 1: the row's own minimum) and rows whose
    s has zeros beside non-zeros."""
    (n, Ap, Aj, Ax, B, rho, eps), r = measured[np.float64]["random 40, epsilon 1"]
    assert len(r["S"][1]) >= n                                               # the minimum itself is dropped (>=), the diagonal stays
    assert _catches("filter_greater", np.float64, ["random 40, epsilon 1"]) and _catches("min_with_zeros", np.float64, ["random 40", "diffusion 7x5 FD angle 0"])


@pytest.mark.parametrize("dtype", DT)
def test_transpose_positions_and_refusals(dtype):
    for name, (n, Ap, Aj, *_rest) in E.decks(dtype).items():
        tpos, ok = E.transpose_positions(n, Ap, Aj)
        assert ok, name
        rows = E.csr_rows(Ap)
        assert np.array_equal(rows[tpos], Aj) and np.array_equal(Aj[tpos], rows) and np.array_equal(tpos[tpos], np.arange(len(Aj))), name
    for name, (n, Ap, Aj) in E.nonconforming().items():
        assert not E.transpose_positions(n, Ap, Aj)[1], name


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("method", ["FD", "FE"])
def test_diffusion_coefficients_and_counts(dtype, method):
    T = dtype
    for eps, theta in ((1e-3, 0.0), (1e-5, np.pi / 4), (0.25, 0.3)):
        got = E.diffusion_coefficients(eps, theta, method, dtype)
        # the reference's formulas, evaluated directly: C, S, CC, SS, CS in T; the rest in double, rounded on assignment
        C, S = T(np.cos(theta)), T(np.sin(theta))
        CC, SS, CS = (np.float64(T(C * C)), np.float64(T(S * S)), np.float64(T(C * S)))
        if method == "FE":
            want = [T((-1.0 * eps - 1.0) * CC + (-1.0 * eps - 1.0) * SS + (3.0 * eps - 3.0) * CS), T((2.0 * eps - 4.0) * CC + (-4.0 * eps + 2.0) * SS),
                    T((-1.0 * eps - 1.0) * CC + (-1.0 * eps - 1.0) * SS + (-3.0 * eps + 3.0) * CS), T((-4.0 * eps + 2.0) * CC + (2.0 * eps - 4.0) * SS),
                    T((8.0 * eps + 8.0) * CC + (8.0 * eps + 8.0) * SS)]
            want = [T(np.float64(x) / 6.0) for x in want]
        else:
            a = T(0.5 * (eps - 1.0) * CS)
            want = [a, T(-(eps * SS + CC)), T(-a), T(-(eps * CC + SS)), T(2.0 * (eps + 1.0))]
        same_bits(np.array(got, dtype), np.array(want, dtype), f"{method} eps {eps} theta {theta}")
    a, b, c, d, e = E.diffusion_coefficients(1e-3, 0.0, "FD", dtype)
    assert a == 0 and c == 0 and b == -1 and e == T(2.0 * 1.001)
    for m, n in ((7, 5), (1, 1), (1, 4), (5, 1), (2, 2)):
        full = (3 * m - 2) * (3 * n - 2)                                      # nine-point: every pair of neighbouring cells, both ways, and the diagonal
        five = m * n + 2 * (m - 1) * n + 2 * m * (n - 1)
        N, Ap, Aj, Ax = E.diffusion(m, n, 1e-3, 0.0, "FD", dtype)
        assert N == m * n and len(Aj) == five and np.all(Ax != 0)
        N, Ap, Aj, Ax = E.diffusion(m, n, 1e-3, np.pi / 4, method, dtype)
        assert len(Aj) == full and np.all(Ax != 0) and E.transpose_positions(N, Ap, Aj)[1]

"""CPU checks of tests/rounding_refs.py: the exact row sums against rational arithmetic, honest summation orders inside the
rounding-error bound, and -- the reason the bound exists -- precision mistakes that the suite's older bar (1e-6 / 1e-5 of
sum |a x|) accepts on every row and the bound rejects on every row."""
from fractions import Fraction

import numpy as np
import pytest

import rounding_refs as rr

MATRICES = ("ladder", "giant", "ell_ladder")
DTYPES = (np.float64, np.float32)


def sample_rows(M, count=40):
    """`count` rows: the longest, the first empty one, the first of one entry, the last, and a seeded draw of the rest."""
    keep = [int(np.argmax(M.lengths)), int(np.argmax(M.lengths == 0)), int(np.argmax(M.lengths == 1)), M.rows - 1]
    for i in np.random.default_rng(5).permutation(M.rows):
        if len(keep) < count and int(i) not in keep:
            keep.append(int(i))
    return sorted(keep)


@pytest.mark.parametrize("name", MATRICES)
@pytest.mark.parametrize("profile", rr.PROFILES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_rows_equal_rational_sums(name, profile, dtype):
    M = rr.matrix(name, profile, dtype)
    for acc in (False, True):
        exact, B, n = rr.exact_of(M, acc)
        assert np.array_equal(n, M.lengths + (1 if acc else 0))
        for i in sample_rows(M):
            lo, hi = int(M.Ap[i]), int(M.Ap[i + 1])
            prods = [Fraction(float(a)) * Fraction(float(M.x[j])) for a, j in zip(M.Ax[lo:hi], M.Aj[lo:hi])]
            if acc:
                prods.append(Fraction(float(M.y0[i])))
            s, mag = sum(prods, Fraction(0)), sum((abs(p) for p in prods), Fraction(0))
            assert exact[i] == float(s), (name, profile, i)  # float(Fraction) rounds to nearest even: the same single rounding
            assert mag <= Fraction(float(B[i])) <= mag * (1 + Fraction(1, 2 ** 40)), (name, profile, i)


@pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="np.longdouble has fewer than 63 mantissa bits here")
@pytest.mark.parametrize("name", MATRICES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_rows_agree_with_longdouble(name, dtype):
    """A cross-check only (63 bits leave no headroom to be the reference): agreement to 2^-60 of B, on top of the one rounding to
    float64 that `exact` has had."""
    M = rr.matrix(name, "normal", dtype)
    exact, B, n = rr.exact_of(M, True)
    prod = M.Ax.astype(np.longdouble) * M.x[M.Aj].astype(np.longdouble)
    for i in range(M.rows):
        s = prod[int(M.Ap[i]):int(M.Ap[i + 1])].sum(dtype=np.longdouble) + np.longdouble(M.y0[i])
        assert abs(float(s - np.longdouble(exact[i]))) <= 2.0 ** -60 * B[i] + 2.0 ** -53 * abs(exact[i]), (name, i)


@pytest.mark.parametrize("name", MATRICES)
@pytest.mark.parametrize("profile", rr.PROFILES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_honest_orders_are_within_the_bound(orc, name, profile, dtype, capsys):
    M = rr.matrix(name, profile, dtype)
    worst = {}
    for acc in (False, True):
        exact, B, n = rr.exact_of(M, acc)
        got = {"storage": orc.spmv_csr(M.Ap, M.Aj, M.Ax, M.x, M.y0.copy() if acc else None)}
        for order, fn in rr.HONEST.items():
            got[order] = rr.apply_order(M, fn, acc)
        for order, y in got.items():
            bad = rr.within_rounding_bound(y, exact, B, n, dtype)
            assert not bad, f"{name} {profile} {np.dtype(dtype)} acc={acc} {order}: {rr.describe(bad)}"
            worst[order] = max(worst.get(order, 0.0), rr.worst_ratio(y, exact, B, n, dtype))
    with capsys.disabled():
        print(f"\n{name} {profile} {np.dtype(dtype)}: worst err / (gamma_(n+1) B): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def old_bar_accepts(y, exact, B, dtype):
    return np.abs(y.astype(np.float64) - exact) <= rr.TOL_TODAY[np.dtype(dtype)] * B


def rejected_rows(y, exact, B, n, dtype):
    out = np.zeros(len(y), bool)
    out[[b[0] for b in rr.within_rounding_bound(y, exact, B, n, dtype)]] = True
    return out


@pytest.mark.parametrize("name", ("giant", "ell_ladder"))
@pytest.mark.parametrize("acc", (False, True))
def test_f64_mutants_are_rejected_on_every_row_and_the_old_bar_accepts_the_float_ones(name, acc):
    """Standard-normal values, f64: every mutant is outside the bound on EVERY row with two or more products; the two that
    pass a value through float32 are inside 1e-6 * B on those same rows -- what the older bar could not see."""
    M = rr.matrix(name, "normal", np.float64)
    exact, B, n = rr.exact_of(M, acc)
    rows = M.lengths >= 2
    for mutant, fn in rr.MUTANTS.items():
        y = rr.apply_order(M, fn, acc)
        rej = rejected_rows(y, exact, B, n, np.float64)
        assert rej[rows].all(), f"{name} acc={acc} {mutant}: accepted on rows {np.nonzero(rows & ~rej)[0][:8]}"
        if "float32" in mutant:
            assert old_bar_accepts(y, exact, B, np.float64)[rows].all(), f"{name} {mutant}: even the old bar rejects it"


@pytest.mark.parametrize("name", ("giant", "ell_ladder"))
def test_f64_mutants_on_the_wide_profile(name):
    """Magnitudes over 2^-20 .. 2^20: the float32 mutants are still rejected on every row (the row's largest term is rounded to
    24 bits); a dropped or doubled term is an error of exactly that term, so it is rejected wherever the term exceeds twice the
    bar (the mutant's own re-ordering may cancel up to one bar of it) -- a term of 2^-60 of its row is below ANY rounding bar."""
    M = rr.matrix(name, "wide", np.float64)
    exact, B, n = rr.exact_of(M, False)
    rows = M.lengths >= 2
    lim = rr.bar(n, np.float64) * B
    first = np.array([abs(rr.row_terms(M, i)[0]) if M.lengths[i] else 0.0 for i in range(M.rows)])
    last = np.array([abs(rr.row_terms(M, i)[-1]) if M.lengths[i] else 0.0 for i in range(M.rows)])
    for mutant, fn in rr.MUTANTS.items():
        rej = rejected_rows(rr.apply_order(M, fn, False), exact, B, n, np.float64)
        must = rows if "float32" in mutant else rows & ((last if "last" in mutant else first) > 2 * lim)
        assert must.sum() >= 0.8 * rows.sum()  # (most rows: the test is not vacuous)
        assert rej[must].all(), f"{name} wide {mutant}: accepted on rows {np.nonzero(must & ~rej)[0][:8]}"


@pytest.mark.parametrize("name", ("giant", "ell_ladder"))
def test_f32_what_is_caught_and_what_is_not(name, capsys):
    """f32, standard-normal values.  A dropped or doubled term is an error of exactly that term (give or take the re-ordering's own
    rounding, which stays inside one bar as every honest order's does), so it is rejected on every row where the term exceeds twice the bar: asserted, and that is more than
    95 % of the rows with two or more products.  NOT caught: a term that happens to be smaller than its row's bar -- the product
    of two standard-normal numbers is below 1e-3 about once in a hundred draws, and beyond about 160 terms the bar stays at
    1e-5 * B, which grows with the row (about 0.6 for the 100 000-entry row).  The rows that slip through are printed.  A lane sum
    carried in bfloat16 is rejected on every row of two or more products, the longest included (4e-4 of B there).  (The f64
    instantiation of the same mistakes is caught on every row: see above.)"""
    M = rr.matrix(name, "normal", np.float32)
    exact, B, n = rr.exact_of(M, False)
    rows = M.lengths >= 2
    lim = rr.bar(n, np.float32) * B
    first = np.array([abs(float(rr.row_terms(M, i)[0])) if M.lengths[i] else 0.0 for i in range(M.rows)])
    last = np.array([abs(float(rr.row_terms(M, i)[-1])) if M.lengths[i] else 0.0 for i in range(M.rows)])
    for mutant, term in (("last term dropped", last), ("first term twice", first)):
        rej = rejected_rows(rr.apply_order(M, rr.MUTANTS[mutant], False), exact, B, n, np.float32)
        must = rows & (term > 2 * lim)
        assert rej[must].all(), f"{name} f32 {mutant}: accepted on rows {np.nonzero(must & ~rej)[0][:8]}"
        assert must.sum() >= 0.95 * rows.sum()
        with capsys.disabled():
            print(f"\n{name} f32 {mutant}: rejected on {int(rej[rows].sum())} of {int(rows.sum())} rows; accepted at lengths "
                  f"{sorted(set(M.lengths[rows & ~rej].tolist()))}")
    y = rr.apply_order(M, lambda t, y0: rr.bfloat16_carry_sum(t, rr.MUTANT_LANES, y0), False)
    rej = rejected_rows(y, exact, B, n, np.float32)
    assert rej[rows].all(), f"{name} f32 bfloat16 carry: accepted on rows {np.nonzero(rows & ~rej)[0][:8]}"

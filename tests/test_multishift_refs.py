"""CPU tests of tests/multishift_refs.py, the numpy restatements the multi-shift kernels and solvers are compared with elsewhere:
the coefficient formulas against fractions.Fraction, the vector kernels against exact integer arithmetic, both solver loops against
numpy.linalg.solve(A + sigma I, b) for every shift, and six deliberate mistakes (multishift_refs.MUTANTS), each of which must be caught
by at least one of those checks.

Bounds.  Coefficients: the inputs are exactly representable and chosen so that the two terms of KERNEL_ZB's denominator have the same
sign, so the relative error of a formula of k operations is about k u; the longest chain (alpha_s through zeta_1 and beta_s) has 14
operations, the bar is 16 u with u = 2^-24 / 2^-53.  Vector kernels: small integers, every operation exact, the bar is
equality.  Solvers: the reference's own criterion, ||b - (A + sigma I) x|| < 100 x the monitor's relative tolerance x ||b||
(testing/multi_mass.cu), and the iteration counts the loops give in IEEE arithmetic."""
from fractions import Fraction

import numpy as np
import pytest

import multishift_refs as R

TYPES = {"f32": np.float32, "f64": np.float64}
U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
SIGMA = (0.1, 0.5, 1.0, 5.0)


def F(v):
    return Fraction(float(v))


def exact_zb(beta_m1, beta_0, alpha_0, z0, zm1, sigma):
    z1 = z0 * zm1 * beta_m1 / (beta_0 * alpha_0 * (zm1 - z0) + beta_m1 * zm1 * (1 - beta_0 * sigma))
    return z1, beta_0 * z1 / z0


def close(got, want, T, k=16):
    return abs(Fraction(float(got)) - want) <= k * Fraction(U[T]) * abs(want)


# ---- the checks; each returns True when the restatement (or its mutant) passes ---------------------------------------------
def check_cg_m_coefficients(T, mutant=None):
    """Two calls in sequence (the second sees the rotated zeta and the stored state) and one call that trips the clamp."""
    sigma = np.array([0.25, 0.5, 2.0], T)
    state, zm1, z0 = np.array([1, 0], T), np.ones(3, T), np.ones(3, T)
    e_state, e_zm1, e_z0 = [Fraction(1), Fraction(0)], [Fraction(1)] * 3, [Fraction(1)] * 3
    ok = True
    # first call: alpha_old = 0 removes the first term of the denominator.  Second call: beta_m1, beta_0 < 0 < alpha_old and zeta has
    # decreased, so both terms are negative; zm1 - z0 is a difference of a rounded value, but its term is under a tenth of the other one
    for rsq_old, pAp, rsq_new in ((8.0, 16.0, 2.0), (2.0, 8.0, 0.5)):
        state, zm1, z0, beta_s, alpha_s = R.cg_m_coefficients(T, rsq_old, pAp, rsq_new, state, sigma, zm1, z0, mutant)
        beta_0, alpha_0 = -Fraction(rsq_old) / Fraction(pAp), Fraction(rsq_new) / Fraction(rsq_old)
        for s in range(3):
            z1, b0 = exact_zb(e_state[0], beta_0, e_state[1], e_z0[s], e_zm1[s], F(sigma[s]))
            a = alpha_0 / beta_0 * z1 * b0 / e_z0[s]
            ok &= close(beta_s[s], b0, T) and close(alpha_s[s], a, T) and close(z0[s], z1, T) and close(zm1[s], e_z0[s], T)
            e_zm1[s], e_z0[s] = e_z0[s], z1
        e_state = [beta_0, alpha_0]
        ok &= F(state[0]) == beta_0 and F(state[1]) == alpha_0
    # the clamp: zeta_0 = 2^-110, zeta_m1 = 1, sigma = 0, state (1, 0), beta_0 = -1 -> zeta_1 = 2^-110 < 1e-30 becomes 1e-18; beta_s = -1 keeps
    # the unclamped value
    tiny = T(2.0 ** -110)
    st, m1, z, beta_s, _ = R.cg_m_coefficients(T, 1.0, 1.0, 1.0, np.array([1, 0], T), np.zeros(1, T), np.ones(1, T), np.array([tiny], T), mutant)
    ok &= z[0] == T(1e-18) and m1[0] == tiny and beta_s[0] == T(-1)
    return bool(ok)


def check_bicgstab_m_coefficients(T, mutant=None):
    sigma = np.array([0.25, 0.5, 2.0], T)
    zm1, z0, rho0 = np.array([1, 1, 1], T), np.array([0.5, 0.5, 0.25], T), np.array([1, 0.5, 2], T)
    beta_m1, beta_0, alpha_old, alpha_new, chi_0 = -0.5, -0.25, 0.5, 0.125, 0.75
    z1, beta_s, chi_s, rho1, alpha_s = R.bicgstab_m_coefficients(T, beta_m1, beta_0, alpha_old, alpha_new, chi_0, sigma, zm1, z0, rho0, mutant)
    ok = True
    for s in range(3):
        e_z1, e_b0 = exact_zb(Fraction(beta_m1), Fraction(beta_0), Fraction(alpha_old), F(z0[s]), F(zm1[s]), F(sigma[s]))
        den = 1 + Fraction(chi_0) * F(sigma[s])
        ok &= close(z1[s], e_z1, T) and close(beta_s[s], e_b0, T) and close(chi_s[s], Fraction(chi_0) / den, T) and close(rho1[s], F(rho0[s]) / den, T)
        ok &= close(alpha_s[s], Fraction(alpha_new) / Fraction(beta_0) * e_z1 * e_b0 / F(z0[s]), T)
    tiny = T(2.0 ** -110)
    z, b, *_ = R.bicgstab_m_coefficients(T, 1, -1, 0, 0, 1, np.zeros(1, T), np.ones(1, T), np.array([tiny], T), np.ones(1, T), mutant)
    return bool(ok and z[0] == T(1e-18) and b[0] == T(-1))


def check_update_xp(T, mutant=None):
    """Small integers: exact in T.  ld = n + 3 leaves gaps that must stay as they were."""
    n, ns, ld = 7, 3, 10
    rng = np.random.default_rng(7)
    r, p0 = rng.integers(-4, 5, n).astype(T), rng.integers(-4, 5, n).astype(T)
    x, ps = rng.integers(-4, 5, (ns - 1) * ld + n).astype(T), rng.integers(-4, 5, (ns - 1) * ld + n).astype(T)
    beta_s, alpha_s, zeta = np.array([2, -1, 3], T), np.array([1, 2, -2], T), np.array([3, 1, 2], T)
    state = np.array([5, 2], T)
    gp0, gx, gps = R.cg_m_update_xp(T, n, ns, ld, state, beta_s, alpha_s, zeta, r, p0, x, ps, mutant)
    wx, wps = x.astype(np.int64), ps.astype(np.int64)
    for s in range(ns):
        sl = slice(s * ld, s * ld + n)
        old = ps[sl].astype(np.int64)
        wx[sl] = x[sl].astype(np.int64) - int(beta_s[s]) * old
        wps[sl] = int(zeta[s]) * r.astype(np.int64) + int(alpha_s[s]) * old
    return bool(np.array_equal(gx, wx) and np.array_equal(gps, wps) and np.array_equal(gp0, r.astype(np.int64) + 2 * p0.astype(np.int64)))


def check_update_xs(T, mutant=None):
    """Integers with beta_s = +-1 and chi_s rho_0 integral: every operation of KERNEL_XS is exact."""
    n, ns, ld = 6, 2, 8
    rng = np.random.default_rng(11)
    r0, r1, w1 = (rng.integers(-3, 4, n).astype(T) for _ in range(3))
    x, ss = rng.integers(-3, 4, ld + n).astype(T), rng.integers(-3, 4, ld + n).astype(T)
    beta_s, chi_s, rho0, zeta0 = np.array([1, -1], T), np.array([2, 1], T), np.array([1, 3], T), np.array([2, -1], T)
    alpha_s, rho1, zeta1, zm1 = np.array([3, -2], T), np.array([2, 5], T), np.array([-1, 2], T), np.array([7, 7], T)
    gx, gss, gzm1, gz0, grho0 = R.bicgstab_m_update_xs(T, n, ns, ld, beta_s, chi_s, rho0, zm1, zeta0, alpha_s, rho1, zeta1, r0, r1, w1, x, ss, mutant)
    wx, wss = x.astype(np.int64), ss.astype(np.int64)
    i = lambda a: a.astype(np.int64)
    for s in range(ns):
        sl = slice(s * ld, s * ld + n)
        b, c, q0, z0, a, q1, z1 = (int(v[s]) for v in (beta_s, chi_s, rho0, zeta0, alpha_s, rho1, zeta1))
        wx[sl] = i(x[sl]) - b * i(ss[sl]) + c * q0 * z1 * i(w1)
        wss[sl] = z1 * q1 * i(r1) + a * (i(ss[sl]) - (c * q0 // b) * (z1 * i(w1) - z0 * i(r0)))
    return bool(np.array_equal(gx, wx) and np.array_equal(gss, wss) and np.array_equal(gzm1, zeta0) and np.array_equal(gz0, zeta1) and np.array_equal(grho0, rho1))


def solve_passes(solver, T, nx, ny, tol, mutant=None):
    A = R.poisson5pt(nx, ny, T)
    b, sigma = np.ones(A[0], T), np.array(SIGMA, T)
    x, mon = solver(A, b, sigma, 100, tol, mutant)
    if not mon.converged() or not np.isfinite(x).all():
        return False, mon, x
    D = R.dense(A)
    for k, s in enumerate(sigma):
        want = np.linalg.solve(D + float(s) * np.eye(A[0]), b.astype(np.float64))
        if not np.linalg.norm(x[k] - want) <= 100 * tol * np.linalg.norm(want):   # the residual bar carries over: every eigenvalue of A + sigma I is > 0.1 ... < 13
            return False, mon, x
    return max(R.relative_residuals(A, x, b, sigma)) < 100 * tol, mon, x


def all_checks(T, mutant=None):
    tol = 1e-6 if T is np.float32 else 1e-10
    return {
        "cg_m_coefficients": check_cg_m_coefficients(T, mutant),
        "bicgstab_m_coefficients": check_bicgstab_m_coefficients(T, mutant),
        "update_xp": check_update_xp(T, mutant),
        "update_xs": check_update_xs(T, mutant),
        "cg_m": solve_passes(R.cg_m, T, 7, 5, tol, mutant)[0],
        "bicgstab_m": solve_passes(R.bicgstab_m, T, 7, 5, tol, mutant)[0],
    }


# ---- the tests ------------------------------------------------------------------------------------------------------
def test_the_dot_is_the_sequential_loop():
    rng = np.random.default_rng(3)
    for T in TYPES.values():
        for n in (0, 1, 2, 35, 100, 1023):
            x, y = rng.standard_normal(n).astype(T), rng.standard_normal(n).astype(T)
            got = R.dot(x, y)
            assert got.dtype == T and got == R.dot_loop(x, y)
    x = np.array([2.0 ** 24, 1, 1, 1, 1], np.float32)   # left to right every 1 is lost; a pairwise sum would keep some
    assert R.dot(x, np.ones(5, np.float32)) == np.float32(2.0 ** 24)


def test_the_multiply_is_the_csr_loop():
    for T in TYPES.values():
        A = R.poisson5pt(7, 5, T)
        x = np.random.default_rng(5).standard_normal(35).astype(T)
        y = R.spmv(A, x)
        assert y.dtype == T
        for i in range(35):
            acc = T(0)
            for jj in range(A[1][i], A[1][i + 1]):
                acc = T(acc + T(A[3][jj] * x[A[2][jj]]))
            assert acc == y[i]
        assert np.array_equal(R.dense(A), R.dense(A).T) and R.dense(A)[0, 0] == 4 and R.dense(A)[0, 1] == -1 and R.dense(A)[0, 7] == -1


@pytest.mark.parametrize("tname", list(TYPES))
def test_kernel_restatements_are_exact(tname):
    assert all(all_checks(TYPES[tname]).values())


@pytest.mark.parametrize("tname", list(TYPES))
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_is_caught(tname, mutant):
    """Each mistake fails a kernel-level check; the ones that change a converged answer also fail the solve."""
    got = all_checks(TYPES[tname], mutant)
    caught = [k for k, v in got.items() if not v]
    assert caught, f"{mutant} passes every check"
    expected = {"zb_new_alpha": {"cg_m_coefficients", "bicgstab_m_coefficients", "cg_m", "bicgstab_m"},
                "no_clamp": {"cg_m_coefficients", "bicgstab_m_coefficients"},
                "rotation": {"cg_m_coefficients", "update_xs", "cg_m", "bicgstab_m"},
                "x_new_p": {"update_xp", "cg_m"},
                "xs_r0": {"update_xs", "bicgstab_m"},
                "xs_rho1": {"update_xs", "bicgstab_m"}}[mutant]
    assert expected <= set(caught), (mutant, caught)


@pytest.mark.parametrize("tname,nx,ny,tol,it_cg,it_bicg", [("f32", 10, 10, 1e-6, 14, 11), ("f32", 7, 5, 1e-6, 12, 8), ("f64", 10, 10, 1e-10, 15, 13),
                                                           ("f64", 7, 5, 1e-10, 12, 11), ("f64", 33, 31, 1e-10, 84, None)])
def test_solver_restatements_solve_every_shift(tname, nx, ny, tol, it_cg, it_bicg):
    T = TYPES[tname]
    ok, mon, _ = solve_passes(R.cg_m, T, nx, ny, tol)
    assert ok and mon.iteration_count == it_cg
    ok, mon, _ = solve_passes(R.bicgstab_m, T, nx, ny, tol)
    assert ok and (it_bicg is None or mon.iteration_count == it_bicg)


def test_bicgstab_m_in_float_loses_a_long_converged_shift():
    """The reference's arithmetic, kept: on Poisson 33 x 31 in float the zeta of sigma = 5 underflows, the clamp sets 1e-18 and the next
    zeta_0 zeta_m1 / (...) is 0 / 0 -- that shift's x is NaN when the loop stops after 47 iterations; the other shifts are solved.
    cg_m keeps all four (its zeta stays normal for the 65 iterations it needs)."""
    T = np.float32
    A = R.poisson5pt(33, 31, T)
    b, sigma = np.ones(A[0], T), np.array(SIGMA, T)
    x, mon = R.bicgstab_m(A, b, sigma, 100, 1e-6)
    assert mon.converged() and mon.iteration_count == 47
    assert np.isnan(x[3]).all() and np.isfinite(x[:3]).all()
    assert max(R.relative_residuals(A, x[:3], b, sigma[:3])) < 1e-4
    x, mon = R.cg_m(A, b, sigma, 100, 1e-6)
    assert mon.converged() and np.isfinite(x).all() and max(R.relative_residuals(A, x, b, sigma)) < 1e-4

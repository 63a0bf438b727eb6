"""CPU tests of the references in lobpcg_refs.py: a wrong reference must not pass a wrong kernel.  The kernels' restatements against exact
rational arithmetic within k * u * sum|terms| (as test_blas_extra_refs.py does), four mutants that must be caught, the restated small solver
against numpy.linalg.eigh of the reduced problem, and the restated loop on the solver cases."""
from fractions import Fraction

import numpy as np
import pytest

import lobpcg_refs as R

TYPES = [np.float32, np.float64]


def inputs(kernel, T, n, seed):
    rng = np.random.default_rng(seed)
    return {name: rng.standard_normal(n).astype(T) for name in kernel.vecs}


def F(x):
    return Fraction(float(x))


def worst_ratio(kernel, T, got, want):
    """The largest |got - exact| / (k u sum|terms|) over every output element."""
    u = Fraction(R.U[T])
    worst = Fraction(0)
    for out in kernel.outputs:
        value, terms = want[out]
        for i in range(len(value)):
            worst = max(worst, abs(F(got[out][i]) - value[i]) / (kernel.k[out] * u * terms[i]))
    return worst


@pytest.mark.parametrize("T", TYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["inexact", "exact"])
@pytest.mark.parametrize("name", sorted(R.KERNELS))
def test_restatement_is_within_the_bound_of_the_exact_formula(name, kind, T):
    kernel = R.KERNELS[name]
    for n in range(1, 9):
        s, v = R.scalars_for(kernel, kind, T), inputs(kernel, T, n, 100 + n)
        got = kernel.restate(T, s, v)
        assert sorted(got) == sorted(kernel.outputs)
        for out in kernel.outputs:
            assert got[out].dtype == T and got[out].shape == (n,)
        want = kernel.formula(*R.rational(s, v))
        assert worst_ratio(kernel, T, got, want) <= 1, (name, n)
        # the higher-precision evaluation the GPU tests may compare with: the same k roundings, in its own unit roundoff
        high = kernel.formula(*R.higher(T, s, v))
        uh = Fraction(float(np.finfo(R.HIGHER[T]).eps)) / 2
        for out in kernel.outputs:
            for i in range(n):
                assert abs(Fraction(*high[out][0][i].as_integer_ratio()) - want[out][0][i]) <= kernel.k[out] * uh * want[out][1][i], (name, out, n, i)


def test_by_value_scalars_are_values_of_T_and_the_roots_are_rational():
    for T in TYPES:
        for kind in ("inexact", "exact"):
            s = R.scalars_for(R.KERNELS["update"], kind, T)
            assert all(float(T(x)) == x for x in s.values())
    assert R._sqrt(Fraction(6.25)) == Fraction(5, 2) and R._sqrt(Fraction(4.0)) == 2
    for T in TYPES:  # 1 / 2.5 is rounded in T, 1 / 2 is not
        assert F(T(1) / T(2.5)) != Fraction(2, 5) and F(T(1) / T(2.0)) == Fraction(1, 2)


# ---- mutants: each check returns True when the restatement (or its mutant) passes -------------------------------------------------------------
def check_unfused(T, mutant=None):
    """Operands chosen so that an UNFUSED multiply-add cancels exactly: ax = -(neg x) rounded, p = -(cr w) rounded with cp = 1 (update) or first.
    A fused multiply-add leaves the product's rounding error instead of zero."""
    rng = np.random.default_rng(3)
    n = 64
    x = rng.standard_normal(n).astype(T)
    lam = 1.75 / 0.6
    neg = -T(np.float64(lam))
    r = R.KERNELS["residual"].restate(T, {"lambda": lam}, {"x": x, "ax": -(neg * x), "r": np.zeros(n, T)}, mutant)["r"]
    ok = not r.any()
    w, aw = rng.standard_normal(n).astype(T), rng.standard_normal(n).astype(T)
    cr = T(-1.1 / 0.3)
    v = {"w": w, "aw": aw, "p": -(cr * w), "ap": -(cr * aw), "x": np.zeros(n, T), "ax": np.zeros(n, T), "r": np.zeros(n, T)}
    s = {"cx": 0.5, "cr": float(cr), "cp": 1.0, "lambda_new": 3.0}
    for name in ("update", "update_first"):
        got = R.KERNELS[name].restate(T, s, v, mutant)
        ok &= not got["p"].any() and not got["ap"].any() and not got["x"].any() and not got["r"].any()
    return bool(ok)


def check_against_formula(name, T, mutant=None):
    kernel = R.KERNELS[name]
    s, v = R.scalars_for(kernel, "inexact", T), inputs(kernel, T, 8, 11)
    got = kernel.restate(T, s, v, mutant)
    return worst_ratio(kernel, T, got, kernel.formula(*R.rational(s, v))) <= 1


def check_gram_sums(T, mutant=None):
    """The eight sums are formed from the SCALED p and ap the kernel returned."""
    kernel = R.KERNELS["gram"]
    s, v = R.scalars_for(kernel, "inexact", T), inputs(kernel, T, 8, 13)
    got = kernel.restate(T, s, v)
    want = kernel.formula(*R.rational(s, v))
    x, w, p, ap = (R.rational({}, {"a": v[k]})[1]["a"] for k in ("x", "w", "p", "ap"))
    p, ap = want["p"][0], want["ap"][0]
    exact = {"xap": sum(x * ap), "wap": sum(w * ap), "pap": sum(p * ap), "xp": sum(x * p), "wp": sum(w * p)}
    named = R._s_gram(T, got, v, mutant)
    ok = tuple(named) == R.GRAM_SUMS
    for key, want_sum in exact.items():
        total, absolute = R.exact_sum(*named[key])
        # the returned p, ap carry up to k u relative error each: pap two factors, the others one
        ok &= abs(Fraction(total) - want_sum) <= (2 * kernel.k["p"] + 1) * Fraction(R.U[T]) * Fraction(absolute)
    return bool(ok)


@pytest.mark.parametrize("T", TYPES, ids=["f32", "f64"])
def test_the_restatements_pass_every_check(T):
    assert check_unfused(T)
    assert check_gram_sums(T)
    for name in ("update", "update_first", "update_no_r"):
        assert check_against_formula(name, T)


@pytest.mark.parametrize("T", TYPES, ids=["f32", "f64"])
def test_every_mutant_is_caught(T):
    assert set(R.MUTANTS) == {"fma", "unscaled_p_in_sums", "old_p_in_x", "first_ignored"}
    assert not check_unfused(T, "fma")
    assert not check_gram_sums(T, "unscaled_p_in_sums")
    assert not check_against_formula("update", T, "old_p_in_x")
    assert not check_against_formula("update_first", T, "old_p_in_x")
    assert not check_against_formula("update_first", T, "first_ignored")
    # a mutant changes only what it names
    assert check_against_formula("update", T, "first_ignored") and check_gram_sums(T, "old_p_in_x")


def test_sums_name_the_products_of_the_returned_vectors():
    for T in TYPES:
        for name in ("residual", "gram", "gram_first", "update", "update_no_r"):
            kernel = R.KERNELS[name]
            s, v = R.scalars_for(kernel, "inexact", T), inputs(kernel, T, 8, 3)
            got = kernel.restate(T, s, v)
            named = kernel.sums(T, got, v)
            assert len(named) == {"residual": 1, "gram": 8, "gram_first": 3, "update": 2, "update_no_r": 1}[name]
            for a, b in named.values():
                assert a.dtype == T and b.dtype == T
                total, absolute = R.exact_sum(a, b)
                exact = sum(F(x) * F(y) for x, y in zip(a, b))
                assert abs(Fraction(total) - exact) <= Fraction(2.0 ** -52) * Fraction(absolute)


# ---- the small solver ----------------------------------------------------------------------------------------------------------------------------
def small_pairs():
    """(group, n, A, B): random symmetric A; B = Q diag(d) Q^T with the smallest d from 1 down to 1e-6, and a unit-diagonal B as lobpcg builds
    it, with nearly parallel directions (gramB's smallest eigenvalue is 1 - c).  A group is one size and one smallest eigenvalue of B."""
    rng = np.random.default_rng(17)
    out = []
    for n in (2, 3):
        for smallest in (1.0, 1e-2, 1e-4, 1e-6):
            for _ in range(8):
                A = rng.standard_normal((n, n))
                A = A + A.T
                Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
                d = np.r_[smallest, rng.uniform(0.5, 2.0, n - 1)]
                B = (Q * d) @ Q.T
                out.append(((n, smallest), n, A, 0.5 * (B + B.T)))
        for c in (0.1, 0.9, 0.999999):
            for _ in range(8):
                A = rng.standard_normal((n, n))
                out.append(((n, "unit diagonal", c), n, A + A.T, np.full((n, n), c) + (1 - c) * np.eye(n)))
    return out


def eigh_of_the_reduced_problem(n, A, B):
    """LAPACK's route: Cholesky, the standard problem by numpy.linalg.eigh, back-transformation."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    L = np.linalg.cholesky(B)
    Li = np.linalg.inv(L)
    w, V = np.linalg.eigh(Li @ A @ Li.T)
    return True, w, Li.T @ V


def pair_errors(A, B, w, Z):
    """(largest ||A z - w B z||, largest |z^T B z - 1|) over the columns."""
    return (max(np.linalg.norm(A @ Z[:, j] - w[j] * (B @ Z[:, j])) for j in range(len(w))), max(abs(Z[:, j] @ B @ Z[:, j] - 1.0) for j in range(len(w))))


def test_small_solver_against_eigh_of_the_reduced_problem():
    """Per group of pairs (one size, one smallest eigenvalue of B) the restated solver's worst ||A z - w B z|| and worst |z^T B z - 1| stay within
    10 x numpy's own worst values on the same pairs (numpy.linalg.eigh of the reduced problem, back-transformed).
    Measured on these pairs (restated solver / numpy): with B's smallest eigenvalue 1 the residuals are 1.1e-15 / 1.7e-15 (2 x 2) and
    3.5e-15 / 3.1e-15 (3 x 3); at 1e-4, 9.6e-10 / 1.2e-9 and 1.8e-10 / 2.5e-10; at 1e-6, 2.2e-7 / 1.4e-7 and 6.7e-7 / 5.6e-7; the unit-diagonal B
    with c = 0.999999: 5.2e-7 / 2.4e-7 and 3.3e-7 / 3.7e-7.  |z^T B z - 1|: 4.4e-16 / 5.6e-16 at 1, 8.4e-11 / 1.3e-10 at 1e-6.  The largest
    ratio restated / numpy in any group is 2.6 (residual) and 1.5 (normalisation), against the factor 10."""
    groups = {}
    for key, n, A, B in small_pairs():
        ok, w, Z = R.sygv_small(n, A, B)
        assert ok and np.all(np.diff(w) >= 0), "eigenvalues ascending"
        _, w_ref, Z_ref = eigh_of_the_reduced_problem(n, A, B)
        g = groups.setdefault(key, [0.0, 0.0, 0.0, 0.0])
        for k, e in enumerate(pair_errors(A, B, w, Z) + pair_errors(A, B, w_ref, Z_ref)):
            g[k] = max(g[k], e)
    for key, (res, nrm, res_ref, nrm_ref) in groups.items():
        print(f"{key}: residual {res:.3g} (numpy {res_ref:.3g}), normalisation {nrm:.3g} (numpy {nrm_ref:.3g})")
        assert res <= 10 * res_ref and nrm <= 10 * nrm_ref, key


def test_small_solver_refuses_a_matrix_that_is_not_positive_definite():
    A2, A3 = [[1.0, 0.5], [0.5, 2.0]], [[1.0, 0.5, 0.1], [0.5, 2.0, 0.2], [0.1, 0.2, 3.0]]
    assert R.sygv_small(2, A2, [[1.0, 1.5], [1.5, 1.0]])[0] is False                                   # indefinite
    assert R.sygv_small(2, A2, [[1.0, 1.0], [1.0, 1.0]])[0] is False                                   # singular
    assert R.sygv_small(2, A2, [[0.0, 0.0], [0.0, 1.0]])[0] is False
    assert R.sygv_small(2, A2, [[1.0, float("nan")], [float("nan"), 1.0]])[0] is False
    assert R.sygv_small(3, A3, [[1.0, 0.1, 1.5], [0.1, 1.0, 0.2], [1.5, 0.2, 1.0]])[0] is False
    assert R.sygv_small(3, A3, [[1.0, 0.1, 0.2], [0.1, 1.0, 0.3], [0.2, 0.3, 1.0]])[0] is True
    # the Rayleigh-Ritz step: the 2 x 2 pair behind a 3 x 3 breakdown, nothing behind a 2 x 2 one
    g = [-0.5, 3.0, 0.125, 0.25, -0.75, 2.5, 1.5, -0.25]
    ok, used_p, lam, cx, cr, cp = R.ritz_step(np.float64, 1.5, g, True, False)
    assert ok and not used_p and cp == 0 and (lam, cx, cr) == R.ritz_step(np.float64, 1.5, g, False, False)[2:5]
    g[2] = -1.25
    assert R.ritz_step(np.float64, 1.5, g, True, False)[0] is False


def test_small_solver_orders_and_normalises_a_known_pair():
    ok, w, Z = R.sygv_small(2, [[2.0, 0.0], [0.0, 8.0]], [[1.0, 0.0], [0.0, 4.0]])   # 2 and 8 / 4
    assert ok and w.tolist() == [2.0, 2.0] and np.allclose(np.abs(Z), [[1.0, 0.0], [0.0, 0.5]])
    ok, w, Z = R.sygv_small(3, np.diag([9.0, 1.0, 4.0]), np.eye(3))
    assert ok and w.tolist() == [1.0, 4.0, 9.0] and np.array_equal(np.abs(Z), [[0, 0, 1], [1, 0, 0], [0, 1, 0]])


# ---- the loop -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "-".join(map(str, c)))
def test_restated_loop_meets_the_bars_of_the_solver_tests(case):
    """Converged, the eigenvalue within the tolerance, unit norm; the iteration count is what the C++ programs are compared with."""
    which, kind, nx, ny, tname, tol, precond = case
    lam, X, res = R.run_case(case)
    exact = R.exact_eigenvalue(kind, nx, ny, which == "largest")
    assert res.converged and 0 < res.iteration_count <= min(nx * ny, R.LIMIT) and res.retries == 0
    assert abs(float(lam) - exact) <= tol
    assert abs(np.linalg.norm(X.astype(np.float64)) - 1) <= 1e-5
    D = R.dense(R.case_matrix(kind, nx, ny, np.float64))
    assert np.linalg.norm(D @ X.astype(np.float64) - float(lam) * X.astype(np.float64)) <= 2 * tol


def test_restated_loop_with_lapack_route_takes_a_similar_path():
    """The two small solvers are both correct, so the loop's counts stay close: the margin of 1.5 the C++ tests use covers their difference."""
    for case in R.CASES[:2] + R.CASES[3:5]:
        mine = R.run_case(case)[2].iteration_count
        other = R.run_case(case, solver=eigh_of_the_reduced_problem)[2].iteration_count
        assert other <= 1.5 * mine and mine <= 1.5 * other, (case, mine, other)


def test_sequential_dot_is_the_host_loop():
    rng = np.random.default_rng(5)
    for T in TYPES:
        x, y = rng.standard_normal(37).astype(T), rng.standard_normal(37).astype(T)
        assert R.dot(x, y) == R.MS.dot_loop(x, y) and R.dot(x, y).dtype == T

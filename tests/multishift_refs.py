"""numpy restatements, in the value type T, of the multi-shift kernels of csrc/krylov_m.hip and of the two solvers
cusp::krylov::cg_m / bicgstab_m as the header layer runs them on host_memory (reference cusp/krylov/detail/cg_m.inl and
bicgstab_m.inl: KERNEL_ZB, KERNEL_A, KERNEL_XP, KERNEL_S, KERNEL_CHIRHO, KERNEL_XS and the two main loops).

Every expression is written in the reference's association with every operand of type T, so each operation rounds once to T
(numpy scalars and arrays of one dtype never widen).  Dots are sequential left-to-right sums in T, as the host cusp::blas::dotc forms
them (`dot`; `dot_loop` is the plain loop it is checked against).  The multiply is the host CSR loop: a row's entries in ascending
column order, added to T(0).

`mutant` names one deliberate mistake; tests/test_multishift_refs.py shows that each is caught:
  zb_new_alpha   KERNEL_ZB uses the new alpha_0        no_clamp         the clamp of a vanishing zeta dropped
  rotation       zeta_0 <- zeta_1 BEFORE zeta_m1 <- zeta_0              x_new_p          x_s updated with the new p_s
  xs_r0          r_0 for r_1 in KERNEL_XS              xs_rho1          rho_1 for rho_0 in KERNEL_XS's x term
"""
import numpy as np

MUTANTS = ("zb_new_alpha", "no_clamp", "rotation", "x_new_p", "xs_r0", "xs_rho1")


# ---- the matrix, the multiply, the dots, the monitor -----------------------------------------------------------------
def poisson5pt(nx, ny, dtype):
    """cusp::gallery::poisson5pt(A, nx, ny) as CSR: node x + nx * y, columns ascending, 4 on the diagonal and -1 off it."""
    r = np.arange(nx * ny)
    ix, iy = r % nx, r // nx
    cand = np.stack([r - nx, r - 1, r, r + 1, r + nx], 1)
    keep = np.stack([iy > 0, ix > 0, np.ones_like(r, bool), ix < nx - 1, iy < ny - 1], 1)
    vals = np.broadcast_to(np.array([-1, -1, 4, -1, -1], dtype), cand.shape)
    Ap = np.r_[0, np.cumsum(keep.sum(1))].astype(np.int32)
    return nx * ny, Ap, cand[keep].astype(np.int32), vals[keep].astype(dtype)


def dense(A, dtype=np.float64):
    N, Ap, Aj, Ax = A
    D = np.zeros((N, N), dtype)
    for i in range(N):
        for jj in range(Ap[i], Ap[i + 1]):
            D[i, Aj[jj]] += Ax[jj]
    return D


def spmv(A, x):
    """y[i] = (((0 + a x) + a x) + ...) over row i's entries in storage order, in x's dtype (the host CSR loop)."""
    N, Ap, Aj, Ax = A
    T = x.dtype.type
    lens = np.diff(Ap)
    y = np.zeros(N, x.dtype)
    for k in range(int(lens.max()) if N else 0):
        rows = np.nonzero(lens > k)[0]
        jj = Ap[rows] + k
        y[rows] = y[rows] + Ax[jj].astype(x.dtype) * x[Aj[jj]]
    return y.astype(T)


def dot(x, y):
    """The sequential left-to-right sum in T (a cumulative sum cannot be reordered)."""
    T = x.dtype.type
    if x.size == 0:
        return T(0)
    return np.cumsum(x * y, dtype=x.dtype)[-1]


def dot_loop(x, y):
    T = x.dtype.type
    s = T(0)
    for a, b in zip(x, y):
        s = T(s + T(a * b))
    return s


def nrm2(x):
    return np.sqrt(dot(x, x))


class Monitor:
    """cusp::monitor<T>(b, limit, relative_tolerance): tolerances and norms are T."""

    def __init__(self, b, iteration_limit, relative_tolerance):
        T = b.dtype.type
        self.b_norm = nrm2(b)
        self.tolerance = T(T(0) + T(relative_tolerance) * self.b_norm)
        self.iteration_limit, self.iteration_count = iteration_limit, 0
        self.r_norm = np.finfo(b.dtype).max

    def converged(self):
        return bool(self.r_norm <= self.tolerance)

    def finished(self, r):
        self.r_norm = nrm2(r)
        return self.converged() or self.iteration_count >= self.iteration_limit


# ---- the per-shift coefficient formulas ---------------------------------------------------------------------------------
def zb(T, beta_m1, beta_0, alpha_0, z0, zm1, sigma, mutant=None):
    """KERNEL_ZB: (zeta_1, beta_s) per shift; the clamp comes behind beta_s."""
    one = T(1)
    with np.errstate(all="ignore"):
        z1 = z0 * zm1 * beta_m1 / (beta_0 * alpha_0 * (zm1 - z0) + beta_m1 * zm1 * (one - beta_0 * sigma))
        b0 = beta_0 * z1 / z0
    if mutant != "no_clamp":
        z1 = np.where(np.abs(z1) < T(1e-30), T(1e-18), z1)
    return z1.astype(T), b0.astype(T)


def ka(T, beta_0, alpha_0, z0, z1, b0):
    """KERNEL_A."""
    with np.errstate(all="ignore"):
        return (alpha_0 / beta_0 * z1 * b0 / z0).astype(T)


def cg_m_coefficients(T, rsq_old, pAp, rsq_new, state, sigma, zeta_m1, zeta_0, mutant=None):
    """cmi_cg_m_coefficients_*: returns (state, zeta_m1, zeta_0, beta_s, alpha_s) after the call.  rsq_old, pAp, rsq_new are doubles."""
    beta_m1, alpha_old = T(state[0]), T(state[1])
    beta_0 = T(-T(np.float64(rsq_old) / np.float64(pAp)))
    alpha_0 = T(np.float64(rsq_new) / np.float64(rsq_old))
    z1, beta_s = zb(T, beta_m1, beta_0, alpha_0 if mutant == "zb_new_alpha" else alpha_old, zeta_0, zeta_m1, sigma, mutant)
    alpha_s = ka(T, beta_0, alpha_0, zeta_0, z1, beta_s)
    if mutant == "rotation":
        new_z0 = z1.copy()
        new_zm1 = new_z0.copy()
    else:
        new_zm1 = zeta_0.copy()
        new_z0 = z1.copy()
    return np.array([beta_0, alpha_0], T), new_zm1, new_z0, beta_s, alpha_s


def cg_m_update_xp(T, n, num_shifts, ld, state, beta_s, alpha_s, zeta_0, r, p0, x, ps, mutant=None):
    """cmi_cg_m_update_xp_*: returns (p0, x, ps); x and ps hold shift s at [s ld, s ld + n), the gaps are left alone."""
    x, ps = x.copy(), ps.copy()
    if p0 is not None:
        p0 = (r + T(state[1]) * p0).astype(T)
    for s in range(num_shifts):
        sl = slice(s * ld, s * ld + n)
        old = ps[sl].copy()
        new = (zeta_0[s] * r + alpha_s[s] * old).astype(T)
        x[sl] = x[sl] - beta_s[s] * (new if mutant == "x_new_p" else old)
        ps[sl] = new
    return p0, x, ps


def bicgstab_m_s(T, alpha_1, chi_0, r1, As, s0):
    """KERNEL_S."""
    return (r1 + T(alpha_1) * (s0 - T(chi_0) * As)).astype(T)


def bicgstab_m_coefficients(T, beta_m1, beta_0, alpha_old, alpha_new, chi_0, sigma, zeta_m1, zeta_0, rho_0, mutant=None):
    """cmi_bicgstab_m_coefficients_*: returns (zeta_1, beta_s, chi_s, rho_1, alpha_s); nothing rotates."""
    beta_m1, beta_0, alpha_old, alpha_new, chi_0 = T(beta_m1), T(beta_0), T(alpha_old), T(alpha_new), T(chi_0)
    z1, beta_s = zb(T, beta_m1, beta_0, alpha_new if mutant == "zb_new_alpha" else alpha_old, zeta_0, zeta_m1, sigma, mutant)
    with np.errstate(all="ignore"):
        den = T(1) + chi_0 * sigma
        chi_s = (chi_0 / den).astype(T)
        rho_1 = (rho_0 / den).astype(T)
    return z1, beta_s, chi_s, rho_1, ka(T, beta_0, alpha_new, zeta_0, z1, beta_s)


def bicgstab_m_update_xs(T, n, num_shifts, ld, beta_s, chi_s, rho_0, zeta_m1, zeta_0, alpha_s, rho_1, zeta_1, r0, r1, w1, x, ss, mutant=None):
    """cmi_bicgstab_m_update_xs_*: returns (x, ss, zeta_m1, zeta_0, rho_0) after the update and the rotation behind it."""
    x, ss = x.copy(), ss.copy()
    rr1 = r0 if mutant == "xs_r0" else r1
    with np.errstate(all="ignore"):
        for s in range(num_shifts):
            sl = slice(s * ld, s * ld + n)
            s_0 = ss[sl].copy()
            z1s, b0s, c0s = zeta_1[s], beta_s[s], chi_s[s]
            rho_x = rho_1[s] if mutant == "xs_rho1" else rho_0[s]
            x[sl] = x[sl] - b0s * s_0 + c0s * rho_x * z1s * w1
            ss[sl] = z1s * rho_1[s] * rr1 + alpha_s[s] * (s_0 - c0s * rho_0[s] / b0s * (z1s * w1 - zeta_0[s] * r0))
    if mutant == "rotation":
        new_z0 = zeta_1.copy()
        new_zm1 = new_z0.copy()
    else:
        new_zm1, new_z0 = zeta_0.copy(), zeta_1.copy()
    return x, ss, new_zm1, new_z0, rho_1.copy()


# ---- the two solvers, as the header layer's host_memory path runs them --------------------------------------------------------
def cg_m(A, b, sigma, iteration_limit, relative_tolerance, mutant=None):
    """Returns (x as num_shifts x N, the monitor)."""
    T = b.dtype.type
    N, ns = b.size, sigma.size
    mon = Monitor(b, iteration_limit, relative_tolerance)
    r, p0 = b.copy(), b.copy()
    x, ps = np.zeros(N * ns, b.dtype), np.tile(b, ns)
    zm1, z0 = np.ones(ns, b.dtype), np.ones(ns, b.dtype)
    beta_0, alpha_0 = T(1), T(0)
    rsq_1 = dot(r, r)
    while not mon.finished(r):
        rsq_0, beta_m1 = rsq_1, beta_0
        Ap = spmv(A, p0)
        beta_0 = T(-rsq_0 / dot(p0, Ap))
        r = (beta_0 * Ap + r).astype(T)
        alpha_old = alpha_0
        rsq_1 = dot(r, r)
        alpha_0 = T(rsq_1 / rsq_0)
        z1, beta_s = zb(T, beta_m1, beta_0, alpha_0 if mutant == "zb_new_alpha" else alpha_old, z0, zm1, sigma, mutant)
        p0 = (T(1) * r + alpha_0 * p0).astype(T)
        alpha_s = ka(T, beta_0, alpha_0, z0, z1, beta_s)
        _, x, ps = cg_m_update_xp(T, N, ns, N, None, beta_s, alpha_s, z1, r, None, x, ps, mutant)
        if mutant == "rotation":
            z0 = z1.copy()
            zm1 = z0.copy()
        else:
            zm1, z0 = z0, z1
        mon.iteration_count += 1
    return x.reshape(ns, N), mon


def bicgstab_m(A, b, sigma, iteration_limit, relative_tolerance, mutant=None):
    """Returns (x as num_shifts x N, the monitor)."""
    T = b.dtype.type
    N, ns = b.size, sigma.size
    mon = Monitor(b, iteration_limit, relative_tolerance)
    r0, w1, w0, s0 = b.copy(), b.copy(), b.copy(), b.copy()
    x, ss = np.zeros(N * ns, b.dtype), np.tile(b, ns)
    zm1, z0, rho0 = np.ones(ns, b.dtype), np.ones(ns, b.dtype), np.ones(ns, b.dtype)
    beta_0, alpha_0 = T(1), T(0)
    As = spmv(A, s0)
    with np.errstate(all="ignore"):
        delta_1 = dot(w0, r0)
        phi_0 = T(dot(w0, As) / delta_1)
        while not mon.finished(r0):
            beta_m1 = beta_0
            beta_0 = T(T(-1.0) / phi_0)
            delta_0 = delta_1
            w1 = (T(1) * r0 + beta_0 * As).astype(T)
            Aw = spmv(A, w1)
            chi_0 = T(dot(Aw, w1) / dot(Aw, Aw))
            r1 = (T(1) * w1 + (-chi_0) * Aw).astype(T)
            delta_1 = dot(w0, r1)
            alpha_old = alpha_0
            alpha_0 = T(-beta_0 * delta_1 / delta_0 / chi_0)
            s0 = bicgstab_m_s(T, alpha_0, chi_0, r1, As, s0)
            As = spmv(A, s0)
            phi_0 = T(dot(w0, As) / delta_1)
            z1, beta_s, chi_s, rho1, alpha_s = bicgstab_m_coefficients(T, beta_m1, beta_0, alpha_old, alpha_0, chi_0, sigma, zm1, z0, rho0, mutant)
            x, ss, zm1, z0, rho0 = bicgstab_m_update_xs(T, N, ns, N, beta_s, chi_s, rho0, zm1, z0, alpha_s, rho1, z1, r0, r1, w1, x, ss, mutant)
            r0 = r1
            mon.iteration_count += 1
    return x.reshape(ns, N), mon


def relative_residuals(A, x, b, sigma):
    """||b - (A + sigma_s I) x_s|| / ||b|| per shift, in double."""
    D = dense(A)
    b64 = b.astype(np.float64)
    return [float(np.linalg.norm(b64 - (D + float(s) * np.eye(b.size)) @ x[k].astype(np.float64)) / np.linalg.norm(b64)) for k, s in enumerate(sigma)]

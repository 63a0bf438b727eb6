"""numpy restatements of what cusp::eigen computes (cusp/eigen/spectral_radius.h, arnoldi.h, csrc/eigen.hip), in the value
type's own arithmetic: the power iteration, Arnoldi and Lanczos WITH the completed column kept on breakdown (and, as a
mutant, with the reference's rule that drops it), the Ritz step, the absolute row sums per format, the library's hash
and the normalise step's host sequence.  Shared by tests/test_eigen_refs.py (CPU) and tests/test_eigen_gpu.py."""
import math

import numpy as np

BREAKDOWN = 1e-10
M64 = (1 << 64) - 1


# ---- matrices -------------------------------------------------------------------------------------------------------
def poisson5pt(m, n, dtype=np.float64):
    """Dense 5-point Poisson matrix on an m x n grid (cusp::gallery::poisson5pt: x runs fastest, 4 on the diagonal)."""
    N = m * n
    A = np.zeros((N, N), dtype)
    for y in range(n):
        for x in range(m):
            i = y * m + x
            A[i, i] = 4
            if x > 0: A[i, i - 1] = -1
            if x + 1 < m: A[i, i + 1] = -1
            if y > 0: A[i, i - m] = -1
            if y + 1 < n: A[i, i + m] = -1
    return A


def poisson_rho(m, n):
    return 4 + 2 * math.cos(math.pi / (m + 1)) + 2 * math.cos(math.pi / (n + 1))


def poisson_operator(m, n, dtype, scale=None):
    """y = A x for the 5-point matrix without storing it (rounded to dtype after every operation, as a sparse row sum is up to
    its order -- the estimators' criterion is 0.1, not bits); scale: an optional row scaling (D^-1)."""
    def apply(v):
        g = v.reshape(n, m)
        out = (dtype(4) * g).astype(dtype)
        out[:, 1:] -= g[:, :-1]
        out[:, :-1] -= g[:, 1:]
        out[1:, :] -= g[:-1, :]
        out[:-1, :] -= g[1:, :]
        out = out.reshape(-1)
        return out if scale is None else (out * scale).astype(dtype)
    return apply


def dense_operator(A):
    return lambda v: (A @ v).astype(A.dtype)


# ---- the estimators ---------------------------------------------------------------------------------------------------
def power_iteration(apply, x0, k):
    """estimate_spectral_radius: k times (scale by the maximum norm, multiply); the ratio of the last two 2-norms."""
    dtype = x0.dtype.type
    x = x0.copy()
    y = x
    for _ in range(k):
        y = (x * (dtype(1) / np.max(np.abs(x)))).astype(dtype)
        x = apply(y)
    if k == 0:
        return 0.0
    return float(dtype(np.sqrt(np.dot(x, x))) / dtype(np.sqrt(np.dot(y, y))))


def arnoldi(apply, x0, k, keep_column=True):
    """cusp::eigen::arnoldi: modified Gram-Schmidt; on breakdown at step j the block is (j + 1) x (j + 1) -- the completed
    column stays.  keep_column=False restores the reference's rule (j x j): the mutant."""
    dtype = x0.dtype.type
    N = x0.size
    maxiter = min(N, k)
    H = np.zeros((maxiter + 1, maxiter), dtype)
    V = [(x0 * (dtype(1) / dtype(np.sqrt(np.dot(x0, x0))))).astype(dtype)]
    size = maxiter
    for j in range(maxiter):
        w = apply(V[j])
        for i in range(j + 1):
            H[i, j] = np.dot(V[i], w)
            w = (w - H[i, j] * V[i]).astype(dtype)
        beta = dtype(np.sqrt(np.dot(w, w)))
        H[j + 1, j] = beta
        if beta < BREAKDOWN:
            size = j + 1 if keep_column else j
            break
        V.append((w * (dtype(1) / beta)).astype(dtype))
    return H[:size, :size].copy()


def lanczos(apply, x0, k, keep_column=True):
    """detail::lanczos_estimate: the three-term loop, the same breakdown rule."""
    dtype = x0.dtype.type
    N = x0.size
    maxiter = min(N, k)
    H = np.zeros((maxiter + 1, maxiter), dtype)
    v0 = np.zeros(N, dtype)
    v1 = (x0 * (dtype(1) / dtype(np.sqrt(np.dot(x0, x0))))).astype(dtype)
    beta = dtype(0)
    size = maxiter
    for j in range(maxiter):
        w = apply(v1)
        if j >= 1:
            H[j - 1, j] = beta
            w = (w - beta * v0).astype(dtype)
        alpha = dtype(np.dot(w, v1))
        H[j, j] = alpha
        w = (w - alpha * v1).astype(dtype)
        beta = dtype(np.sqrt(np.dot(w, w)))
        H[j + 1, j] = beta
        if beta < BREAKDOWN:
            size = j + 1 if keep_column else j
            break
        v0, v1 = v1, (w * (dtype(1) / beta)).astype(dtype)
    return H[:size, :size].copy()


def ritz(H, x0, k=20):
    """The Ritz step of ritz_spectral_radius: the power iteration on the small Hessenberg matrix."""
    if H.shape[0] == 0:
        return 0.0
    return power_iteration(dense_operator(H), x0[:H.shape[0]].astype(H.dtype), k)


def ritz_spectral_radius(apply, x0, k=10, symmetric=False, keep_column=True, x0_small=None):
    H = (lanczos if symmetric else arnoldi)(apply, x0, k, keep_column)
    return ritz(H, x0 if x0_small is None else x0_small)


# ---- absolute row sums per format (the entries each format's multiply reads) --------------------------------------------------
def csr_abs_row_sums(Ap, Ax):
    """The exactly rounded sum of |a| per row (math.fsum)."""
    return np.array([math.fsum(abs(float(v)) for v in Ax[Ap[i]:Ap[i + 1]]) for i in range(len(Ap) - 1)], np.float64)


def ell_abs_row_sums(num_rows, width, pitch, Ax, row_lengths=None):
    out = np.zeros(num_rows, np.float64)
    for i in range(num_rows):
        w = width if row_lengths is None else min(width, max(0, int(row_lengths[i])))
        out[i] = math.fsum(abs(float(Ax[n * pitch + i])) for n in range(w))
    return out


def dia_abs_row_sums(num_rows, num_cols, pitch, offsets, values):
    out = np.zeros(num_rows, np.float64)
    for i in range(num_rows):
        out[i] = math.fsum(abs(float(values[d * pitch + i])) for d, off in enumerate(offsets) if 0 <= i + int(off) < num_cols)
    return out


def hyb_abs_row_sums(num_rows, width, pitch, ell_Ax, coo_Ai, coo_Ax):
    """The terms of the ELL part and of the COO part of every row, summed exactly."""
    terms = [[abs(float(ell_Ax[n * pitch + i])) for n in range(width)] for i in range(num_rows)]
    for i, v in zip(coo_Ai, coo_Ax):
        terms[int(i)].append(abs(float(v)))
    return np.array([math.fsum(t) for t in terms], np.float64)


def row_lengths(Ap):
    return np.diff(np.asarray(Ap, np.int64))


# ---- the library's hash (cusp/detail/random_hash.h: splitmix64's output function) and the normalise step -----------
def random_hash(i, seed):
    z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def random_fill(n, seed, dtype):
    """cmi_random_fill_*: f64 (h >> 11) * 2^-53, f32 (h >> 40) * 2^-24 -- both exact."""
    i = np.arange(1, n + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + i * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    if np.dtype(dtype) == np.float64:
        return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def scal_recip(x, s, squared):
    """The host sequence `beta = nrm2(w); scal(w, T(1) / beta)`: s a T, or a double holding the norm's square (its root taken in
    double and rounded to T once); the reciprocal formed once in T, one multiply per element."""
    dtype = x.dtype.type
    s = dtype(np.sqrt(np.float64(s))) if squared else dtype(s)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = dtype(1) / s
        return (r * x).astype(dtype)

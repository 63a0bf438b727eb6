// cusp/detail/sygv_small.h -- the generalised symmetric eigenproblem A z = w B z for n = 2 or 3 in double, on the host: what cusp::eigen::lobpcg
// needs of the reference's cusp::lapack::sygv (its Rayleigh-Ritz step on the 2 x 2 / 3 x 3 Gram pair) without LAPACK.
//   1. B = L L^T (Cholesky); a pivot that is not a positive finite number: B is not positive definite, the function returns false.
//   2. C = L^-1 A L^-T (the standard problem; symmetrised).
//   3. cyclic Jacobi rotations on C (Golub & Van Loan, "Matrix Computations", 8.5), the rotations accumulated in V.
//   4. eigenvalues sorted ascending, Z = L^-T V: the columns are B-orthonormal (z^T B z = 1), as sygv returns them.
// Nothing is thrown.  The sign of an eigenvector is whatever the rotations leave (LAPACK's is not specified either).
// tests/lobpcg_refs.py restates these steps in numpy, operation by operation.
#pragma once
#include <cmath>

namespace cusp {
namespace detail {

// A, B, Z: n x n, row-major (element (i, j) at [i * n + j]); only the lower triangles of A and B are read.  Column j of Z belongs to w[j].
inline bool sygv_small(int n, const double *A, const double *B, double *w, double *Z)
{
    if (n < 1 || n > 3) return false;
    double L[3][3] = {}, C[3][3] = {}, V[3][3] = {};
    for (int j = 0; j < n; j++) {
        double d = B[j * n + j];
        for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k];
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        L[j][j] = std::sqrt(d);
        for (int i = j + 1; i < n; i++) {
            double s = B[i * n + j];
            for (int k = 0; k < j; k++) s -= L[i][k] * L[j][k];
            L[i][j] = s / L[j][j];
        }
    }
    // Y = L^-1 A (forward substitution on every column of the full symmetric A), then C = Y L^-T = (L^-1 Y^T)^T
    double Y[3][3] = {};
    for (int c = 0; c < n; c++)
        for (int i = 0; i < n; i++) {
            double s = i >= c ? A[i * n + c] : A[c * n + i];
            for (int k = 0; k < i; k++) s -= L[i][k] * Y[k][c];
            Y[i][c] = s / L[i][i];
        }
    for (int r = 0; r < n; r++)
        for (int i = 0; i < n; i++) {
            double s = Y[r][i];
            for (int k = 0; k < i; k++) s -= L[i][k] * C[r][k];
            C[r][i] = s / L[i][i];
        }
    for (int i = 0; i < n; i++)
        for (int j = 0; j < i; j++) C[i][j] = C[j][i] = 0.5 * (C[i][j] + C[j][i]);
    for (int i = 0; i < n; i++) V[i][i] = 1.0;
    for (int sweep = 0; sweep < 60; sweep++) {
        bool rotated = false;
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                const double apq = C[p][q];
                if (!(std::abs(apq) > 1e-18 * (std::abs(C[p][p]) + std::abs(C[q][q])))) continue; // negligible (or NaN)
                rotated = true;
                const double tau = (C[q][q] - C[p][p]) / (2.0 * apq);
                const double t = tau >= 0.0 ? 1.0 / (tau + std::sqrt(1.0 + tau * tau)) : -1.0 / (-tau + std::sqrt(1.0 + tau * tau));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                for (int k = 0; k < n; k++) { // columns p, q:  C <- C J,  V <- V J  with J = [[c, s], [-s, c]]
                    const double ckp = C[k][p], ckq = C[k][q];
                    C[k][p] = c * ckp - s * ckq;
                    C[k][q] = s * ckp + c * ckq;
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
                for (int k = 0; k < n; k++) { // rows p, q:  C <- J^T C
                    const double cpk = C[p][k], cqk = C[q][k];
                    C[p][k] = c * cpk - s * cqk;
                    C[q][k] = s * cpk + c * cqk;
                }
                C[p][q] = C[q][p] = 0.0;
            }
        if (!rotated) break;
    }
    int order[3] = {0, 1, 2};
    for (int i = 1; i < n; i++) // insertion sort, stable
        for (int j = i; j > 0 && C[order[j]][order[j]] < C[order[j - 1]][order[j - 1]]; j--) { const int t = order[j]; order[j] = order[j - 1]; order[j - 1] = t; }
    for (int j = 0; j < n; j++) {
        const int src = order[j];
        w[j] = C[src][src];
        for (int i = n - 1; i >= 0; i--) { // L^T z = v: back substitution
            double s = V[i][src];
            for (int k = i + 1; k < n; k++) s -= L[k][i] * Z[k * n + j];
            Z[i * n + j] = s / L[i][i];
        }
    }
    return true;
}

} // namespace detail
} // namespace cusp

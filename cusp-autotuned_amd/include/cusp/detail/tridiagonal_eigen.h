// cusp/detail/tridiagonal_eigen.h -- the symmetric tridiagonal eigenproblem in double, on the host: what cusp::eigen::lanczos needs of the
// reference's cusp::lapack::stev without LAPACK (the counterpart of sygv_small.h).
//   Implicit QL sweeps with Wilkinson shifts (Golub & Van Loan, "Matrix Computations", 8.3; the EISPACK routine tql2 is the classic form):
//   for every leading position l the matrix is deflated at the first off-diagonal e[m], m >= l, that is negligible beside its two diagonal
//   neighbours (|e[m]| + (|d[m]| + |d[m+1]|) == |d[m]| + |d[m+1]|), and the block l .. m takes one shifted sweep of plane rotations, which
//   are accumulated in Z.  An off-diagonal that is exactly zero (a Lanczos restart stores beta = 0) deflates at once; so does the tiny
//   trailing beta of a run taken to m = N.  Each eigenvalue has a budget of kSweeps sweeps; when it runs out the function returns false.
//   The eigenvalues are sorted ascending at the end, the columns of Z with them.
// Nothing is thrown.  tests/lanczos_refs.py restates these steps in numpy.
#pragma once
#include <cmath>
#include <cstddef>
#include <utility>
#include <vector>

namespace cusp {
namespace detail {

// diagonal[0 .. n), off_diagonal[0 .. n - 1) (off_diagonal[i] couples i and i + 1).  w[0 .. n): the eigenvalues, ascending.  Z: null, or
// n x n column-major (element (i, j) at [j * n + i]): column j is the unit eigenvector of w[j].
inline bool tridiagonal_eigen(size_t n, const double *diagonal, const double *off_diagonal, double *w, double *Z)
{
    const int kSweeps = 60;
    if (n == 0) return true;
    std::vector<double> e(n, 0.0);
    for (size_t i = 0; i < n; i++) w[i] = diagonal[i];
    for (size_t i = 0; i + 1 < n; i++) e[i] = off_diagonal[i];
    if (Z) {
        for (size_t i = 0; i < n * n; i++) Z[i] = 0.0;
        for (size_t i = 0; i < n; i++) Z[i * n + i] = 1.0;
    }
    double *d = w;
    for (size_t l = 0; l < n; l++) {
        int sweeps = 0;
        for (;;) {
            size_t m = l;
            for (; m + 1 < n; m++) {
                const double dd = std::abs(d[m]) + std::abs(d[m + 1]);
                if (std::abs(e[m]) + dd == dd) break;
            }
            if (m == l) break;
            if (sweeps++ == kSweeps) return false;
            double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
            double r = std::hypot(g, 1.0);
            g = d[m] - d[l] + e[l] / (g + std::copysign(r, g));
            double s = 1.0, c = 1.0, p = 0.0;
            bool underflow = false;
            for (size_t i = m; i-- > l;) {
                double f = s * e[i];
                const double b = c * e[i];
                r = std::hypot(f, g);
                e[i + 1] = r;
                if (r == 0.0) { // the rotation is undefined: undo the shift on this element and start the block again
                    d[i + 1] -= p;
                    e[m] = 0.0;
                    underflow = true;
                    break;
                }
                s = f / r;
                c = g / r;
                g = d[i + 1] - p;
                r = (d[i] - g) * s + 2.0 * c * b;
                p = s * r;
                d[i + 1] = g + p;
                g = c * r - b;
                if (Z) {
                    double *zi = Z + i * n, *zj = Z + (i + 1) * n;
                    for (size_t k = 0; k < n; k++) {
                        f = zj[k];
                        zj[k] = s * zi[k] + c * f;
                        zi[k] = c * zi[k] - s * f;
                    }
                }
            }
            if (underflow) continue;
            d[l] -= p;
            e[l] = g;
            e[m] = 0.0;
        }
    }
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(d[i])) return false; // (values that cannot be ordered)
    for (size_t i = 0; i + 1 < n; i++) { // selection sort: n is a few hundred at most, and the columns move once
        size_t k = i;
        for (size_t j = i + 1; j < n; j++)
            if (d[j] < d[k]) k = j;
        if (k != i) {
            std::swap(d[i], d[k]);
            if (Z)
                for (size_t q = 0; q < n; q++) std::swap(Z[i * n + q], Z[k * n + q]);
        }
    }
    return true;
}

} // namespace detail
} // namespace cusp

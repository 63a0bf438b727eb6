// cusp/gallery/diffusion.h -- cusp::gallery::diffusion<Method>(matrix, m, n, eps = 1e-5, theta = pi / 4), Method = FD or FE
// (reference cusp/gallery/diffusion.h, detail/diffusion.inl): the anisotropic diffusion operator -div(K grad u) on an m x n
// grid, K = Q diag(1, eps) Q^T with Q the rotation by theta, as a nine-point stencil
//     (-1,-1) a  ( 0,-1) b  ( 1,-1) c      FD: a = 0.5 (eps - 1) CS, b = -(eps SS + CC), c = -a, d = -(eps CC + SS), e = 2 (eps + 1)
//     (-1, 0) d  ( 0, 0) e  ( 1, 0) d      FE: the bilinear (Q1) element stencil, every value divided by 6
//     (-1, 1) c  ( 0, 1) b  ( 1, 1) a      (C = cos theta, S = sin theta, CC = C C, SS = S S, CS = C S)
// in the reference's order.  C, S and their products are formed in the matrix's value type; every expression with a double
// literal is evaluated in double and rounded once on assignment, as the reference's C++ does.  The matrix goes through
// generate_matrix_from_stencil (a host DIA matrix, then cusp::convert): a stencil value that is exactly zero (a and c of FD at
// theta = 0) leaves no entry in CSR, COO, ELL and HYB.  All five formats; a device_memory target is built on the host and copied.
#pragma once
#include <cmath>
#include <type_traits>

#include "poisson.h"

namespace cusp {
namespace gallery {

struct FD {};
struct FE {};

namespace detail {

template <typename Matrix> struct host_twin;
template <template <typename, typename, typename> class Format, typename I, typename V, typename Space> struct host_twin<Format<I, V, Space>> {
    typedef Format<I, V, cusp::host_memory> type;
};

template <typename Method, typename V> std::vector<stencil_point> diffusion_stencil(double eps, double theta)
{
    static_assert(std::is_same<Method, FD>::value || std::is_same<Method, FE>::value, "cusp::gallery::diffusion: the discretisation method is FD or FE");
    const V C = std::cos(theta), S = std::sin(theta);
    const V CC = C * C, SS = S * S, CS = C * S;
    V a, b, c, d, e;
    if (std::is_same<Method, FE>::value) {
        a = (-1.0 * eps - 1.0) * CC + (-1.0 * eps - 1.0) * SS + (3.0 * eps - 3.0) * CS;
        b = (2.0 * eps - 4.0) * CC + (-4.0 * eps + 2.0) * SS;
        c = (-1.0 * eps - 1.0) * CC + (-1.0 * eps - 1.0) * SS + (-3.0 * eps + 3.0) * CS;
        d = (-4.0 * eps + 2.0) * CC + (2.0 * eps - 4.0) * SS;
        e = (8.0 * eps + 8.0) * CC + (8.0 * eps + 8.0) * SS;
        a /= 6.0;
        b /= 6.0;
        c /= 6.0;
        d /= 6.0;
        e /= 6.0;
    } else {
        a = 0.5 * (eps - 1.0) * CS;
        b = -(eps * SS + CC);
        c = -a;
        d = -(eps * CC + SS);
        e = 2.0 * (eps + 1.0);
    }
    return {{-1, -1, 0, (double)a}, {0, -1, 0, (double)b}, {1, -1, 0, (double)c}, {-1, 0, 0, (double)d}, {0, 0, 0, (double)e},
            {1, 0, 0, (double)d},   {-1, 1, 0, (double)c}, {0, 1, 0, (double)b},  {1, 1, 0, (double)a}};
}

template <typename Method, typename Matrix> void diffusion_impl(Matrix &matrix, size_t m, size_t n, double eps, double theta, cusp::host_memory)
{
    generate_matrix_from_stencil(matrix, diffusion_stencil<Method, typename Matrix::value_type>(eps, theta), m, n);
}
template <typename Method, typename Matrix> void diffusion_impl(Matrix &matrix, size_t m, size_t n, double eps, double theta, cusp::device_memory)
{
    typename host_twin<Matrix>::type host;
    diffusion_impl<Method>(host, m, n, eps, theta, cusp::host_memory());
    matrix = host;
}

} // namespace detail

template <typename Method, typename MatrixType> void diffusion(MatrixType &matrix, size_t m, size_t n, const double eps = 1e-5, const double theta = M_PI / 4.0)
{
    detail::diffusion_impl<Method>(matrix, m, n, eps, theta, typename MatrixType::memory_space());
}

} // namespace gallery
} // namespace cusp

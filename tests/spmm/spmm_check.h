// Shared by the SpMM test programs: small CSR builders and the naive storage-order loop every result is checked against
// (sequential/multiply/csr_block_spmv.h: per element, initialize, then each entry of the row in storage order,
// multiply then add).
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include <cusp/array2d.h>
#include <cusp/csr_matrix.h>
#include <cusp/gallery/poisson.h>
#include <cusp/io/matrix_market.h>
#include <cusp/multiply.h>

#include "unittest.h"

namespace spmm_check {

// seeded values in [-8, 8) with a fractional part, so that sums are not exact and the order shows in the bits
inline double seeded(uint64_t i)
{
    uint64_t z = i * 0x9E3779B97F4A7C15ull + 0x2545F4914F6CDD1Dull;
    z ^= z >> 31; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 29;
    return (double)(z % 4096) / 256.0 - 8.0 + 1.0 / 3.0;
}

template <typename V, typename O> void fill(cusp::array2d<V, cusp::host_memory, O> &a, uint64_t salt)
{
    for (size_t i = 0; i < a.num_rows; i++)
        for (size_t c = 0; c < a.num_cols; c++) a(i, c) = (V)seeded(salt + i * 131 + c * 7);
}

// Y(i, c) = [Y(i, c) +] sum over the row in storage order of Ax[jj] * X(Aj[jj], c)
template <typename M, typename XA, typename YA> void naive(const M &A, const XA &X, YA &Y, bool accumulate)
{
    typedef typename YA::value_type V;
    for (size_t i = 0; i < A.num_rows; i++)
        for (size_t c = 0; c < X.num_cols; c++) {
            V acc = accumulate ? Y(i, c) : V(0);
            for (int jj = A.row_offsets[i]; jj < A.row_offsets[i + 1]; jj++) acc = acc + A.values[jj] * X(A.column_indices[jj], c);
            Y(i, c) = acc;
        }
}

template <typename V, typename O1, typename O2>
bool bits_equal(const cusp::array2d<V, cusp::host_memory, O1> &a, const cusp::array2d<V, cusp::host_memory, O2> &b)
{
    if (a.num_rows != b.num_rows || a.num_cols != b.num_cols) return false;
    for (size_t i = 0; i < a.num_rows; i++)
        for (size_t c = 0; c < a.num_cols; c++) {
            const V x = a(i, c), y = b(i, c);
            if (std::memcmp(&x, &y, sizeof(V)) != 0) return false;
        }
    return true;
}

// CSR of an irregular matrix: row lengths 0..24 (some empty rows), seeded columns and values
template <typename V> cusp::csr_matrix<int, V, cusp::host_memory> irregular(size_t rows, size_t cols, uint64_t salt)
{
    std::vector<int> Ap(1, 0), Aj;
    std::vector<V> Ax;
    for (size_t i = 0; i < rows; i++) {
        const int len = (int)((uint64_t)(seeded(salt + i) * 256.0 + 4096.0) % 25);
        for (int t = 0; t < len; t++) {
            Aj.push_back((int)((uint64_t)(seeded(salt + 977 * i + t) * 256.0 + 4096.0) * 7919 % cols));
            Ax.push_back((V)seeded(salt + 31 * i + 5 * t + 1));
        }
        Ap.push_back((int)Aj.size());
    }
    cusp::csr_matrix<int, V, cusp::host_memory> A(rows, cols, Aj.size());
    for (size_t i = 0; i <= rows; i++) A.row_offsets[i] = Ap[i];
    for (size_t n = 0; n < Aj.size(); n++) { A.column_indices[n] = Aj[n]; A.values[n] = Ax[n]; }
    return A;
}

} // namespace spmm_check

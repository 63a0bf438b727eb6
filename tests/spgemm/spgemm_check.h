// Shared by the SpGEMM test programs: seeded CSR builders with unsorted rows, duplicate columns and explicit zeros, and the
// naive product every result is checked against -- per output entry the chain s = 0; s = s + a * b over the entry's products in
// expansion order (A's row in storage order, then B's row in storage order), columns ascending; zeros kept or dropped.
#pragma once
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include <cusp/coo_matrix.h>
#include <cusp/csr_matrix.h>
#include <cusp/convert.h>
#include <cusp/gallery/poisson.h>
#include <cusp/io/matrix_market.h>
#include <cusp/multiply.h>

#include "unittest.h"

namespace spgemm_check {

inline uint64_t mix(uint64_t i)
{
    uint64_t z = i * 0x9E3779B97F4A7C15ull + 0x2545F4914F6CDD1Dull;
    z ^= z >> 31; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 29;
    return z;
}
// values in [-8, 8) with a fractional part, so that sums are not exact and the order shows in the bits
inline double seeded(uint64_t i) { return (double)(mix(i) % 4096) / 256.0 - 8.0 + 1.0 / 3.0; }

template <typename V> using host_csr = cusp::csr_matrix<int, V, cusp::host_memory>;

template <typename V> host_csr<V> from_rows(size_t rows, size_t cols, const std::vector<std::vector<std::pair<int, V>>> &r)
{
    size_t nnz = 0;
    for (auto &row : r) nnz += row.size();
    host_csr<V> A(rows, cols, nnz);
    size_t n = 0;
    A.row_offsets[0] = 0;
    for (size_t i = 0; i < rows; i++) {
        for (auto &e : r[i]) { A.column_indices[n] = e.first; A.values[n] = e.second; n++; }
        A.row_offsets[i + 1] = (int)n;
    }
    return A;
}

// row lengths 0..max_len (some empty rows), columns anywhere (unsorted, duplicates), one value in sixteen an explicit zero
template <typename V> host_csr<V> irregular(size_t rows, size_t cols, int max_len, uint64_t salt)
{
    std::vector<std::vector<std::pair<int, V>>> r(rows);
    for (size_t i = 0; i < rows; i++) {
        const int len = (int)(mix(salt + i) % (uint64_t)(max_len + 1));
        for (int t = 0; t < len; t++) {
            const uint64_t h = salt + 977 * i + 13 * (uint64_t)t;
            r[i].push_back({(int)(mix(h) % cols), mix(h + 5) % 16 == 0 ? V(0) : (V)seeded(h + 1)});
        }
    }
    return from_rows<V>(rows, cols, r);
}

template <typename M1, typename M2> auto naive(const M1 &A, const M2 &B, bool keep_zeros) -> host_csr<typename M1::value_type>
{
    typedef typename M1::value_type V;
    std::vector<std::vector<std::pair<int, V>>> rows(A.num_rows);
    for (size_t i = 0; i < A.num_rows; i++) {
        std::map<int, V> sums; // (ascending columns; value-initialised to +0 at the first touch)
        for (int jj = A.row_offsets[i]; jj < A.row_offsets[i + 1]; jj++) {
            const int j = A.column_indices[jj];
            for (int kk = B.row_offsets[j]; kk < B.row_offsets[j + 1]; kk++) {
                V &s = sums[B.column_indices[kk]];
                const V p = A.values[jj] * B.values[kk];
                s = s + p;
            }
        }
        for (auto &e : sums)
            if (keep_zeros || e.second != V(0)) rows[i].push_back({e.first, e.second});
    }
    return from_rows<V>(A.num_rows, B.num_cols, rows);
}

template <typename M> host_csr<typename M::value_type> without_zeros(const M &C)
{
    typedef typename M::value_type V;
    std::vector<std::vector<std::pair<int, V>>> rows(C.num_rows);
    for (size_t i = 0; i < C.num_rows; i++)
        for (int q = C.row_offsets[i]; q < C.row_offsets[i + 1]; q++)
            if (C.values[q] != V(0)) rows[i].push_back({C.column_indices[q], C.values[q]});
    return from_rows<V>(C.num_rows, C.num_cols, rows);
}

template <typename M1, typename M2> bool csr_bits_equal(const M1 &a, const M2 &b)
{
    typedef typename M1::value_type V;
    if (a.num_rows != b.num_rows || a.num_cols != b.num_cols || a.num_entries != b.num_entries) return false;
    for (size_t i = 0; i <= a.num_rows; i++)
        if (a.row_offsets[i] != b.row_offsets[i]) return false;
    for (size_t q = 0; q < a.num_entries; q++) {
        const V x = a.values[q], y = b.values[q];
        if (a.column_indices[q] != b.column_indices[q]) return false;
        if (!(x != x && y != y) && std::memcmp(&x, &y, sizeof(V)) != 0) return false; // (a NaN equals a NaN whatever its payload)
    }
    return true;
}

template <typename M> bool rows_strictly_ascending(const M &C)
{
    for (size_t i = 0; i < C.num_rows; i++)
        for (int q = C.row_offsets[i] + 1; q < C.row_offsets[i + 1]; q++)
            if (C.column_indices[q - 1] >= C.column_indices[q]) return false;
    return true;
}

} // namespace spgemm_check

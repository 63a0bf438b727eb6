// cusp/precond/aggregation/strength.h -- symmetric_strength_of_connection(A, S, theta = 0) and strength_of_connection
// (reference cusp/precond/aggregation/strength.h; sequential loop system/detail/sequential/symmetric_strength.h).
// S keeps the entries of the square CSR matrix A with |A_ij| >= theta * sqrt(|A_ii| * |A_jj|), in storage order: product and
// square root in the value type, the product with theta and the comparison in double; A_ii is cusp::extract_diagonal's.
//   host_memory   : the reference's sequential loop.
//   device_memory : cmi_csr_strength_symmetric_*; it returns the bits of the host path.
//
// evolution_strength_of_connection(A, S, B, rho_DinvA = 0, epsilon = 4) (reference strength.h,
// system/detail/generic/evolution_strength.h): the measure of Olson, Schroder and Tuminaro with k = 2.  A and S
// are CSR matrices of one memory space (COO operands are converted), B is the candidate vector.  M entries, row(e) / col(e) an
// entry's coordinates, t(e) the position of the entry (col(e), row(e)), T the value type:
//    1  D = extract_diagonal(A)                               2  v[e] = Ax[e] / D[row(e)]
//    3  rho_DinvA == 0: rho = ritz_spectral_radius of that scaled matrix, 8 steps
//    4  v[e] = (row == col) - (1.0 / rho) * v[e]              in double, rounded once; rho is first rounded to T
//    5  data[e] = sum of v[p] * v[t(q)] over the columns that rows row(e) and col(e) have in common (p, q the two positions),
//       in ascending column order from +0, product and sum rounded separately in T: (Atilde Atilde)(row, col)
//    6  DAt[i] = the diagonal entry of data (0 where none)    7  Bs = B with zeros replaced by 1
//    8  a[e] = (1 * DAt[row]) * Bs[col]                       9  neg = data * a < 0
//   10  a = a / data                                         11  weak = a < T(1e-4)
//   12  a = |1.0 - a|  in double, rounded once               13  a = 0 where neg || weak
//   14  a = T(1e-4) where a < sqrt(eps_T) && a != 0           15  s[e] = 0.5 * (a[e] + a[t(e)])  the sum in T, the half in double
//   16  unless epsilon is T's infinity: small[i] = the row's left-to-right non_zero_minimum chain of s, and
//       s[e] = (s[e] >= T(epsilon) * small[row]) ? 0 : s[e]   (the reference's functor holds epsilon in T)
//   17  s[e] = 1 on the diagonal                             18  s[e] = s[e] + s[t(e)]
//   19  S = the entries with s[e] != 0, in storage order
// Deliberate departures from the reference:
//   (a) the values of S are the final s[e] (the reference's copy_if writes indices only and leaves the values unset);
//   (b) the reference's permutation trick silently assumes a symmetric pattern with rows sorted by column and no repeated
//       column: here the pattern is checked (on the device for device_memory) and refused with invalid_input_exception;
//   (c) t(e) comes from a search of row col(e) for row(e), not from a sort of the column indices: the same map on such input;
//   (d) the host_memory path is a sequential loop written here; it is the contract the device path returns bit for bit;
//   (e) step 3 uses this project's start vector, not the reference's: the estimate differs from the reference's in its digits.
//   host_memory   : the loops below.
//   device_memory : cmi_csr_evolution_strength_* (step 3: cmi_csr_scale_rows_* with lambda = 1, then ritz_spectral_radius).
#pragma once
#include <cmath>
#include <limits>
#include <vector>

#include "../../coo_matrix.h"
#include "../../csr_matrix.h"
#include "../../eigen/spectral_radius.h"
#include "../../execution_policy.h"
#include "../../format_utils.h"

namespace cusp {
namespace precond {
namespace aggregation {
namespace detail {

template <typename A, typename S> void strength(const A &a, S &s, double theta, cusp::host_memory)
{
    typedef typename S::index_type I;
    typedef typename S::value_type V;
    cusp::array1d<V, cusp::host_memory> d;
    cusp::extract_diagonal(a, d);
    std::vector<I> Sp(a.num_rows + 1, I(0)), Sj;
    std::vector<V> Sx;
    for (size_t i = 0; i < a.num_rows; i++) {
        const V aii = d[i];
        for (auto jj = a.row_offsets[i]; jj < a.row_offsets[i + 1]; jj++) {
            const I j = a.column_indices[jj];
            const V aij = a.values[jj], ajj = (j >= 0 && static_cast<size_t>(j) < a.num_rows) ? d[j] : V(0);
            const V prod = std::abs(aii) * std::abs(ajj);
            const V root = std::sqrt(prod);
            if (static_cast<double>(std::abs(aij)) >= theta * static_cast<double>(root)) {
                Sj.push_back(j);
                Sx.push_back(aij);
            }
        }
        Sp[i + 1] = static_cast<I>(Sj.size());
    }
    s.resize(a.num_rows, a.num_cols, Sj.size());
    for (size_t i = 0; i <= s.num_rows; i++) s.row_offsets[i] = Sp[i];
    for (size_t q = 0; q < Sj.size(); q++) {
        s.column_indices[q] = Sj[q];
        s.values[q] = Sx[q];
    }
}

template <typename A, typename S> void strength(const A &a, S &s, double theta, cusp::device_memory)
{
    typedef typename S::value_type V;
    cusp::csr_matrix<int, V, cusp::device_memory> t(a.num_rows, a.num_cols, a.num_entries);
    const int64_t n = (int64_t)a.num_rows, nnz = (int64_t)a.num_entries; // square: n rows and n columns; t holds up to nnz entries
    cusp::detail::check(cusp::detail::by_type<V>(cmi_csr_strength_symmetric_f64, cmi_csr_strength_symmetric_f32)(
        n, n, nnz, a.row_offsets.data(), a.column_indices.data(), a.values.data(), theta,
                                                                                                                 t.row_offsets.data(), t.column_indices.data(), t.values.data(), nnz, nullptr));
    cusp::detail::take_compacted(t, s);
}

// t(e) for a host CSR matrix; false when the pattern does not conform (departure (b))
template <typename A> bool transpose_positions(const A &a, std::vector<int> &tpos, std::vector<int> &rows)
{
    const long n = (long)a.num_rows, M = (long)a.num_entries;
    tpos.assign((size_t)M, 0);
    rows.assign((size_t)M, 0);
    if (a.row_offsets.size() != (size_t)n + 1 || a.row_offsets[0] != 0 || (long)a.row_offsets[n] != M) return false;
    for (long i = 0; i < n; i++) {
        const long lo = a.row_offsets[i], hi = a.row_offsets[i + 1];
        if (lo < 0 || hi < lo || hi > M) return false;
        for (long e = lo; e < hi; e++) {
            const long j = a.column_indices[e];
            if (j < 0 || j >= n || (e > lo && (long)a.column_indices[e - 1] >= j)) return false;
            rows[e] = (int)i;
        }
    }
    for (long e = 0; e < M; e++) {
        const long j = a.column_indices[e];
        long lo = a.row_offsets[j], hi = a.row_offsets[j + 1];
        const long end = hi;
        while (lo < hi) { // the first position of row j whose column is >= row(e)
            const long mid = lo + (hi - lo) / 2;
            if ((long)a.column_indices[mid] < (long)rows[e]) lo = mid + 1;
            else hi = mid;
        }
        if (lo >= end || (long)a.column_indices[lo] != (long)rows[e]) return false;
        tpos[e] = (int)lo;
    }
    return true;
}

template <typename V> V non_zero_minimum(V lhs, V rhs)
{
    if (lhs == V(0)) return rhs;
    if (rhs == V(0)) return lhs;
    return lhs < rhs ? lhs : rhs;
}

// the scaled values of step 2 (the operator of step 3)
template <typename A, typename V> void evolution_scaled_values(const A &a, cusp::array1d<V, cusp::host_memory> &v, cusp::host_memory)
{
    cusp::array1d<V, cusp::host_memory> d;
    cusp::extract_diagonal(a, d);
    v.resize(a.num_entries);
    for (size_t i = 0; i < a.num_rows; i++)
        for (auto e = a.row_offsets[i]; e < a.row_offsets[i + 1]; e++) v[e] = a.values[e] / d[i];
}
template <typename A, typename V> void evolution_scaled_values(const A &a, cusp::array1d<V, cusp::device_memory> &v, cusp::device_memory)
{
    cusp::array1d<V, cusp::device_memory> d;
    cusp::extract_diagonal(a, d);
    v.resize(a.num_entries);
    cusp::detail::check(cusp::detail::by_type<V>(cmi_csr_scale_rows_f64, cmi_csr_scale_rows_f32)((int64_t)a.num_rows, (int64_t)a.num_entries, a.row_offsets.data(),
                                                                                                a.values.data(), d.data(), V(1), v.data(), nullptr));
    cusp::detail::check(cmi_stream_synchronize(nullptr));
}

template <typename A, typename S, typename Array> void evolution(const A &a, S &s_out, const Array &B, double rho, double epsilon, cusp::host_memory)
{
    typedef typename S::index_type I;
    typedef typename S::value_type V;
    const size_t n = a.num_rows, M = a.num_entries;
    std::vector<int> tpos, rows;
    if (!transpose_positions(a, tpos, rows))
        throw cusp::invalid_input_exception("evolution_strength_of_connection: the pattern must be symmetric, with every row strictly ascending by column");
    cusp::array1d<V, cusp::host_memory> D;
    cusp::extract_diagonal(a, D); // step 1
    const V rho_t = static_cast<V>(rho);
    const double inv = 1.0 / static_cast<double>(rho_t);
    std::vector<V> v(M), data(M), DAt(n, V(0)), x(M), s(M), small(n, std::numeric_limits<V>::max());
    for (size_t e = 0; e < M; e++) { // steps 2 and 4
        const V scaled = a.values[e] / D[rows[e]];
        const double prod = inv * static_cast<double>(scaled);
        v[e] = static_cast<V>((rows[e] == (int)a.column_indices[e] ? 1.0 : 0.0) - prod);
    }
    for (size_t e = 0; e < M; e++) { // step 5: one merge of rows row(e) and col(e)
        V sum = V(0);
        long p = a.row_offsets[rows[e]], q = a.row_offsets[a.column_indices[e]];
        const long pe = a.row_offsets[rows[e] + 1], qe = a.row_offsets[a.column_indices[e] + 1];
        while (p < pe && q < qe) {
            const long cp = a.column_indices[p], cq = a.column_indices[q];
            if (cp == cq) {
                const V prod = v[p] * v[tpos[q]];
                sum = sum + prod;
                p++;
                q++;
            } else if (cp < cq) p++;
            else q++;
        }
        data[e] = sum;
    }
    for (size_t e = 0; e < M; e++) // step 6: extract_diagonal's sum from +0
        if (rows[e] == (int)a.column_indices[e]) DAt[rows[e]] = DAt[rows[e]] + data[e];
    const V perfect = std::sqrt(std::numeric_limits<V>::epsilon());
    for (size_t e = 0; e < M; e++) { // steps 7 to 14
        V b = B[a.column_indices[e]];
        if (b == V(0)) b = V(1);
        const V scaled_row = V(1) * DAt[rows[e]];
        V r = scaled_row * b;
        const V angle = data[e] * r;
        const bool neg = angle < V(0);
        r = r / data[e];
        const bool weak = r < static_cast<V>(1e-4);
        r = static_cast<V>(std::fabs(1.0 - static_cast<double>(r)));
        if (neg || weak) r = V(0);
        if (r < perfect && r != V(0)) r = static_cast<V>(1e-4);
        x[e] = r;
    }
    for (size_t e = 0; e < M; e++) { // step 15
        const V both = x[e] + x[tpos[e]];
        s[e] = static_cast<V>(0.5 * static_cast<double>(both));
    }
    if (epsilon != static_cast<double>(std::numeric_limits<V>::infinity())) { // step 16
        const V eps_t = static_cast<V>(epsilon);
        for (size_t i = 0; i < n; i++) {
            const long lo = a.row_offsets[i], hi = a.row_offsets[i + 1];
            if (hi <= lo) continue;
            V acc = s[lo];
            for (long e = lo + 1; e < hi; e++) acc = non_zero_minimum(acc, s[e]);
            small[i] = acc;
        }
        for (size_t e = 0; e < M; e++) {
            const V limit = eps_t * small[rows[e]];
            if (s[e] >= limit) s[e] = V(0);
        }
    }
    for (size_t e = 0; e < M; e++) // step 17
        if (rows[e] == (int)a.column_indices[e]) s[e] = V(1);
    size_t kept = 0;
    for (size_t e = 0; e < M; e++) { // step 18 (x is free: it takes the result)
        x[e] = s[e] + s[tpos[e]];
        kept += x[e] != V(0);
    }
    s_out.resize(n, n, kept); // step 19
    size_t at = 0;
    for (size_t i = 0; i < n; i++) {
        s_out.row_offsets[i] = static_cast<I>(at);
        for (long e = a.row_offsets[i]; e < (long)a.row_offsets[i + 1]; e++)
            if (x[e] != V(0)) {
                s_out.column_indices[at] = a.column_indices[e];
                s_out.values[at] = x[e];
                at++;
            }
    }
    s_out.row_offsets[n] = static_cast<I>(at);
}

template <typename A, typename S, typename Array> void evolution(const A &a, S &s, const Array &B, double rho, double epsilon, cusp::device_memory)
{
    typedef typename S::value_type V;
    cusp::csr_matrix<int, V, cusp::device_memory> t(a.num_rows, a.num_cols, a.num_entries);
    const cusp::array1d<V, cusp::device_memory> b(B);
    const int64_t n = (int64_t)a.num_rows, nnz = (int64_t)a.num_entries;
    int conforming = 0;
    cusp::detail::check(cusp::detail::by_type<V>(cmi_csr_evolution_strength_f64, cmi_csr_evolution_strength_f32)(
        n, nnz, a.row_offsets.data(), a.column_indices.data(), a.values.data(), b.data(), rho, epsilon, t.row_offsets.data(), t.column_indices.data(), t.values.data(), nnz,
        &conforming, nullptr));
    if (!conforming) throw cusp::invalid_input_exception("evolution_strength_of_connection: the pattern must be symmetric, with every row strictly ascending by column");
    cusp::detail::take_compacted(t, s);
}

template <typename A, typename S, typename Array> void evolution_csr(const A &a, S &s, const Array &B, double rho, double epsilon)
{
    typedef typename S::value_type V;
    typedef typename S::memory_space Space;
    if (a.num_rows != a.num_cols) throw cusp::invalid_input_exception("evolution_strength_of_connection: matrix must be square");
    if (B.size() != a.num_rows) throw cusp::invalid_input_exception("evolution_strength_of_connection: the candidate vector must have the matrix's size");
    if (rho == 0.0 && a.num_entries > 0) { // step 3 (a copy of the structure carries the scaled values: set-up work)
        cusp::csr_matrix<int, V, Space> scaled(a);
        evolution_scaled_values(a, scaled.values, Space());
        rho = cusp::eigen::ritz_spectral_radius(scaled, 8);
    }
    if (a.num_entries > 0 && (rho == 0.0 || !std::isfinite(rho))) throw cusp::invalid_input_exception("evolution_strength_of_connection: rho(D^-1 A) is zero or not finite");
    evolution(a, s, B, rho == 0.0 ? 1.0 : rho, epsilon, Space());
}

template <typename A, typename S, typename Array> void evolution_dispatch(const A &a, S &s, const Array &B, double rho, double epsilon, cusp::csr_format, cusp::csr_format)
{
    evolution_csr(a, s, B, rho, epsilon);
}
template <typename A, typename S, typename Array> void evolution_dispatch(const A &a, S &s, const Array &B, double rho, double epsilon, cusp::coo_format, cusp::coo_format)
{
    cusp::csr_matrix<int, typename S::value_type, typename S::memory_space> csr(a), kept;
    evolution_csr(csr, kept, B, rho, epsilon);
    s = kept;
}

} // namespace detail

// S = the evolution measure of A for the candidate vector B (see the head of this file); rho_DinvA == 0: estimated here
template <typename MatrixType1, typename MatrixType2, typename ArrayType>
void evolution_strength_of_connection(const MatrixType1 &A, MatrixType2 &S, const ArrayType &B, double rho_DinvA = 0.0, const double epsilon = 4.0)
{
    static_assert(std::is_same<typename MatrixType1::format, typename MatrixType2::format>::value &&
                      (std::is_same<typename MatrixType1::format, cusp::csr_format>::value || std::is_same<typename MatrixType1::format, cusp::coo_format>::value),
                  "evolution_strength_of_connection is implemented for csr and coo matrices of one format: cusp::convert first");
    static_assert(std::is_same<typename MatrixType1::memory_space, typename MatrixType2::memory_space>::value, "evolution_strength_of_connection: A and S must live in one memory space");
    detail::evolution_dispatch(A, S, B, rho_DinvA, epsilon, typename MatrixType1::format(), typename MatrixType2::format());
}
template <typename Derived, typename MatrixType1, typename MatrixType2, typename ArrayType>
void evolution_strength_of_connection(const cusp::execution_policy<Derived> &, const MatrixType1 &A, MatrixType2 &S, const ArrayType &B, double rho_DinvA = 0.0,
                                      const double epsilon = 4.0)
{
    evolution_strength_of_connection(A, S, B, rho_DinvA, epsilon);
}

template <typename MatrixType1, typename MatrixType2> void symmetric_strength_of_connection(const MatrixType1 &A, MatrixType2 &S, const double theta = 0.0)
{
    static_assert(std::is_same<typename MatrixType1::format, cusp::csr_format>::value && std::is_same<typename MatrixType2::format, cusp::csr_format>::value,
                  "symmetric_strength_of_connection is implemented for csr matrices: cusp::convert first");
    static_assert(std::is_same<typename MatrixType1::memory_space, typename MatrixType2::memory_space>::value, "symmetric_strength_of_connection: A and S must live in one memory space");
    if (A.num_rows != A.num_cols) throw cusp::invalid_input_exception("symmetric_strength_of_connection: matrix must be square");
    detail::strength(A, S, theta, typename MatrixType2::memory_space());
}
template <typename MatrixType1, typename MatrixType2> void strength_of_connection(const MatrixType1 &A, MatrixType2 &S, const double theta = 0.0)
{
    symmetric_strength_of_connection(A, S, theta);
}

} // namespace aggregation
} // namespace precond
} // namespace cusp

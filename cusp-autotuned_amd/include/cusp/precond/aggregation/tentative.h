// cusp/precond/aggregation/tentative.h -- fit_candidates(aggregates, B, Q, R) for one candidate vector
// (reference cusp/precond/aggregation/tentative.h; system/detail/generic/tentative.h).
// Q (n x num_aggregates, CSR) has the entry B[i] / R[aggregates[i]] in every row with aggregates[i] >= 0 and an empty row
// otherwise; R[a] = sqrt(sum of B[i]^2 over the rows of aggregate a), added in ascending row order from the first square
// (the order the reference's stable transpose + reduce_by_key gives).  num_aggregates = max(aggregates) + 1.
//   host_memory   : that loop.   device_memory : cmi_aggregates_fit_*; it returns the bits of the host path.
// Not built: more than one candidate vector.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../csr_matrix.h"
#include "../../format_utils.h"

namespace cusp {
namespace precond {
namespace aggregation {
namespace detail {

template <typename Agg, typename BA, typename Q, typename RA> void fit(const Agg &agg, const BA &B, Q &q, RA &R, size_t na, cusp::host_memory)
{
    typedef typename Q::index_type I;
    typedef typename Q::value_type V;
    const size_t n = agg.size();
    std::vector<V> sum(na, V(0));
    std::vector<char> seen(na, 0);
    size_t inside = 0;
    for (size_t i = 0; i < n; i++) {
        if (agg[i] < 0) continue;
        const V b = B[i], sq = b * b;
        sum[agg[i]] = seen[agg[i]] ? V(sum[agg[i]] + sq) : sq;
        seen[agg[i]] = 1;
        inside++;
    }
    R.resize(na);
    for (size_t a = 0; a < na; a++) R[a] = seen[a] ? V(std::sqrt(sum[a])) : V(0);
    q.resize(n, na, inside);
    size_t at = 0;
    for (size_t i = 0; i < n; i++) {
        q.row_offsets[i] = static_cast<I>(at);
        if (agg[i] < 0) continue;
        q.column_indices[at] = agg[i];
        q.values[at] = V(B[i]) / V(R[agg[i]]);
        at++;
    }
    q.row_offsets[n] = static_cast<I>(at);
}

template <typename Agg, typename BA, typename Q, typename RA> void fit(const Agg &agg, const BA &B, Q &q, RA &R, size_t na, cusp::device_memory)
{
    typedef typename Q::value_type V;
    const size_t n = agg.size();
    cusp::csr_matrix<int, V, cusp::device_memory> t(n, na, n);
    R.resize(na);
    cusp::detail::check(cusp::detail::by_type<V>(cmi_aggregates_fit_f64, cmi_aggregates_fit_f32)((int64_t)n, (int64_t)na, agg.data(), B.data(), t.row_offsets.data(),
                                                                                                 t.column_indices.data(), t.values.data(),
                                                                                                 (int64_t)n, R.data(), nullptr)); // (capacity of t: one entry per row)
    cusp::detail::take_compacted(t, q);
}

} // namespace detail

template <typename ArrayType1, typename ArrayType2, typename MatrixType, typename ArrayType3>
void fit_candidates(const ArrayType1 &aggregates, const ArrayType2 &B, MatrixType &Q, ArrayType3 &R)
{
    static_assert(std::is_same<typename MatrixType::format, cusp::csr_format>::value, "fit_candidates writes a csr matrix");
    if (aggregates.size() != B.size()) throw cusp::invalid_input_exception("fit_candidates: aggregates and B must have the same length");
    const std::vector<typename ArrayType1::value_type> h = cusp::detail::host_copy(aggregates); // (one read: the number of aggregates)
    typename ArrayType1::value_type top = -1;
    for (size_t i = 0; i < h.size(); i++) top = std::max(top, h[i]);
    detail::fit(aggregates, B, Q, R, static_cast<size_t>(top + 1), typename MatrixType::memory_space());
}

} // namespace aggregation
} // namespace precond
} // namespace cusp

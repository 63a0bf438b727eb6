// cusp/elementwise.h -- cusp::add(A, B, C), cusp::subtract(A, B, C) and cusp::elementwise(A, B, C, op) for CSR and COO
// matrices in both memory spaces (reference cusp/elementwise.h; host loop system/detail/sequential/elementwise.h).
//
// C(i,j) = the left-to-right sum of A's entries at (i,j) in storage order, then B's -- each negated first for subtraction --
// starting from the first of them; a result that compares equal to zero is dropped (as in the reference), NaN is kept; C's
// rows come out sorted by column.
//   host_memory   : a merge of the two rows (a row whose columns are not sorted is ordered first by a stable sort, so the
//                   chains keep storage order).
//   device_memory : cmi_csr_elementwise_* (one lane merges a row); when it reports an operand as not sorted the host path
//                   runs on host copies.  Every path returns the bits of the host path.
// `op` of cusp::elementwise is cusp::plus<V> or cusp::minus<V>.  A dimension mismatch throws invalid_input_exception.
#pragma once
#include <algorithm>
#include <vector>

#include "convert.h"
#include "format_utils.h"
#include "coo_matrix.h"
#include "csr_matrix.h"
#include "exception.h"
#include "functional.h"

namespace cusp {

template <typename T> struct minus { T operator()(const T &a, const T &b) const { return a - b; } };

namespace detail {

template <typename V> int elementwise_op(const cusp::plus<V> &) { return 0; }
template <typename V> int elementwise_op(const cusp::minus<V> &) { return 1; }

template <typename A, typename B, typename C> void host_elementwise(const A &a, const B &b, C &c, int op, csr_format)
{
    typedef typename C::index_type I;
    typedef typename C::value_type V;
    struct term { I col; V val; };
    std::vector<term> ra, rb;
    std::vector<I> Cp(a.num_rows + 1, I(0)), Cj;
    std::vector<V> Cx;
    auto by_col = [](const term &x, const term &y) { return x.col < y.col; };
    for (size_t i = 0; i < a.num_rows; i++) {
        ra.clear();
        rb.clear();
        for (auto q = a.row_offsets[i]; q < a.row_offsets[i + 1]; q++) ra.push_back({I(a.column_indices[q]), V(a.values[q])});
        for (auto q = b.row_offsets[i]; q < b.row_offsets[i + 1]; q++) rb.push_back({I(b.column_indices[q]), op ? V(-V(b.values[q])) : V(b.values[q])});
        if (!std::is_sorted(ra.begin(), ra.end(), by_col)) std::stable_sort(ra.begin(), ra.end(), by_col);
        if (!std::is_sorted(rb.begin(), rb.end(), by_col)) std::stable_sort(rb.begin(), rb.end(), by_col);
        size_t ia = 0, ib = 0;
        while (ia < ra.size() || ib < rb.size()) {
            I col;
            if (ib == rb.size() || (ia < ra.size() && ra[ia].col <= rb[ib].col)) col = ra[ia].col;
            else col = rb[ib].col;
            V s = V(0);
            bool first = true;
            for (; ia < ra.size() && ra[ia].col == col; ia++) {
                s = first ? ra[ia].val : V(s + ra[ia].val);
                first = false;
            }
            for (; ib < rb.size() && rb[ib].col == col; ib++) {
                s = first ? rb[ib].val : V(s + rb[ib].val);
                first = false;
            }
            if (!(s == V(0))) {
                Cj.push_back(col);
                Cx.push_back(s);
            }
        }
        Cp[i + 1] = static_cast<I>(Cj.size());
    }
    c.resize(a.num_rows, a.num_cols, Cj.size()); // (after the loops: C may be A or B)
    for (size_t i = 0; i <= c.num_rows; i++) c.row_offsets[i] = Cp[i];
    for (size_t q = 0; q < Cj.size(); q++) {
        c.column_indices[q] = Cj[q];
        c.values[q] = Cx[q];
    }
}
template <typename A, typename B, typename C> void host_elementwise(const A &a, const B &b, C &c, int op, coo_format)
{
    csr_matrix<typename C::index_type, typename C::value_type, host_memory> ca, cb, cc;
    cusp::convert(a, ca);
    cusp::convert(b, cb);
    host_elementwise(ca, cb, cc, op, csr_format());
    cusp::convert(cc, c);
}

template <typename A, typename B, typename C> void device_elementwise(const A &a, const B &b, C &c, int op, csr_format)
{
    typedef typename C::value_type V;
    static_assert(std::is_same<typename A::index_type, int>::value && std::is_same<typename B::index_type, int>::value && std::is_same<typename C::index_type, int>::value,
                  "cusp::elementwise on device_memory needs int indices");
    static_assert(std::is_same<typename A::value_type, V>::value && std::is_same<typename B::value_type, V>::value && (std::is_same<V, double>::value || std::is_same<V, float>::value),
                  "cusp::elementwise on device_memory: A, B and C must share one value type, float or double");
    const size_t cap = a.num_entries + b.num_entries;
    csr_matrix<int, V, device_memory> t(a.num_rows, a.num_cols, cap);
    int sorted = 0;
    check(by_type<V>(cmi_csr_elementwise_f64, cmi_csr_elementwise_f32)((int64_t)a.num_rows, (int64_t)a.num_cols, (int64_t)a.num_entries, a.row_offsets.data(),
                                                                       a.column_indices.data(), a.values.data(),
                        (int64_t)b.num_entries, b.row_offsets.data(), b.column_indices.data(), b.values.data(), op, t.row_offsets.data(), t.column_indices.data(),
                                                                       t.values.data(), (int64_t)cap, &sorted, nullptr));
    if (!sorted) { // an operand's rows are not sorted by column: the host path on host copies
        csr_matrix<int, V, host_memory> ha(a), hb(b), hc;
        host_elementwise(ha, hb, hc, op, csr_format());
        c = hc;
        return;
    }
    take_compacted(t, c);
}
template <typename A, typename B, typename C> void device_elementwise(const A &a, const B &b, C &c, int op, coo_format)
{
    csr_matrix<int, typename C::value_type, device_memory> ca, cb, cc;
    cusp::convert(a, ca);
    cusp::convert(b, cb);
    device_elementwise(ca, cb, cc, op, csr_format());
    cusp::convert(cc, c);
}

template <typename A, typename B, typename C> void elementwise_in_space(const A &a, const B &b, C &c, int op, host_memory) { host_elementwise(a, b, c, op, typename A::format()); }
template <typename A, typename B, typename C> void elementwise_in_space(const A &a, const B &b, C &c, int op, device_memory) { device_elementwise(a, b, c, op, typename A::format()); }

template <typename A, typename B, typename C> void elementwise_any(const A &a, const B &b, C &c, int op)
{
    typedef typename A::format F;
    static_assert(std::is_same<F, typename B::format>::value && std::is_same<F, typename C::format>::value &&
                      (std::is_same<F, csr_format>::value || std::is_same<F, coo_format>::value),
                  "cusp::add / subtract / elementwise are implemented for csr and coo matrices of one format: bring A, B and C to one of them with cusp::convert first");
    static_assert(std::is_same<typename A::memory_space, typename B::memory_space>::value && std::is_same<typename A::memory_space, typename C::memory_space>::value,
                  "cusp::add / subtract / elementwise: A, B and C must live in one memory space");
    if (a.num_rows != b.num_rows || a.num_cols != b.num_cols) throw cusp::invalid_input_exception("cusp::elementwise: matrix dimensions do not match");
    elementwise_in_space(a, b, c, op, typename C::memory_space());
}

} // namespace detail

template <typename A, typename B, typename C> void add(const A &a, const B &b, C &c) { detail::elementwise_any(a, b, c, 0); }
template <typename A, typename B, typename C> void subtract(const A &a, const B &b, C &c) { detail::elementwise_any(a, b, c, 1); }
template <typename A, typename B, typename C, typename Op> void elementwise(const A &a, const B &b, C &c, Op op) { detail::elementwise_any(a, b, c, detail::elementwise_op(op)); }

} // namespace cusp

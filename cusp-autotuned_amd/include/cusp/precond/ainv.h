// cusp/precond/ainv.h -- the approximate-inverse preconditioners of Bridson's outer-product form: scaled_bridson_ainv (z = W^T W r), bridson_ainv
// (z = W^T (d .* (W r))) and nonsym_bridson_ainv (z = W^T (d .* (Z r))), with a drop tolerance and / or the Lin-More bound on the entries per row
// (reference cusp/precond/ainv.h:51-178, detail/ainv.inl).
//
// Set-up runs on the host in both memory spaces, as in the reference, and is sequential: row j of the factor must be final before it updates the
// rows i > j.  It follows the reference's expressions and their rounding, because every dropping decision hangs on them:
//   u      = sum over the entries (k, w_jk) of factor row j, in index order, of A's row k times w_jk, scattered into an index-ordered map
//   p      = the merge dot product of factor row j with u                                   (nonsym: of W^T's row j with l = the same over A)
//   d_j    = (ValueType)(1.0 / p), the quotient formed in double                             (bridson, nonsym)
//   s      = 1.0 / sqrt((ValueType)p): the root in ValueType, the quotient in double, then u and row j times s   (scaled)
//   row i += (-u_i / p) row j  (scaled: -u_i), for the indices i > j of u in ascending order, term by term: a term with |term| < drop_tolerance is
//            skipped; a new index in a row that already holds row_count entries replaces the entry of smallest |value| unless the term is strictly
//            smaller than it (detail::ainv_matrix_row: an index-ordered map and a min-heap on |value| that point at each other).
// Then the rows go into a host CSR matrix in index order, that into hyb_matrix in MemorySpace, and w_t = cusp::transpose(w).
//
// Applying it on device_memory: bridson_ainv and nonsym_bridson_ainv own a SECOND plan for w (nonsym: z) that carries `diagonals` as its row scale
// (cmi_plan_set_row_scale), so that z = W^T (d .* (W r)) is two launches -- the scaled multiply and the multiply by w_t -- with the bits of the
// reference's three steps (multiply, blas::xmy, multiply).  The container's own plan is untouched: cusp::multiply(M.w, x, y) is W x.  Where the plan
// refuses the scale (a heavy COO part: two launches per multiply) or `row_scale_route` is false, the three steps run.  scaled_bridson_ainv has no
// diagonal: two planned multiplies.  host_memory: the reference's sequence.
//
// Departures from the reference:
//   * a zero (or NaN) pivot -- for scaled_bridson_ainv any pivot that is not positive -- throws cusp::invalid_input_exception naming the row, and so
//     does a matrix that is not square; the reference fills the factor with inf / NaN in silence;
//   * operator() is const (the temporaries are mutable), so that a const preconditioner can be applied;
//   * apply_dot(r, z, out, ws): the apply whose last multiply also leaves <z, r> in device memory (cusp::krylov::cg's fused branch);
//   * row_scale_route: a public switch between the two device routes (measurements and tests); it has no effect on the result's bits.
#pragma once
#include <cmath>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../array1d.h"
#include "../blas/blas.h"
#include "../csr_matrix.h"
#include "../exception.h"
#include "../hyb_matrix.h"
#include "../krylov/detail/multiply_dot.h"
#include "../linear_operator.h"
#include "../multiply.h"
#include "../transpose.h"

namespace cusp {
namespace precond {
namespace detail {

// One row of the factor while it is being built: the entries by index (a map) and by magnitude (a binary min-heap on |value|); a map entry knows
// its heap slot and a heap slot its map entry.  All comparisons are strict < on absolute values: ties decide which entry is dropped.
template <typename IndexType, typename ValueType> class ainv_matrix_row {
public:
    struct map_entry {
        ValueType value;
        int heapidx;
    };
    typedef std::map<IndexType, map_entry> map_type;
    typedef typename map_type::const_iterator const_iterator;

private:
    struct heap_entry {
        ValueType value;
        typename map_type::iterator mapiter;
    };
    map_type row_map;
    std::vector<heap_entry> row_heap;

    static bool less_abs(const ValueType &a, const ValueType &b) { return (a < 0 ? -a : a) < (b < 0 ? -b : b); }
    int slots() const { return (int)row_heap.size(); }
    void exchange(int i, int j)
    {
        std::swap(row_heap[i], row_heap[j]);
        row_heap[i].mapiter->second.heapidx = i;
        row_heap[j].mapiter->second.heapidx = j;
    }
    void sift_up(int i)
    {
        while (i != 0) {
            const int parent = (i - 1) / 2;
            if (!less_abs(row_heap[i].value, row_heap[parent].value)) break;
            exchange(i, parent);
            i = parent;
        }
    }
    // the smaller child is the first one unless the second is STRICTLY smaller; the node moves down while either child is strictly smaller than it
    void sift_down(int i)
    {
        for (;;) {
            const int c0 = 2 * i + 1, c1 = c0 + 1;
            if (c0 >= slots()) break;
            const bool has1 = c1 < slots();
            const int smaller = has1 && less_abs(row_heap[c1].value, row_heap[c0].value) ? c1 : c0;
            if (!(less_abs(row_heap[c0].value, row_heap[i].value) || (has1 && less_abs(row_heap[c1].value, row_heap[i].value)))) break;
            exchange(i, smaller);
            i = smaller;
        }
    }

public:
    const_iterator begin() const { return row_map.begin(); }
    const_iterator end() const { return row_map.end(); }
    size_t size() const { return row_map.size(); }
    bool has_entry_at_index(IndexType i) const { return row_map.count(i) != 0; }

    void mult_by_scalar(ValueType scalar)
    {
        for (heap_entry &h : row_heap) { // (the order of a uniform scaling's heap is kept)
            h.value *= scalar;
            h.mapiter->second.value *= scalar;
        }
    }
    // a new index (an index already present keeps its map entry, as std::map::insert does)
    void insert(IndexType i, ValueType t)
    {
        heap_entry h;
        h.value = t;
        h.mapiter = row_map.insert(std::make_pair(i, map_entry{t, -1})).first;
        row_heap.push_back(h);
        h.mapiter->second.heapidx = slots() - 1;
        sift_up(slots() - 1);
    }
    // the root's value (signed; 0 for an empty row)
    ValueType min_abs_value() const { return row_heap.empty() ? ValueType(0) : row_heap.front().value; }
    void add_to_value(IndexType i, ValueType addend)
    {
        typename map_type::iterator it = row_map.find(i);
        it->second.value += addend;
        const int slot = it->second.heapidx;
        const ValueType before = row_heap[slot].value;
        row_heap[slot].value = it->second.value;
        if (less_abs(it->second.value, before)) sift_up(slot); // strictly smaller in magnitude: towards the root; else away from it
        else sift_down(slot);
    }
    // the root changes places with the last slot, the heap shrinks, the new root sinks
    void remove_min()
    {
        if (row_heap.empty()) return;
        const typename map_type::iterator gone = row_heap.front().mapiter;
        exchange(0, slots() - 1);
        row_heap.pop_back();
        sift_down(0);
        row_map.erase(gone);
    }
    // (i, t) takes the place of the smallest entry unless t is strictly smaller than it
    void replace_min_if_greater(IndexType i, ValueType t)
    {
        if (less_abs(t, min_abs_value())) return;
        remove_min();
        insert(i, t);
    }
    // for tests: every parent strictly smaller than its children; map and heap point at each other and agree on the values
    bool validate_heap() const
    {
        for (int i = 0; i < slots(); i++)
            for (int c = 2 * i + 1; c <= 2 * i + 2; c++)
                if (c < slots() && !less_abs(row_heap[i].value, row_heap[c].value)) return false;
        return true;
    }
    bool validate_backpointers() const
    {
        for (const_iterator it = row_map.begin(); it != row_map.end(); ++it) {
            const heap_entry &h = row_heap[it->second.heapidx];
            if (const_iterator(h.mapiter) != it || h.value != it->second.value) return false;
        }
        return true;
    }
};

// b <- sum over the entries (k, x_k) of x, in index order, of A's row k times x_k; the first product of a column starts its sum
template <typename I, typename V, typename Csr> void ainv_scatter_rows(const Csr &A, const ainv_matrix_row<I, V> &x, std::map<I, V> &b)
{
    b.clear();
    for (typename ainv_matrix_row<I, V>::const_iterator it = x.begin(); it != x.end(); ++it) {
        const V xk = it->second.value;
        for (I e = A.row_offsets[it->first]; e < A.row_offsets[it->first + 1]; e++) {
            const V product = A.values[e] * xk;
            const std::pair<typename std::map<I, V>::iterator, bool> at = b.insert(std::make_pair((I)A.column_indices[e], product));
            if (!at.second) at.first->second += product;
        }
    }
}

// <a, b> over the indices both hold, in ascending order, from 0
template <typename I, typename V> V ainv_merge_dot(const ainv_matrix_row<I, V> &a, const std::map<I, V> &b)
{
    typename ainv_matrix_row<I, V>::const_iterator ia = a.begin();
    typename std::map<I, V>::const_iterator ib = b.begin();
    V sum = 0;
    while (ia != a.end() && ib != b.end()) {
        if (ia->first == ib->first) { sum += ia->second.value * ib->second; ++ia; ++ib; }
        else if (ia->first < ib->first) ++ia;
        else ++ib;
    }
    return sum;
}

// result += mult * operand term by term under the drop rule (the header's comment); row_count < 0: no bound
template <typename I, typename V> void ainv_add_row_dropping(ainv_matrix_row<I, V> &result, V mult, const ainv_matrix_row<I, V> &operand, V tolerance, int row_count)
{
    for (typename ainv_matrix_row<I, V>::const_iterator it = operand.begin(); it != operand.end(); ++it) {
        const V term = mult * it->second.value;
        if ((term < 0 ? -term : term) < tolerance) continue;
        if (result.has_entry_at_index(it->first)) result.add_to_value(it->first, term);
        else if (row_count < 0 || result.size() < (size_t)row_count) result.insert(it->first, term);
        else result.replace_min_if_greater(it->first, term);
    }
}

// the bound on the entries of factor row i
template <typename Csr> int ainv_row_count(const Csr &A, size_t i, int nonzero_per_row, bool lin_dropping, int lin_param)
{
    if (!lin_dropping) return nonzero_per_row;
    const int count = lin_param + (int)(A.row_offsets[i + 1] - A.row_offsets[i]);
    return count < 1 ? 1 : count;
}

template <typename I, typename V> std::vector<ainv_matrix_row<I, V>> ainv_identity_rows(size_t n)
{
    std::vector<ainv_matrix_row<I, V>> rows(n);
    for (size_t i = 0; i < n; i++) rows[i].insert((I)i, V(1));
    return rows;
}

template <typename Matrix> void ainv_require_square(const Matrix &A, const char *who)
{
    if (A.num_rows != A.num_cols) throw cusp::invalid_input_exception(std::string(who) + ": the matrix must be square");
}
[[noreturn]] inline void ainv_bad_pivot(const char *who, size_t row, const char *what)
{
    throw cusp::invalid_input_exception(std::string(who) + ": " + what + " pivot in row " + std::to_string(row));
}

// the rows, in index order, as a CSR matrix on the host and from there as a hyb_matrix in the target's memory space
template <typename I, typename VA, typename V, typename MemorySpace>
void ainv_rows_to_hyb(const std::vector<ainv_matrix_row<I, VA>> &rows, cusp::hyb_matrix<int, V, MemorySpace> &dst)
{
    size_t entries = 0;
    for (const ainv_matrix_row<I, VA> &r : rows) entries += r.size();
    cusp::csr_matrix<int, V, cusp::host_memory> csr(rows.size(), rows.size(), entries);
    size_t pos = 0;
    csr.row_offsets[0] = 0;
    for (size_t i = 0; i < rows.size(); i++) {
        for (typename ainv_matrix_row<I, VA>::const_iterator it = rows[i].begin(); it != rows[i].end(); ++it, ++pos) {
            csr.column_indices[pos] = (int)it->first;
            csr.values[pos] = (V)it->second.value;
        }
        csr.row_offsets[i + 1] = (int)pos;
    }
    dst = csr;
}

// The second plan of a device_memory factor: made with cmi_plan_create_hyb for the matrix's current arrays and given `scale` as its row scale.
// Re-made when the arrays or the scale have moved (a copied preconditioner gets its own); `refused`: the plan runs two launches and took no scale.
struct ainv_scaled_plan {
    std::shared_ptr<cmi_plan> plan;
    const void *index = nullptr, *scale = nullptr;
    size_t rows = 0, width = 0, coo = 0;
    bool refused = false;

    template <typename Hyb, typename Scale> const cmi_plan *get(const Hyb &m, const Scale &d)
    {
        const void *idx = m.coo.row_indices.data();
        const size_t w = m.ell.column_indices.num_cols, n = m.coo.num_entries;
        if (!(plan || refused) || idx != index || d.data() != scale || rows != m.num_rows || width != w || coo != n) {
            plan.reset();
            index = idx; scale = d.data(); rows = m.num_rows; width = w; coo = n;
            refused = m.ell.column_indices.pitch != m.ell.values.pitch || d.size() != m.num_rows || m.num_rows == 0;
            if (!refused) {
                cmi_plan *p = nullptr;
                cusp::detail::check(cmi_plan_create_hyb(cusp::detail::dtype_code<typename Hyb::value_type>::value, (int64_t)m.num_rows, (int64_t)m.num_cols, (int64_t)w, (int64_t)n,
                                                        m.coo.row_indices.data(), nullptr, nullptr, nullptr, &p));
                plan.reset(p, [](cmi_plan *q) { cmi_plan_destroy(q); });
                const int st = cmi_plan_set_row_scale(p, d.data());
                if (st == CMI_ERROR_NOT_SUPPORTED) { plan.reset(); refused = true; }
                else cusp::detail::check(st);
            }
        }
        return plan.get();
    }
};

// t <- d .* (m x): through the scaled plan in one launch (returns true), or not at all (false: the caller runs multiply and xmy)
template <typename Hyb, typename Scale, typename X, typename Y> bool ainv_scaled_multiply(ainv_scaled_plan &slot, const Hyb &m, const Scale &d, const X &x, Y &t, cusp::device_memory)
{
    typedef typename Hyb::value_type V;
    if constexpr (cusp::detail::is_real<V>::value && std::is_same<typename X::value_type, V>::value && std::is_same<typename Y::value_type, V>::value) {
        if (x.size() != m.num_cols || t.size() != m.num_rows) throw cusp::invalid_input_exception("ainv: vector sizes do not match the factor");
        const cmi_plan *p = slot.get(m, d);
        if (!p) return false;
        cusp::detail::check(cusp::detail::by_type<V>(cmi_spmv_hyb_plan_f64, cmi_spmv_hyb_plan_f32)(
            p, m.ell.column_indices.pitch, cusp::detail::data_of(m.ell.column_indices), cusp::detail::data_of(m.ell.values), m.coo.row_indices.data(), m.coo.column_indices.data(),
            m.coo.values.data(), x.data(), t.data(), 0, nullptr));
        return true;
    } else {
        return false;
    }
}
template <typename Hyb, typename Scale, typename X, typename Y> bool ainv_scaled_multiply(ainv_scaled_plan &, const Hyb &, const Scale &, const X &, Y &, cusp::host_memory) { return false; }

// z <- w_t t, and with `out` also *out <- <z, r> (a double in device memory) in the same launch where the format's kernel can
template <typename Hyb, typename T1, typename Z, typename R> void ainv_last_multiply(const Hyb &w_t, const T1 &t, Z &z, const R *r, double *out, void *ws)
{
    if (out) cusp::krylov::detail::multiply_dot(w_t, t, z, *r, out, ws);
    else cusp::multiply(w_t, t, z);
}

} // namespace detail

// z = W^T W r, the diagonal folded into the factor; SPD matrices only
template <typename ValueType, typename MemorySpace> class scaled_bridson_ainv : public cusp::linear_operator<ValueType, MemorySpace> {
    typedef cusp::linear_operator<ValueType, MemorySpace> Parent;

public:
    cusp::hyb_matrix<int, ValueType, MemorySpace> w;
    cusp::hyb_matrix<int, ValueType, MemorySpace> w_t;

    template <typename MatrixTypeA>
    scaled_bridson_ainv(const MatrixTypeA &A, ValueType drop_tolerance = 0.1, int nonzero_per_row = -1, bool lin_dropping = false, int lin_param = 1)
        : Parent(A.num_rows, A.num_cols, A.num_rows)
    {
        typedef typename MatrixTypeA::index_type I;
        typedef typename MatrixTypeA::value_type V;
        detail::ainv_require_square(A, "scaled_bridson_ainv");
        const size_t n = A.num_rows;
        temp1.resize(n);
        const cusp::csr_matrix<I, V, cusp::host_memory> host_A(A);
        std::vector<detail::ainv_matrix_row<I, V>> rows = detail::ainv_identity_rows<I, V>(n);
        std::map<I, V> u;
        for (size_t j = 0; j < n; j++) {
            detail::ainv_scatter_rows(host_A, rows[j], u);
            const V p = detail::ainv_merge_dot(rows[j], u);
            if (!(p > 0)) detail::ainv_bad_pivot("scaled_bridson_ainv", j, "a non-positive");
            const V s = (V)(1.0 / std::sqrt((ValueType)p));
            for (typename std::map<I, V>::iterator it = u.begin(); it != u.end(); ++it) it->second *= s;
            rows[j].mult_by_scalar(s);
            for (typename std::map<I, V>::const_iterator it = u.upper_bound((I)j); it != u.end(); ++it)
                detail::ainv_add_row_dropping(rows[it->first], (V)(-it->second), rows[j], (V)drop_tolerance,
                                              detail::ainv_row_count(host_A, (size_t)it->first, nonzero_per_row, lin_dropping, lin_param));
        }
        detail::ainv_rows_to_hyb(rows, w);
        cusp::transpose(w, w_t);
    }

    template <typename VectorType1, typename VectorType2> void operator()(const VectorType1 &x, VectorType2 &y) const { apply_dot(x, y, nullptr, nullptr); }
    // y <- W^T W x; with `out`, *out <- <y, x> as well (device_memory: the last multiply's fused dot)
    template <typename VectorType1, typename VectorType2> void apply_dot(const VectorType1 &x, VectorType2 &y, double *out, void *ws) const
    {
        cusp::multiply(w, x, temp1);
        detail::ainv_last_multiply(w_t, temp1, y, &x, out, ws);
    }

protected:
    mutable cusp::array1d<ValueType, MemorySpace> temp1;
};

// z = W^T (d .* (W r)); SPD matrices only
template <typename ValueType, typename MemorySpace> class bridson_ainv : public cusp::linear_operator<ValueType, MemorySpace> {
    typedef cusp::linear_operator<ValueType, MemorySpace> Parent;

public:
    cusp::hyb_matrix<int, ValueType, MemorySpace> w;
    cusp::hyb_matrix<int, ValueType, MemorySpace> w_t;
    cusp::array1d<ValueType, MemorySpace> diagonals;
    bool row_scale_route = true; // device_memory: d .* (W x) in the multiply's own launch where the plan takes the scale

    template <typename MatrixTypeA>
    bridson_ainv(const MatrixTypeA &A, ValueType drop_tolerance = 0.1, int nonzero_per_row = -1, bool lin_dropping = false, int lin_param = 1)
        : Parent(A.num_rows, A.num_cols, A.num_rows)
    {
        typedef typename MatrixTypeA::index_type I;
        typedef typename MatrixTypeA::value_type V;
        detail::ainv_require_square(A, "bridson_ainv");
        const size_t n = A.num_rows;
        temp1.resize(n);
        temp2.resize(n);
        const cusp::csr_matrix<I, V, cusp::host_memory> host_A(A);
        cusp::array1d<ValueType, cusp::host_memory> host_diagonals(n);
        std::vector<detail::ainv_matrix_row<I, V>> rows = detail::ainv_identity_rows<I, V>(n);
        std::map<I, V> u;
        for (size_t j = 0; j < n; j++) {
            detail::ainv_scatter_rows(host_A, rows[j], u);
            const V p = detail::ainv_merge_dot(rows[j], u);
            if (p == 0 || p != p) detail::ainv_bad_pivot("bridson_ainv", j, "a zero");
            host_diagonals[j] = (ValueType)(1.0 / p);
            for (typename std::map<I, V>::const_iterator it = u.upper_bound((I)j); it != u.end(); ++it)
                detail::ainv_add_row_dropping(rows[it->first], (V)(-it->second / p), rows[j], (V)drop_tolerance,
                                              detail::ainv_row_count(host_A, (size_t)it->first, nonzero_per_row, lin_dropping, lin_param));
        }
        diagonals = host_diagonals;
        detail::ainv_rows_to_hyb(rows, w);
        cusp::transpose(w, w_t);
    }

    template <typename VectorType1, typename VectorType2> void operator()(const VectorType1 &x, VectorType2 &y) const { apply_dot(x, y, nullptr, nullptr); }
    template <typename VectorType1, typename VectorType2> void apply_dot(const VectorType1 &x, VectorType2 &y, double *out, void *ws) const
    {
        if (row_scale_route && detail::ainv_scaled_multiply(scaled_, w, diagonals, x, temp1, MemorySpace())) {
            detail::ainv_last_multiply(w_t, temp1, y, &x, out, ws);
            return;
        }
        cusp::multiply(w, x, temp1);
        cusp::blas::xmy(temp1, diagonals, temp2);
        detail::ainv_last_multiply(w_t, temp2, y, &x, out, ws);
    }
    // does the apply run through the scaled plan?  (device_memory, after the first apply)
    bool row_scale_in_use() const { return row_scale_route && (bool)scaled_.plan; }

protected:
    mutable cusp::array1d<ValueType, MemorySpace> temp1;
    mutable cusp::array1d<ValueType, MemorySpace> temp2;
    mutable detail::ainv_scaled_plan scaled_;
};

// z = W^T (d .* (Z r)): the form for matrices that are not symmetric (on a symmetric matrix, bridson_ainv's factor twice over)
template <typename ValueType, typename MemorySpace> class nonsym_bridson_ainv : public cusp::linear_operator<ValueType, MemorySpace> {
    typedef cusp::linear_operator<ValueType, MemorySpace> Parent;

public:
    cusp::hyb_matrix<int, ValueType, MemorySpace> w_t;
    cusp::hyb_matrix<int, ValueType, MemorySpace> z;
    cusp::array1d<ValueType, MemorySpace> diagonals;
    bool row_scale_route = true;

    template <typename MatrixTypeA>
    nonsym_bridson_ainv(const MatrixTypeA &A, ValueType drop_tolerance = 0.1, int nonzero_per_row = -1, bool lin_dropping = false, int lin_param = 1)
        : Parent(A.num_rows, A.num_cols, A.num_rows)
    {
        typedef typename MatrixTypeA::index_type I;
        typedef typename MatrixTypeA::value_type V;
        detail::ainv_require_square(A, "nonsym_bridson_ainv");
        const size_t n = A.num_rows;
        temp1.resize(n);
        temp2.resize(n);
        const cusp::csr_matrix<I, V, cusp::host_memory> host_A(A);
        cusp::csr_matrix<I, V, cusp::host_memory> host_At;
        cusp::transpose(host_A, host_At);
        cusp::array1d<ValueType, cusp::host_memory> host_diagonals(n);
        std::vector<detail::ainv_matrix_row<I, V>> wt_rows = detail::ainv_identity_rows<I, V>(n), z_rows = detail::ainv_identity_rows<I, V>(n);
        std::map<I, V> u, l;
        for (size_t j = 0; j < n; j++) {
            detail::ainv_scatter_rows(host_At, wt_rows[j], u);
            detail::ainv_scatter_rows(host_A, z_rows[j], l);
            const V p = detail::ainv_merge_dot(wt_rows[j], l);
            if (p == 0 || p != p) detail::ainv_bad_pivot("nonsym_bridson_ainv", j, "a zero");
            host_diagonals[j] = (ValueType)(1.0 / p);
            for (typename std::map<I, V>::const_iterator it = u.upper_bound((I)j); it != u.end(); ++it)
                detail::ainv_add_row_dropping(z_rows[it->first], (V)(-it->second / p), z_rows[j], (V)drop_tolerance,
                                              detail::ainv_row_count(host_A, (size_t)it->first, nonzero_per_row, lin_dropping, lin_param));
            for (typename std::map<I, V>::const_iterator it = l.upper_bound((I)j); it != l.end(); ++it)
                detail::ainv_add_row_dropping(wt_rows[it->first], (V)(-it->second / p), wt_rows[j], (V)drop_tolerance,
                                              detail::ainv_row_count(host_A, (size_t)it->first, nonzero_per_row, lin_dropping, lin_param));
        }
        diagonals = host_diagonals;
        cusp::hyb_matrix<int, ValueType, MemorySpace> w;
        detail::ainv_rows_to_hyb(wt_rows, w);
        cusp::transpose(w, w_t);
        detail::ainv_rows_to_hyb(z_rows, z);
    }

    template <typename VectorType1, typename VectorType2> void operator()(const VectorType1 &x, VectorType2 &y) const { apply_dot(x, y, nullptr, nullptr); }
    template <typename VectorType1, typename VectorType2> void apply_dot(const VectorType1 &x, VectorType2 &y, double *out, void *ws) const
    {
        if (row_scale_route && detail::ainv_scaled_multiply(scaled_, z, diagonals, x, temp1, MemorySpace())) {
            detail::ainv_last_multiply(w_t, temp1, y, &x, out, ws);
            return;
        }
        cusp::multiply(z, x, temp1);
        cusp::blas::xmy(temp1, diagonals, temp2);
        detail::ainv_last_multiply(w_t, temp2, y, &x, out, ws);
    }
    bool row_scale_in_use() const { return row_scale_route && (bool)scaled_.plan; }

protected:
    mutable cusp::array1d<ValueType, MemorySpace> temp1;
    mutable cusp::array1d<ValueType, MemorySpace> temp2;
    mutable detail::ainv_scaled_plan scaled_;
};

} // namespace precond
} // namespace cusp

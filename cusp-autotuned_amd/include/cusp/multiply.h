// cusp/multiply.h -- cusp::multiply(A, x, y): the drop-in boundary of the SpMV hot path.
//
// Reference: cusp/multiply.h:40,101,113,190 (the four overloads), cusp/detail/multiply.inl:27-105
// (memory-space dispatch), cusp/system/detail/generic/multiply.inl:98-111,173-191 (format dispatch).
//
//   host_memory   : the reference's sequential loops, restated (sequential/multiply/{csr,coo,ell,dia,
//                   hyb}_spmv.h) -- same summation order, fully generic in (initialize, combine, reduce).
//   device_memory : forwards to the MI355X C-ABI (cmi_spmv_{csr,coo,ell,dia,hyb}_{f64,f32}): hand-written
//                   gfx950 kernels, launch shape from the persisted tuning table.  NEVER falls back to the
//                   host: a functor combination the kernels do not implement throws
//                   cusp::not_implemented_exception.  combine = multiplies, reduce = plus with
//                   initialize = constant_functor(0) (y = A x) or identity_function (y = y + A x) -- the
//                   combinations the reference's own multiply / hyb path use -- run the plans and tuned kernels.
//                   Every other combination of the NAMED functors of cusp/functional.h (combine: plus,
//                   multiplies, minimum, maximum, project1st, project2nd; reduce: the first four; initialize:
//                   identity_function or constant_functor of any value) runs the semiring kernels
//                   (cmi_spmv_*_semiring_*): one chain per row in the format's own order, the host loops' bits;
//                   HYB in two launches; a coo_matrix (and HYB's COO part) must be sorted by row --
//                   cusp::not_implemented_exception naming sort_by_row() otherwise.  A functor type the library
//                   does not know (a user's struct) throws.
//
// x and y may be any contiguous vector type of the matrix's memory space with data()/size():
// cusp::array1d, cusp::array1d_view, or a solver's temporary (the reference's CG passes
// temporary_array, which the fork's KTT hook fails to match -- SURVEY.md 3.3; here every vector type
// reaches the tuned kernels).
//
// Dense blocks (SpMM): multiply(A, X, Y) with cusp::array2d X (num_cols x k) and Y (num_rows x k) and a CSR matrix or view
// computes Y = A X column by column (reference csr_block_spmv.h; dispatch on X's format, section "dense blocks" below):
//   host_memory   : the reference's sequential loop (sequential/multiply/csr_block_spmv.h), generic in the functors;
//                   cusp::omp::par splits the rows over threads with the same per-row arithmetic.
//   device_memory : cmi_spmm_csr_{f64,f32} with the strides of each array2d's orientation and pitch; a one-column block
//                   with a contiguous column runs the container's planned SpMV (the reference forwards k == 1 the same
//                   way, cuda/detail/multiply/csr_block_spmv.h:198-201).
// Other sparse formats with an array2d X, and mixed array1d / array2d arguments, are compile-time errors.
//
// Sparse products (SpGEMM): multiply(A, B, C) with three sparse matrices computes C = A B and resizes C (reference
// generalized_spgemm; section "sparse x sparse" below).  csr x csr -> csr and coo x coo -> coo; every other combination is a
// compile-time error naming cusp::convert.  Structure: one entry per (i, c) with a structural product, every row's columns ascending.
// Values: s = 0; the products of the entry in expansion order (A's row in storage order, then B's row in storage order):
// s = s + a * b -- the chain of sequential/multiply/csr_spgemm.h:102-131.
//   host_memory   : that loop, generic in (combine, reduce); entries whose sum compares equal to zero are DROPPED, as the reference
//                   drops them, and each row's columns are sorted (the reference leaves them in reverse first-touch order).
//   device_memory : cmi_spgemm_csr_{f64,f32}; exact-zero sums are KEPT, as the reference's device path keeps them: the host
//                   result is the device result with its zeros removed, bit for bit.  COO operands are converted to CSR on the
//                   device (stable sort by row, row offsets) and the product back.  Standard functors only.
//
// Execution policies: multiply(exec, A, x, y) with cusp::hip::par.on(stream) selects the stream.  A
// user-derived policy reaches a user-provided multiply overload by ADL without being copied
// (testing/multiply.cu:792-858): see cusp/execution_policy.h.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>
#include "array1d.h"
#include "array2d.h"
#include "convert.h"
#include "execution_policy.h"
#include "functional.h"

namespace cusp {

namespace detail {

// ---- host loops (reference sequential backend) ---------------------------------------------------
template <typename A, typename X, typename Y, typename Init, typename Comb, typename Red>
void host_multiply(const A &a, const X &x, Y &y, Init initialize, Comb combine, Red reduce, csr_format)
{
    typedef typename A::index_type I;
    typedef typename Y::value_type V;
    for (size_t i = 0; i < a.num_rows; i++) { // sequential/multiply/csr_spmv.h:56-72
        V acc = initialize(y[i]);
        for (I jj = a.row_offsets[i]; jj < a.row_offsets[i + 1]; jj++) acc = reduce(acc, combine(a.values[jj], x[a.column_indices[jj]]));
        y[i] = acc;
    }
}

template <typename A, typename X, typename Y, typename Init, typename Comb, typename Red>
void host_multiply(const A &a, const X &x, Y &y, Init initialize, Comb combine, Red reduce, coo_format)
{
    for (size_t i = 0; i < a.num_rows; i++) y[i] = initialize(y[i]); // coo_spmv.h:56-67
    for (size_t n = 0; n < a.num_entries; n++) {
        const auto i = a.row_indices[n];
        y[i] = reduce(y[i], combine(a.values[n], x[a.column_indices[n]]));
    }
}

template <typename A, typename X, typename Y, typename Init, typename Comb, typename Red>
void host_multiply(const A &a, const X &x, Y &y, Init initialize, Comb combine, Red reduce, ell_format)
{
    typedef typename A::index_type I;
    const size_t width = a.column_indices.num_cols, pitch = a.column_indices.pitch;
    const I *cj = a.column_indices.data_ptr();
    const auto *va = a.values.data_ptr();
    for (size_t i = 0; i < a.num_rows; i++) y[i] = initialize(y[i]); // ell_spmv.h:59-74
    for (size_t n = 0; n < width; n++)
        for (size_t i = 0; i < a.num_rows; i++) {
            const I j = cj[n * pitch + i];
            if (j != I(-1)) y[i] = reduce(y[i], combine(va[n * pitch + i], x[j]));
        }
}

template <typename A, typename X, typename Y, typename Init, typename Comb, typename Red>
void host_multiply(const A &a, const X &x, Y &y, Init initialize, Comb combine, Red reduce, dia_format)
{
    typedef typename A::index_type I;
    const size_t nd = a.values.num_cols, pitch = a.values.pitch;
    const auto *va = a.values.data_ptr();
    for (size_t i = 0; i < a.num_rows; i++) y[i] = initialize(y[i]); // dia_spmv.h:61-80
    for (size_t d = 0; d < nd; d++) {
        const I k = a.diagonal_offsets[d];
        const size_t i_start = std::max<I>(0, -k), j_start = std::max<I>(0, k);
        if (i_start >= a.num_rows || j_start >= a.num_cols) continue;
        const size_t N = std::min(a.num_rows - i_start, a.num_cols - j_start);
        for (size_t n = 0; n < N; n++) y[i_start + n] = reduce(y[i_start + n], combine(va[d * pitch + i_start + n], x[j_start + n]));
    }
}

template <typename A, typename X, typename Y, typename Init, typename Comb, typename Red>
void host_multiply(const A &a, const X &x, Y &y, Init initialize, Comb combine, Red reduce, hyb_format)
{
    typedef typename Y::value_type V;
    host_multiply(a.ell, x, y, initialize, combine, reduce, ell_format()); // hyb_spmv.h:55-56
    host_multiply(a.coo, x, y, identity_function<V>(), combine, reduce, coo_format());
}

// dense matrix-vector product on the host (the reference tests' ground truth, array2d_mv.h)
template <typename A, typename X, typename Y, typename Init, typename Comb, typename Red>
void host_multiply(const A &a, const X &x, Y &y, Init initialize, Comb combine, Red reduce, array2d_format)
{
    typedef typename Y::value_type V;
    for (size_t i = 0; i < a.num_rows; i++) {
        V acc = initialize(y[i]);
        for (size_t j = 0; j < a.num_cols; j++) acc = reduce(acc, combine(a(i, j), x[j]));
        y[i] = acc;
    }
}

// uniform access to the raw 2-D storage of containers and views
template <typename T, typename M, typename O> const T *data_of(const array2d<T, M, O> &a) { return a.values.data(); }
template <typename V2> auto data_of(const V2 &v) -> decltype(v.data()) { return v.data(); }

// ---- device dispatch: which accumulate flag does (initialize, combine, reduce) mean? -------------
template <typename V, typename Init, typename Comb, typename Red> struct device_functors {
    static int accumulate(const Init &)
    {
        throw cusp::not_implemented_exception("cusp::multiply on device_memory implements combine = multiplies, reduce = plus, "
                                              "initialize = constant_functor(0) or identity_function; other functors are host-only");
    }
};
template <typename V> struct device_functors<V, constant_functor<V>, multiplies<V>, plus<V>> {
    static int accumulate(const constant_functor<V> &f)
    {
        if (!(f.value == V(0))) throw cusp::not_implemented_exception("cusp::multiply on device_memory: initialize must be constant 0 or identity");
        return 0;
    }
};
template <typename V> struct device_functors<V, identity_function<V>, multiplies<V>, plus<V>> {
    static int accumulate(const identity_function<V> &) { return 1; }
};

// explicit launch configuration for cusp::ktt::tune (thread-local; nullptr = tuning table)
inline const cmi_config *&forced_config() { static thread_local const cmi_config *c = nullptr; return c; }

// the container's plan (views, and anything while cusp::ktt::tune forces a configuration: none)
template <typename A> auto plan_of(const A &a, void *stream, int) -> decltype(a.plan(stream))
{
    return (forced_config() || a.num_entries == 0) ? nullptr : a.plan(stream);
}
template <typename A> const cmi_plan *plan_of(const A &, void *, long) { return nullptr; }

template <typename A> void require_int_index()
{
    static_assert(std::is_same<typename A::index_type, int>::value, "device_memory matrices use 32-bit int indices (the reference's default IndexType)");
}

// optional ELLR row lengths
template <typename A> auto row_lengths_of(const A &a, int) -> decltype(a.row_lengths.data()) { return a.row_lengths.size() ? a.row_lengths.data() : nullptr; }
template <typename A> const int *row_lengths_of(const A &, long) { return nullptr; }

template <typename A, typename X, typename Y> void device_multiply(const A &a, const X &x, Y &y, int acc, void *stream, csr_format)
{
    require_int_index<A>();
    typedef typename A::value_type V;
    if (const cmi_plan *p = plan_of(a, stream, 0)) {
        check(by_type<V>(cmi_spmv_csr_plan_f64, cmi_spmv_csr_plan_f32)(p, a.row_offsets.data(), a.column_indices.data(), a.values.data(), x.data(), y.data(), acc, stream));
        return;
    }
    check(by_type<V>(cmi_spmv_csr_f64, cmi_spmv_csr_f32)(a.num_rows, a.num_cols, a.num_entries, a.row_offsets.data(), a.column_indices.data(), a.values.data(), x.data(),
                                                         y.data(), acc, forced_config(), stream));
}
template <typename A, typename X, typename Y> void device_multiply(const A &a, const X &x, Y &y, int acc, void *stream, coo_format)
{
    require_int_index<A>();
    typedef typename A::value_type V;
    if (const cmi_plan *p = plan_of(a, stream, 0)) {
        check(by_type<V>(cmi_spmv_coo_plan_f64, cmi_spmv_coo_plan_f32)(p, a.row_indices.data(), a.column_indices.data(), a.values.data(), x.data(), y.data(), acc, stream));
        return;
    }
    check(by_type<V>(cmi_spmv_coo_f64, cmi_spmv_coo_f32)(a.num_rows, a.num_cols, a.num_entries, a.row_indices.data(), a.column_indices.data(), a.values.data(), x.data(),
                                                         y.data(), acc, forced_config(), stream));
}
template <typename A, typename X, typename Y> void device_multiply(const A &a, const X &x, Y &y, int acc, void *stream, ell_format)
{
    require_int_index<A>();
    // reference ell_spmv.h:138 asserts equal pitches; here it is an error the caller sees
    if (a.column_indices.pitch != a.values.pitch) throw cusp::invalid_input_exception("ell_matrix: column_indices.pitch != values.pitch");
    check(by_type<typename A::value_type>(cmi_spmv_ell_f64, cmi_spmv_ell_f32)(a.num_rows, a.num_cols, a.column_indices.num_cols, a.column_indices.pitch, data_of(a.column_indices),
                                                                              data_of(a.values), row_lengths_of(a, 0), x.data(), y.data(), acc, forced_config(), stream));
}
template <typename A, typename X, typename Y> void device_multiply(const A &a, const X &x, Y &y, int acc, void *stream, dia_format)
{
    require_int_index<A>();
    check(by_type<typename A::value_type>(cmi_spmv_dia_f64, cmi_spmv_dia_f32)(a.num_rows, a.num_cols, a.values.num_cols, a.values.pitch, a.diagonal_offsets.data(),
                                                                              data_of(a.values),
                                                                              x.data(), y.data(), acc, forced_config(), stream));
}
template <typename A, typename X, typename Y> void device_multiply(const A &a, const X &x, Y &y, int acc, void *stream, hyb_format)
{
    require_int_index<A>();
    typedef typename A::value_type V;
    if (a.ell.column_indices.pitch != a.ell.values.pitch) throw cusp::invalid_input_exception("hyb_matrix: ell.column_indices.pitch != ell.values.pitch");
    if (const cmi_plan *p = plan_of(a, stream, 0)) { // COO part sorted by row (every conversion's output): one launch, y written once
        check(by_type<V>(cmi_spmv_hyb_plan_f64, cmi_spmv_hyb_plan_f32)(p, a.ell.column_indices.pitch, data_of(a.ell.column_indices), data_of(a.ell.values),
                                                                       a.coo.row_indices.data(),
                                                                       a.coo.column_indices.data(), a.coo.values.data(), x.data(), y.data(), acc, stream));
        return;
    }
    check(by_type<V>(cmi_spmv_hyb_f64, cmi_spmv_hyb_f32)(a.num_rows, a.num_cols, a.ell.column_indices.num_cols, a.ell.column_indices.pitch, data_of(a.ell.column_indices),
                                                         data_of(a.ell.values), a.coo.num_entries, a.coo.row_indices.data(), a.coo.column_indices.data(), a.coo.values.data(),
                                                         x.data(), y.data(), acc, nullptr, nullptr, stream)); // (no configuration for either part: the tuning table's)
}

// ---- device dispatch of the NAMED functors (the semiring multiply, cmi_spmv_*_semiring_*) ---------------------------
// functor type -> cmi_op; -1: a type the library does not know (a user's struct), which the device route refuses
template <typename V, typename F> struct semiring_op : std::integral_constant<int, -1> {};
template <typename V> struct semiring_op<V, plus<V>> : std::integral_constant<int, CMI_OP_PLUS> {};
template <typename V> struct semiring_op<V, multiplies<V>> : std::integral_constant<int, CMI_OP_MULTIPLIES> {};
template <typename V> struct semiring_op<V, minimum<V>> : std::integral_constant<int, CMI_OP_MINIMUM> {};
template <typename V> struct semiring_op<V, maximum<V>> : std::integral_constant<int, CMI_OP_MAXIMUM> {};
template <typename V> struct semiring_op<V, project1st<V>> : std::integral_constant<int, CMI_OP_PROJECT1ST> {};
template <typename V> struct semiring_op<V, project2nd<V>> : std::integral_constant<int, CMI_OP_PROJECT2ND> {};
// initialize -> (does the chain start from y[i]?, the constant it starts from otherwise)
template <typename V, typename I> struct semiring_init : std::false_type {};
template <typename V> struct semiring_init<V, identity_function<V>> : std::true_type {
    static bool from_y(const identity_function<V> &) { return true; }
    static V constant(const identity_function<V> &) { return V(0); }
};
template <typename V> struct semiring_init<V, constant_functor<V>> : std::true_type {
    static bool from_y(const constant_functor<V> &) { return false; }
    static V constant(const constant_functor<V> &f) { return f.value; }
};
// a (combine, reduce) pair the semiring kernels run: any named combine, a named reduce that is no projection
template <typename V, typename C, typename R> struct semiring_pair
    : std::integral_constant<bool, (semiring_op<V, C>::value >= 0) && (semiring_op<V, R>::value >= 0) && (semiring_op<V, R>::value <= CMI_OP_MAXIMUM)> {};
// ... and the one pair that has tuned kernels and plans of its own
template <typename V, typename C, typename R> struct arithmetic_pair
    : std::integral_constant<bool, std::is_same<C, multiplies<V>>::value && std::is_same<R, plus<V>>::value> {};

template <typename A> void require_row_sorted(const A &coo, void *stream)
{
    if (coo.num_entries == 0) return;
    int sorted = 0;
    check(cmi_coo_is_sorted((int64_t)coo.num_rows, (int64_t)coo.num_entries, coo.row_indices.data(), nullptr, 0, &sorted, stream));
    if (!sorted)
        throw cusp::not_implemented_exception("cusp::multiply on device_memory with these functors needs a coo_matrix whose entries are sorted by row: call sort_by_row() first");
}

// y[i] = the chain of row i started from y0[i] (y0 != nullptr) or from `init`; the operands of cmi_spmv_*_semiring_*
template <typename A, typename X, typename V, typename Y> void device_semiring(const A &a, const X &x, const V *y0, V init, int comb, int red, Y &y, void *stream, csr_format)
{
    check(by_type<V>(cmi_spmv_csr_semiring_f64, cmi_spmv_csr_semiring_f32)(a.num_rows, a.num_cols, a.num_entries, a.row_offsets.data(), a.column_indices.data(), a.values.data(),
                                                                           x.data(), y0, init, comb, red, y.data(), stream));
}
template <typename A, typename X, typename V, typename Y> void device_semiring_sorted_coo(const A &a, const X &x, const V *y0, V init, int comb, int red, Y &y, void *stream)
{
    check(by_type<V>(cmi_spmv_coo_semiring_f64, cmi_spmv_coo_semiring_f32)(a.num_rows, a.num_cols, a.num_entries, a.row_indices.data(), a.column_indices.data(), a.values.data(),
                                                                           x.data(), y0, init, comb, red, y.data(), stream));
}
template <typename A, typename X, typename V, typename Y> void device_semiring(const A &a, const X &x, const V *y0, V init, int comb, int red, Y &y, void *stream, coo_format)
{
    require_row_sorted(a, stream);
    device_semiring_sorted_coo(a, x, y0, init, comb, red, y, stream);
}
template <typename A, typename X, typename V, typename Y> void device_semiring(const A &a, const X &x, const V *y0, V init, int comb, int red, Y &y, void *stream, ell_format)
{
    if (a.column_indices.pitch != a.values.pitch) throw cusp::invalid_input_exception("ell_matrix: column_indices.pitch != values.pitch");
    check(by_type<V>(cmi_spmv_ell_semiring_f64, cmi_spmv_ell_semiring_f32)(a.num_rows, a.num_cols, a.column_indices.num_cols, a.column_indices.pitch, data_of(a.column_indices),
                                                                           data_of(a.values), x.data(), y0, init, comb, red, y.data(), stream));
}
template <typename A, typename X, typename V, typename Y> void device_semiring(const A &a, const X &x, const V *y0, V init, int comb, int red, Y &y, void *stream, dia_format)
{
    check(by_type<V>(cmi_spmv_dia_semiring_f64, cmi_spmv_dia_semiring_f32)(a.num_rows, a.num_cols, a.values.num_cols, a.values.pitch, a.diagonal_offsets.data(), data_of(a.values),
                                                                           x.data(), y0, init, comb, red, y.data(), stream));
}
// HYB: the ELL part with the caller's start, then the COO part on top of what the first call left (hyb_spmv.h:55-56): two launches
template <typename A, typename X, typename V, typename Y> void device_semiring(const A &a, const X &x, const V *y0, V init, int comb, int red, Y &y, void *stream, hyb_format)
{
    require_row_sorted(a.coo, stream);
    device_semiring(a.ell, x, y0, init, comb, red, y, stream, ell_format());
    device_semiring_sorted_coo(a.coo, x, static_cast<const V *>(y.data()), V(0), comb, red, y, stream);
}
template <typename A, typename X, typename Y, typename I, typename C, typename R>
void device_semiring_multiply(const A &a, const X &x, Y &y, const I &init, void *stream)
{
    require_int_index<A>();
    typedef typename Y::value_type V;
    static_assert(std::is_same<typename A::value_type, V>::value, "cusp::multiply on device_memory: the matrix and y must have the same value type");
    const V *y0 = semiring_init<V, I>::from_y(init) ? static_cast<const V *>(y.data()) : nullptr;
    device_semiring(a, x, y0, semiring_init<V, I>::constant(init), semiring_op<V, C>::value, semiring_op<V, R>::value, y, stream, typename A::format());
}

// host adaptor: containers expose operator[] / data; give ELL/DIA a data_ptr() view for the loops
template <typename M> struct host_ell_adaptor {
    const M &m;
    size_t num_rows, num_cols, num_entries;
    struct arr_i { const typename M::index_type *p; size_t num_cols, pitch; const typename M::index_type *data_ptr() const { return p; } } column_indices;
    struct arr_v { const typename M::value_type *p; size_t num_cols, pitch; const typename M::value_type *data_ptr() const { return p; } } values;
    typedef typename M::index_type index_type;
    explicit host_ell_adaptor(const M &mm)
        : m(mm), num_rows(mm.num_rows), num_cols(mm.num_cols), num_entries(mm.num_entries),
          column_indices{data_of(mm.column_indices), mm.column_indices.num_cols, mm.column_indices.pitch},
          values{data_of(mm.values), mm.values.num_cols, mm.values.pitch} {}
};
template <typename M> struct host_dia_adaptor {
    size_t num_rows, num_cols, num_entries;
    decltype(std::declval<const M &>().diagonal_offsets) const &diagonal_offsets;
    struct arr_v { const typename M::value_type *p; size_t num_cols, pitch; const typename M::value_type *data_ptr() const { return p; } } values;
    typedef typename M::index_type index_type;
    explicit host_dia_adaptor(const M &mm)
        : num_rows(mm.num_rows), num_cols(mm.num_cols), num_entries(mm.num_entries), diagonal_offsets(mm.diagonal_offsets),
          values{data_of(mm.values), mm.values.num_cols, mm.values.pitch} {}
};
template <typename M> struct host_hyb_adaptor {
    size_t num_rows, num_cols, num_entries;
    host_ell_adaptor<decltype(std::declval<const M &>().ell)> ell;
    decltype(std::declval<const M &>().coo) const &coo;
    explicit host_hyb_adaptor(const M &mm) : num_rows(mm.num_rows), num_cols(mm.num_cols), num_entries(mm.num_entries), ell(mm.ell), coo(mm.coo) {}
};

template <typename A, typename X, typename Y, typename I, typename C, typename R, typename F>
void host_dispatch(const A &a, const X &x, Y &y, I i, C c, R r, F f) { host_multiply(a, x, y, i, c, r, f); }
template <typename A, typename X, typename Y, typename I, typename C, typename R>
void host_dispatch(const A &a, const X &x, Y &y, I i, C c, R r, ell_format) { host_multiply(host_ell_adaptor<A>(a), x, y, i, c, r, ell_format()); }
template <typename A, typename X, typename Y, typename I, typename C, typename R>
void host_dispatch(const A &a, const X &x, Y &y, I i, C c, R r, dia_format) { host_multiply(host_dia_adaptor<A>(a), x, y, i, c, r, dia_format()); }
template <typename A, typename X, typename Y, typename I, typename C, typename R>
void host_dispatch(const A &a, const X &x, Y &y, I i, C c, R r, hyb_format) { host_multiply(host_hyb_adaptor<A>(a), x, y, i, c, r, hyb_format()); }

template <typename A, typename X, typename Y> void check_shapes(const A &a, const X &x, const Y &y)
{
    // reference: cusp::invalid_input_exception on mismatched dimensions
    if (x.size() != a.num_cols || y.size() != a.num_rows) throw cusp::invalid_input_exception("cusp::multiply: vector sizes do not match the matrix shape");
}

template <typename A, typename X, typename Y, typename I, typename C, typename R>
void multiply_in_space(const A &a, const X &x, Y &y, I init, C comb, R red, void * /*stream*/, host_memory)
{
    host_dispatch(a, x, y, init, comb, red, typename A::format());
}
template <typename A, typename X, typename Y, typename I, typename C, typename R>
void multiply_in_space(const A &a, const X &x, Y &y, I init, C comb, R red, void *stream, device_memory)
{
    typedef typename Y::value_type V;
    if constexpr (semiring_pair<V, C, R>::value && semiring_init<V, I>::value) {
        // (constant 0 | identity, multiplies, plus): the plans and tuned kernels, as ever.  Every other named combination -- a constant other
        // than zero among them -- runs the semiring kernels: one chain per row, in the format's own order.
        const bool tuned = arithmetic_pair<V, C, R>::value && (semiring_init<V, I>::from_y(init) || semiring_init<V, I>::constant(init) == V(0));
        if (!tuned) {
            device_semiring_multiply<A, X, Y, I, C, R>(a, x, y, init, stream);
            return;
        }
    }
    const int acc = device_functors<V, I, C, R>::accumulate(init);
    device_multiply(a, x, y, acc, stream, typename A::format());
}

// ---- dense blocks: Y = A X with array2d X and Y (SpMM) ------------------------------------------------------
template <typename T, typename = void> struct is_block : std::false_type {};
template <typename T> struct is_block<T, typename std::enable_if<std::is_same<typename T::format, array2d_format>::value>::type> : std::true_type {};

// (row stride, column stride) of an array2d in elements: row-major (pitch, 1), column-major (1, pitch)
template <typename T, typename M> void strides_of(const array2d<T, M, row_major> &a, int64_t *rs, int64_t *cs) { *rs = (int64_t)a.pitch; *cs = 1; }
template <typename T, typename M> void strides_of(const array2d<T, M, column_major> &a, int64_t *rs, int64_t *cs) { *rs = 1; *cs = (int64_t)a.pitch; }

template <typename A, typename X, typename Y> void check_block_shapes(const A &a, const X &x, const Y &y)
{
    if (x.num_rows != a.num_cols || y.num_rows != a.num_rows || x.num_cols != y.num_cols)
        throw cusp::invalid_input_exception("cusp::multiply: array2d shapes do not match (X must be num_cols x k, Y num_rows x k)");
}

template <typename A> void require_csr_for_blocks()
{
    static_assert(std::is_same<typename A::format, csr_format>::value,
                  "cusp::multiply(A, X, Y) with array2d X and Y is implemented for CSR matrices only: convert A to a csr_matrix with cusp::convert first");
}

// sequential/multiply/csr_block_spmv.h: per row, one accumulator per column, the row's entries in storage order.  `parallel`:
// rows split over OpenMP threads (cusp::omp::par), the same per-row arithmetic.
template <typename A, typename X, typename Y, typename Init, typename Comb, typename Red>
void host_block_multiply(const A &a, const X &x, Y &y, Init initialize, Comb combine, Red reduce, bool parallel)
{
    typedef typename A::index_type I;
    typedef typename Y::value_type V;
    const long long n = static_cast<long long>(a.num_rows);
    const size_t k = x.num_cols;
#if defined(_OPENMP)
#pragma omp parallel for if (parallel)
#endif
    for (long long i = 0; i < n; i++) {
        std::vector<V> acc(k);
        for (size_t c = 0; c < k; c++) acc[c] = initialize(y(i, c));
        for (I jj = a.row_offsets[i]; jj < a.row_offsets[i + 1]; jj++) {
            const I j = a.column_indices[jj];
            const V aij = a.values[jj];
            for (size_t c = 0; c < k; c++) acc[c] = reduce(acc[c], combine(aij, x(j, c)));
        }
        for (size_t c = 0; c < k; c++) y(i, c) = acc[c];
    }
    (void)parallel;
}

// a contiguous device column as the vector device_multiply takes
template <typename T> struct column_ref {
    T *p;
    T *data() const { return p; }
};

template <typename A, typename X, typename Y> void device_block_multiply(const A &a, const X &x, Y &y, int acc, void *stream)
{
    require_int_index<A>();
    typedef typename Y::value_type V;
    int64_t xrs, xcs, yrs, ycs;
    strides_of(x, &xrs, &xcs);
    strides_of(y, &yrs, &ycs);
    if (x.num_cols == 1 && (xrs == 1 || x.num_rows <= 1) && (yrs == 1 || y.num_rows <= 1)) { // one contiguous column: the planned SpMV
        const column_ref<const V> xc{data_of(x)};
        column_ref<V> yc{const_cast<V *>(data_of(y))};
        device_multiply(a, xc, yc, acc, stream, csr_format());
        return;
    }
    check(by_type<V>(cmi_spmm_csr_f64, cmi_spmm_csr_f32)(a.num_rows, a.num_cols, a.num_entries, a.row_offsets.data(), a.column_indices.data(), a.values.data(), (int64_t)x.num_cols,
                                                         data_of(x), xrs, xcs, const_cast<V *>(data_of(y)), yrs, ycs, acc, forced_config(), stream));
}

// ---- sparse x sparse: C = A B with three sparse matrices (SpGEMM) ---------------------------------------------
template <typename T, typename = void> struct is_sparse : std::false_type {};
template <typename T> struct is_sparse<T, typename std::enable_if<std::is_base_of<sparse_format, typename T::format>::value>::type> : std::true_type {};
struct sparse_product {}; // the third route tag beside std::false_type (vectors) and std::true_type (dense blocks)

template <typename A, typename B, typename C> void require_spgemm_formats()
{
    typedef typename A::format FA;
    static_assert(std::is_same<FA, typename B::format>::value && std::is_same<FA, typename C::format>::value &&
                      (std::is_same<FA, csr_format>::value || std::is_same<FA, coo_format>::value),
                  "cusp::multiply(A, B, C) with three sparse matrices is implemented for csr x csr -> csr and coo x coo -> coo only: bring A, B and C "
                  "to one of these formats with cusp::convert first");
}

template <typename A, typename B> void check_product_shapes(const A &a, const B &b)
{
    if (a.num_cols != b.num_rows) throw cusp::invalid_input_exception("cusp::multiply: A.num_cols != B.num_rows in the sparse product C = A B");
}

// sequential/multiply/csr_spgemm.h:102-131 restated: one dense accumulator per column of B, reset after every row; a row's touched
// columns are then SORTED (the reference emits them in reverse first-touch order) and sums that compare equal to zero are dropped.
// `initialize` is not applied, as in the reference: every chain starts at V(0).
template <typename A, typename B, typename C, typename Comb, typename Red>
void host_spgemm(const A &a, const B &b, C &c, Comb combine, Red reduce, csr_format)
{
    typedef typename C::index_type I;
    typedef typename C::value_type V;
    std::vector<V> sums(b.num_cols, V(0)), Cx;
    std::vector<char> seen(b.num_cols, 0);
    std::vector<I> touched, Cp(a.num_rows + 1, I(0)), Cj;
    for (size_t i = 0; i < a.num_rows; i++) {
        touched.clear();
        for (auto jj = a.row_offsets[i]; jj < a.row_offsets[i + 1]; jj++) {
            const auto j = a.column_indices[jj];
            const V v = a.values[jj];
            for (auto kk = b.row_offsets[j]; kk < b.row_offsets[j + 1]; kk++) {
                const I col = b.column_indices[kk];
                sums[col] = reduce(sums[col], combine(v, V(b.values[kk])));
                if (!seen[col]) {
                    seen[col] = 1;
                    touched.push_back(col);
                }
            }
        }
        std::sort(touched.begin(), touched.end());
        for (const I col : touched) {
            if (sums[col] != V(0)) {
                Cj.push_back(col);
                Cx.push_back(sums[col]);
            }
            sums[col] = V(0);
            seen[col] = 0;
        }
        Cp[i + 1] = static_cast<I>(Cj.size());
    }
    c.resize(a.num_rows, b.num_cols, Cj.size()); // (after the loops: C may be A or B)
    for (size_t i = 0; i <= c.num_rows; i++) c.row_offsets[i] = Cp[i];
    for (size_t q = 0; q < Cj.size(); q++) {
        c.column_indices[q] = Cj[q];
        c.values[q] = Cx[q];
    }
}
// COO: entries in any order -> CSR (stable by row: the chains are those of the storage order), the loop above, and back
template <typename A, typename B, typename C, typename Comb, typename Red>
void host_spgemm(const A &a, const B &b, C &c, Comb combine, Red reduce, coo_format)
{
    csr_matrix<typename A::index_type, typename A::value_type, host_memory> ca, cb, cc;
    cusp::convert(a, ca);
    cusp::convert(b, cb);
    host_spgemm(ca, cb, cc, combine, reduce, csr_format());
    cusp::convert(cc, c);
}

template <typename A, typename B, typename C> void device_spgemm(const A &a, const B &b, C &c, void *stream, csr_format)
{
    require_int_index<A>();
    require_int_index<B>();
    require_int_index<C>();
    static_assert(std::is_same<typename A::value_type, typename B::value_type>::value && std::is_same<typename A::value_type, typename C::value_type>::value,
                  "cusp::multiply(A, B, C) on device_memory: A, B and C must have the same value type");
    struct handle { // the product lives in the library until it has been copied into C
        cmi_spgemm *p = nullptr;
        ~handle() { cmi_spgemm_destroy(p); }
    } h;
    typedef typename A::value_type V;
    check(by_type<V>(cmi_spgemm_csr_f64, cmi_spgemm_csr_f32)((int64_t)a.num_rows, (int64_t)a.num_cols, (int64_t)b.num_cols, (int64_t)a.num_entries, a.row_offsets.data(),
                                                             a.column_indices.data(),
                                                             a.values.data(), (int64_t)b.num_entries, b.row_offsets.data(), b.column_indices.data(), b.values.data(), &h.p, stream));
    int64_t entries = 0;
    check(cmi_spgemm_num_entries(h.p, &entries));
    c.resize(a.num_rows, b.num_cols, (size_t)entries); // (A and B have been read: C may be one of them)
    check(by_type<V>(cmi_spgemm_take_f64, cmi_spgemm_take_f32)(h.p, c.row_offsets.data(), c.column_indices.data(), c.values.data(), entries, stream));
    check(cmi_stream_synchronize(stream)); // the copies read the handle's arrays
}
// COO on the device: the existing device conversions around the CSR product (stable sort by row + row offsets in, row indices out)
template <typename A, typename B, typename C> void device_spgemm(const A &a, const B &b, C &c, void *stream, coo_format)
{
    csr_matrix<int, typename A::value_type, device_memory> ca, cb, cc;
    cusp::convert(a, ca);
    cusp::convert(b, cb);
    device_spgemm(ca, cb, cc, stream, csr_format());
    cusp::convert(cc, c);
}


// the route every public overload takes: vectors -> the SpMV paths above, unchanged; array2d blocks -> SpMM
template <typename X, typename Y> struct block_route {
    static_assert(is_block<X>::value == is_block<Y>::value,
                  "cusp::multiply: x and y must both be vectors (array1d) or both be dense blocks (array2d); mixed array1d / array2d arguments are not supported");
    typedef std::integral_constant<bool, is_block<X>::value> type;
};
// ... and two sparse matrices in the places of x and y -> the sparse product
template <typename X, typename Y, bool Sparse = is_sparse<X>::value || is_sparse<Y>::value> struct operand_route : block_route<X, Y> {};
template <typename X, typename Y> struct operand_route<X, Y, true> {
    static_assert(is_sparse<X>::value && is_sparse<Y>::value,
                  "cusp::multiply(A, B, C): B and C must both be sparse matrices (C = A B); a sparse matrix cannot stand for a vector or a dense block");
    typedef sparse_product type;
};

template <typename A, typename X, typename Y, typename I, typename C, typename R, typename Space>
void multiply_route(const A &a, const X &x, Y &y, I init, C comb, R red, void *stream, Space, std::false_type)
{
    check_shapes(a, x, y);
    multiply_in_space(a, x, y, init, comb, red, stream, Space());
}
template <typename A, typename X, typename Y, typename I, typename C, typename R>
void multiply_route(const A &a, const X &x, Y &y, I init, C comb, R red, void *, host_memory, std::true_type)
{
    require_csr_for_blocks<A>();
    check_block_shapes(a, x, y);
    host_block_multiply(a, x, y, init, comb, red, false);
}
template <typename A, typename X, typename Y, typename I, typename C, typename R>
void multiply_route(const A &a, const X &x, Y &y, I init, C comb, R red, void *stream, device_memory, std::true_type)
{
    require_csr_for_blocks<A>();
    check_block_shapes(a, x, y);
    typedef typename Y::value_type V;
    const int acc = device_functors<V, I, C, R>::accumulate(init);
    if (a.num_rows == 0 || x.num_cols == 0) return;
    device_block_multiply(a, x, y, acc, stream);
}
template <typename A, typename B, typename C, typename I, typename Comb, typename R>
void multiply_route(const A &a, const B &b, C &c, I, Comb comb, R red, void *, host_memory, sparse_product)
{
    require_spgemm_formats<A, B, C>();
    check_product_shapes(a, b);
    host_spgemm(a, b, c, comb, red, typename A::format());
}
template <typename A, typename B, typename C, typename I, typename Comb, typename R>
void multiply_route(const A &a, const B &b, C &c, I init, Comb, R, void *stream, device_memory, sparse_product)
{
    require_spgemm_formats<A, B, C>();
    check_product_shapes(a, b);
    (void)device_functors<typename C::value_type, I, Comb, R>::accumulate(init); // plus / multiplies or cusp::not_implemented_exception
    device_spgemm(a, b, c, stream, typename A::format());
}

} // namespace detail

// ---- public overloads (reference cusp/multiply.h:40,101,113,190) ----------------------------------

// y = A*x with explicit functors: y[i] = reduce(initialize(y[i]), ... combine(A_ij, x_j))
template <typename LinearOperator, typename Vector1, typename Vector2, typename UnaryFunction, typename BinaryFunction1, typename BinaryFunction2,
          typename = typename std::enable_if<detail::has_format<LinearOperator>::value>::type>
void multiply(const LinearOperator &A, const Vector1 &x, Vector2 &y, UnaryFunction initialize, BinaryFunction1 combine, BinaryFunction2 reduce)
{
    static_assert(std::is_same<typename LinearOperator::memory_space, typename Vector2::memory_space>::value &&
                      std::is_same<typename Vector1::memory_space, typename Vector2::memory_space>::value,
                  "cusp::multiply: A, x and y must live in the same memory space");
    detail::multiply_route(A, x, y, initialize, combine, reduce, nullptr, typename LinearOperator::memory_space(),
                           typename detail::operand_route<Vector1, Vector2>::type());
}

// y = A*x (initialize = 0, combine = *, reduce = +: generic/multiply.inl:104-110)
template <typename LinearOperator, typename Vector1, typename Vector2, typename = typename std::enable_if<detail::has_format<LinearOperator>::value>::type>
void multiply(const LinearOperator &A, const Vector1 &x, Vector2 &y)
{
    typedef typename Vector2::value_type V;
    cusp::multiply(A, x, y, constant_functor<V>(V(0)), multiplies<V>(), plus<V>());
}
// an operator WITHOUT a storage format -- cusp::linear_operator's children: identity_operator, precond::diagonal, a user's matrix-free operator --
// is applied through its own operator()(x, y) (reference cusp/detail/multiply.inl: the unknown_format branch calls A(x, y)).  Excluded:
// execution policies (the policy-first overloads below) and the sharded operator of cusp/distributed/multiply.h, which has its own overload.
template <typename LinearOperator, typename Vector1, typename Vector2,
          typename = typename std::enable_if<!detail::has_format<LinearOperator>::value && !std::is_base_of<cusp::execution_policy<LinearOperator>, LinearOperator>::value>::type,
          typename = decltype(std::declval<const LinearOperator &>()(std::declval<const Vector1 &>(), std::declval<Vector2 &>()))>
void multiply(const LinearOperator &A, const Vector1 &x, Vector2 &y)
{
    A(x, y);
}
// views are cheap handles and are often passed as temporaries
template <typename LinearOperator, typename Vector1, typename T, typename M, typename = typename std::enable_if<detail::has_format<LinearOperator>::value>::type>
void multiply(const LinearOperator &A, const Vector1 &x, array1d_view<T, M> &&y)
{
    cusp::multiply(A, x, y);
}

// with the library's execution policy: selects the HIP stream (device) / is ignored (host)
template <typename LinearOperator, typename Vector1, typename Vector2, typename UnaryFunction, typename BinaryFunction1, typename BinaryFunction2>
void multiply(const cusp::hip::execution_policy &exec, const LinearOperator &A, const Vector1 &x, Vector2 &y, UnaryFunction initialize,
              BinaryFunction1 combine, BinaryFunction2 reduce)
{
    detail::multiply_route(A, x, y, initialize, combine, reduce, exec.stream(), typename LinearOperator::memory_space(),
                           typename detail::operand_route<Vector1, Vector2>::type());
}
template <typename LinearOperator, typename Vector1, typename Vector2>
void multiply(const cusp::hip::execution_policy &exec, const LinearOperator &A, const Vector1 &x, Vector2 &y)
{
    typedef typename Vector2::value_type V;
    cusp::multiply(exec, A, x, y, constant_functor<V>(V(0)), multiplies<V>(), plus<V>());
}

// cusp::omp::par: the reference's OpenMP host backend.  CSR: cusp/system/omp/detail/multiply/csr_spmv.h:51-86 -- rows split
// over the threads (#pragma omp parallel for, :67), per-row arithmetic the sequential kernel's (so the result is
// bit-identical to the sequential multiply); every other format: the sequential loops (omp/detail/multiply.h:26-40).
namespace detail {
template <typename A, typename X, typename Y, typename Init, typename Comb, typename Red>
void omp_multiply(const A &a, const X &x, Y &y, Init initialize, Comb combine, Red reduce, csr_format)
{
    typedef typename A::index_type I;
    typedef typename Y::value_type V;
    const long long n = static_cast<long long>(a.num_rows);
#if defined(_OPENMP)
#pragma omp parallel for
#endif
    for (long long i = 0; i < n; i++) {
        V acc = initialize(y[i]);
        for (I jj = a.row_offsets[i]; jj < a.row_offsets[i + 1]; jj++) acc = reduce(acc, combine(a.values[jj], x[a.column_indices[jj]]));
        y[i] = acc;
    }
}
template <typename A, typename X, typename Y, typename Init, typename Comb, typename Red, typename F>
void omp_multiply(const A &a, const X &x, Y &y, Init i, Comb c, Red r, F f) { host_dispatch(a, x, y, i, c, r, f); }

template <typename A, typename X, typename Y, typename Init, typename Comb, typename Red>
void omp_route(const A &a, const X &x, Y &y, Init i, Comb c, Red r, std::false_type)
{
    check_shapes(a, x, y);
    omp_multiply(a, x, y, i, c, r, typename A::format());
}
template <typename A, typename X, typename Y, typename Init, typename Comb, typename Red>
void omp_route(const A &a, const X &x, Y &y, Init i, Comb c, Red r, std::true_type)
{
    require_csr_for_blocks<A>();
    check_block_shapes(a, x, y);
    host_block_multiply(a, x, y, i, c, r, true);
}
template <typename A, typename B, typename C, typename Init, typename Comb, typename Red>
void omp_route(const A &a, const B &b, C &c, Init, Comb comb, Red red, sparse_product) // (the sequential loop: the reference's omp backend has no SpGEMM of its own)
{
    require_spgemm_formats<A, B, C>();
    check_product_shapes(a, b);
    host_spgemm(a, b, c, comb, red, typename A::format());
}
} // namespace detail

template <typename LinearOperator, typename Vector1, typename Vector2, typename UnaryFunction, typename BinaryFunction1, typename BinaryFunction2>
void multiply(const cusp::omp::execution_policy &, const LinearOperator &A, const Vector1 &x, Vector2 &y, UnaryFunction initialize,
              BinaryFunction1 combine, BinaryFunction2 reduce)
{
    static_assert(std::is_same<typename LinearOperator::memory_space, host_memory>::value, "cusp::omp::par runs on host_memory containers");
    detail::omp_route(A, x, y, initialize, combine, reduce, typename detail::operand_route<Vector1, Vector2>::type());
}
template <typename LinearOperator, typename Vector1, typename Vector2>
void multiply(const cusp::omp::execution_policy &exec, const LinearOperator &A, const Vector1 &x, Vector2 &y)
{
    typedef typename Vector2::value_type V;
    cusp::multiply(exec, A, x, y, constant_functor<V>(V(0)), multiplies<V>(), plus<V>());
}

// z = y + A*x (reference cusp/multiply.h:301,377 generalized_spmv with combine = *, reduce = +)
// device_memory vectors with a named pair other than (multiplies, plus): row i's chain starts from y[i] and is stored to z[i] by the semiring
// kernels, without a copy of y.  (multiplies, plus) keeps the copy and the tuned kernels.
namespace detail {
template <typename A, typename X, typename Z, typename C, typename R, typename = void> struct semiring_generalized : std::false_type {};
template <typename A, typename X, typename Z, typename C, typename R>
struct semiring_generalized<A, X, Z, C, R, typename std::enable_if<has_format<A>::value && std::is_same<typename Z::memory_space, device_memory>::value>::type>
    : std::integral_constant<bool, semiring_pair<typename Z::value_type, C, R>::value && !arithmetic_pair<typename Z::value_type, C, R>::value && !is_block<X>::value &&
                                       !is_sparse<X>::value && !is_block<Z>::value && !is_sparse<Z>::value> {};
} // namespace detail
template <typename LinearOperator, typename Vector1, typename Vector2, typename Vector3, typename BinaryFunction1, typename BinaryFunction2>
void generalized_spmv(const LinearOperator &A, const Vector1 &x, const Vector2 &y, Vector3 &z, BinaryFunction1 combine, BinaryFunction2 reduce)
{
    typedef typename Vector3::value_type V;
    if constexpr (detail::semiring_generalized<LinearOperator, Vector1, Vector3, BinaryFunction1, BinaryFunction2>::value) {
        static_assert(std::is_same<typename LinearOperator::memory_space, device_memory>::value && std::is_same<typename Vector1::memory_space, device_memory>::value &&
                          std::is_same<typename Vector2::memory_space, device_memory>::value && std::is_same<typename Vector2::value_type, V>::value &&
                          std::is_same<typename LinearOperator::value_type, V>::value,
                      "cusp::generalized_spmv: A, x, y and z must live in the same memory space and have the same value type");
        detail::require_int_index<LinearOperator>();
        detail::check_shapes(A, x, z);
        if (y.size() != z.size()) throw cusp::invalid_input_exception("cusp::generalized_spmv: y and z differ in length");
        if (A.num_rows == 0) return;
        detail::device_semiring(A, x, static_cast<const V *>(y.data()), V(0), detail::semiring_op<V, BinaryFunction1>::value, detail::semiring_op<V, BinaryFunction2>::value, z,
                                nullptr, typename LinearOperator::format());
    } else {
        if (static_cast<const void *>(y.data()) != static_cast<const void *>(z.data())) cusp::copy_array(y, z);
        cusp::multiply(A, x, z, identity_function<V>(), combine, reduce);
    }
}

} // namespace cusp

// ---- user-derived execution policies ---------------------------------------------------------------
namespace cusp {
namespace detail {
namespace policy_default {
// what a policy without its own multiply overload gets: the memory-space dispatch above
template <typename Derived, typename LinearOperator, typename Vector1, typename Vector2,
          typename = typename std::enable_if<std::is_base_of<cusp::execution_policy<Derived>, Derived>::value>::type>
void multiply(Derived &, const LinearOperator &A, const Vector1 &x, Vector2 &y)
{
    cusp::multiply(A, x, y);
}
} // namespace policy_default
} // namespace detail

// cusp::multiply(exec, A, x, y) for any policy derived from cusp::execution_policy<Derived>
// (reference cusp/detail/multiply.inl:27-39): unqualified call with the DERIVED policy, by reference.
template <typename Derived, typename LinearOperator, typename Vector1, typename Vector2>
void multiply(const cusp::execution_policy<Derived> &exec, const LinearOperator &A, const Vector1 &x, Vector2 &y)
{
    using cusp::detail::policy_default::multiply;
    multiply(const_cast<Derived &>(exec.derived()), A, x, y);
}

} // namespace cusp

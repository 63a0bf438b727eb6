// cusp/relaxation/gauss_seidel.h -- cusp::relaxation::gauss_seidel<ValueType, MemorySpace>: multicolour Gauss-Seidel
// sweeps on a CSR matrix (reference cusp/relaxation/gauss_seidel.h, detail/gauss_seidel.inl).
//
// The constructor colours A (cusp/graph/vertex_coloring.h), orders the rows by colour -- ascending row index inside a
// colour -- and keeps the colours' offsets into that ordering.  A sweep visits the colours in turn (FORWARD 0 .. C-1,
// BACKWARD C-1 .. 0, the rows inside a colour always ascending; SYMMETRIC = FORWARD then BACKWARD) and relaxes every row
// i of the colour (reference sequential/relaxation/gauss_seidel.h):
//   rsum = 0; over row i in storage order: an entry in column i sets diag (the last one wins) and adds nothing, any other
//   entry does rsum = rsum + A(i,j) * x[j]; if (diag != 0) x[i] = (b[i] - rsum) / diag, otherwise x[i] stays.
//
//   host_memory   : that loop.
//   device_memory : one cmi_csr_gauss_seidel_colour_* call per colour (one lane-ordered chain per row: the host loop's bits).
//
// The greedy colouring looks at a row's own entries only, so on a pattern that is not symmetric a row may hold a column
// j of its own colour; j is then always the larger index, which the host loop visits later: every row of a colour reads
// the x from before the colour.  The constructor finds those colours on the host (`color_conflicts`); on the device they
// take the call's two-launch form through `scratch` (new values parked, then stored), which gives exactly that -- where
// the reference's device kernel reads x[j] while another lane writes it.  Colours without such a row take one launch.
#pragma once
#include <algorithm>
#include <type_traits>
#include <vector>

#include "../blas/blas.h"
#include "../format_utils.h"
#include "../graph/vertex_coloring.h"
#include "../linear_operator.h"

namespace cusp {
namespace relaxation {

typedef enum { FORWARD, BACKWARD, SYMMETRIC } sweep;

template <typename ValueType, typename MemorySpace> class gauss_seidel : public cusp::linear_operator<ValueType, MemorySpace> {
    typedef cusp::linear_operator<ValueType, MemorySpace> Parent;

public:
    cusp::array1d<int, MemorySpace> ordering;              // the rows sorted by colour, ascending inside a colour
    cusp::array1d<int, cusp::host_memory> color_offsets;   // colour c owns ordering[color_offsets[c] .. color_offsets[c + 1])
    cusp::array1d<ValueType, MemorySpace> diagonal;
    sweep default_direction;
    cusp::array1d<int, cusp::host_memory> color_conflicts; // 1: some row of the colour holds an off-diagonal column of that colour
    cusp::array1d<ValueType, MemorySpace> scratch;         // as long as the largest such colour

    gauss_seidel() : default_direction(SYMMETRIC) {}

    template <typename MatrixType>
    gauss_seidel(const MatrixType &A, sweep default_direction = SYMMETRIC,
                 typename std::enable_if<std::is_convertible<typename MatrixType::format, cusp::csr_format>::value>::type * = 0)
        : Parent(A.num_rows, A.num_cols, A.num_entries), default_direction(default_direction)
    {
        const size_t n = A.num_rows;
        cusp::array1d<int, cusp::host_memory> colors(n);
        const size_t num_colors = cusp::graph::vertex_coloring(A, colors);

        cusp::array1d<int, cusp::host_memory> order(n);
        for (size_t i = 0; i < n; i++) order[i] = static_cast<int>(i);
        std::stable_sort(order.begin(), order.end(), [&](int p, int q) { return colors[p] < colors[q]; });
        color_offsets.assign(num_colors + 1, 0);
        for (size_t i = 0; i < n; i++) color_offsets[colors[i] + 1]++;
        for (size_t c = 0; c < num_colors; c++) color_offsets[c + 1] += color_offsets[c];
        ordering = order;

        cusp::extract_diagonal(A, diagonal);

        // which colours hold a row with an off-diagonal column of its own colour, and the longest of them
        cusp::array1d<typename MatrixType::index_type, cusp::host_memory> Ap(A.row_offsets), Aj(A.column_indices);
        color_conflicts.assign(num_colors, 0);
        for (size_t i = 0; i < n; i++)
            for (auto jj = Ap[i]; jj < Ap[i + 1]; jj++)
                if (static_cast<size_t>(Aj[jj]) != i && colors[Aj[jj]] == colors[i]) color_conflicts[colors[i]] = 1;
        size_t longest = 0;
        for (size_t c = 0; c < num_colors; c++)
            if (color_conflicts[c]) longest = std::max(longest, static_cast<size_t>(color_offsets[c + 1] - color_offsets[c]));
        scratch.resize(longest);
    }

    template <typename MemorySpace2>
    gauss_seidel(const gauss_seidel<ValueType, MemorySpace2> &o)
        : Parent(o.num_rows, o.num_cols, o.num_entries), ordering(o.ordering), color_offsets(o.color_offsets), diagonal(o.diagonal),
          default_direction(o.default_direction), color_conflicts(o.color_conflicts), scratch(o.scratch.size())
    {
    }

    // one sweep in the constructor's direction
    template <typename MatrixType, typename VectorType1, typename VectorType2> void operator()(const MatrixType &A, const VectorType1 &b, VectorType2 &x)
    {
        (*this)(A, b, x, default_direction);
    }

    // one sweep in the given direction
    template <typename MatrixType, typename VectorType1, typename VectorType2>
    void operator()(const MatrixType &A, const VectorType1 &b, VectorType2 &x, sweep direction)
    {
        static_assert(std::is_convertible<typename MatrixType::format, cusp::csr_format>::value, "cusp::relaxation::gauss_seidel runs on CSR matrices");
        if (A.num_rows != A.num_cols || b.size() != A.num_rows || x.size() != A.num_rows || ordering.size() != A.num_rows)
            throw cusp::invalid_input_exception("cusp::relaxation::gauss_seidel: A must be the square matrix this object was made from, b and x of its size");
        const size_t num_colors = color_offsets.size() ? color_offsets.size() - 1 : 0;
        if (direction == FORWARD) {
            for (size_t c = 0; c < num_colors; c++) colour(A, b, x, c, MemorySpace());
        } else if (direction == BACKWARD) {
            for (size_t c = num_colors; c > 0; c--) colour(A, b, x, c - 1, MemorySpace());
        } else if (direction == SYMMETRIC) {
            (*this)(A, b, x, FORWARD);
            (*this)(A, b, x, BACKWARD);
        } else {
            throw cusp::runtime_exception("Unknown Gauss-Seidel sweep direction specified.");
        }
    }

private:
    template <typename MatrixType, typename VectorType1, typename VectorType2>
    void colour(const MatrixType &A, const VectorType1 &b, VectorType2 &x, size_t c, cusp::host_memory)
    {
        typedef typename MatrixType::index_type I;
        for (int s = color_offsets[c]; s < color_offsets[c + 1]; s++) {
            const I i = ordering[s];
            ValueType rsum = ValueType(0), diag = ValueType(0);
            for (I jj = A.row_offsets[i]; jj < A.row_offsets[i + 1]; jj++) {
                const I j = A.column_indices[jj];
                if (j == i) diag = A.values[jj];
                else {
                    const ValueType p = A.values[jj] * x[j];
                    rsum = rsum + p;
                }
            }
            if (diag != ValueType(0)) x[i] = (b[i] - rsum) / diag;
        }
    }
    template <typename MatrixType, typename VectorType1, typename VectorType2>
    void colour(const MatrixType &A, const VectorType1 &b, VectorType2 &x, size_t c, cusp::device_memory)
    {
        static_assert(std::is_same<ValueType, double>::value || std::is_same<ValueType, float>::value,
                      "device_memory cusp::relaxation::gauss_seidel is implemented for float and double");
        static_assert(std::is_same<typename MatrixType::index_type, int>::value, "device_memory cusp::relaxation::gauss_seidel needs int indices");
        const size_t len = static_cast<size_t>(color_offsets[c + 1] - color_offsets[c]);
        ValueType *park = nullptr;
        if (color_conflicts[c]) {
            if (scratch.size() < len) scratch.resize(len);
            park = scratch.data();
        }
        cusp::detail::check(cusp::detail::by_type<ValueType>(cmi_csr_gauss_seidel_colour_f64, cmi_csr_gauss_seidel_colour_f32)(
            (int64_t)A.num_rows, (int64_t)A.num_entries, A.row_offsets.data(), A.column_indices.data(),
                                                A.values.data(), b.data(), x.data(), ordering.data(), color_offsets[c], color_offsets[c + 1], park, nullptr));
    }
};

} // namespace relaxation
} // namespace cusp

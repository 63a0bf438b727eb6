// Shared by the semiring test programs: a deck file written by tests/test_semiring_host.py (one matrix in CSR form with a DIA layout and a HYB
// split, x, y0 and a list of cases) is run through cusp::multiply / cusp::generalized_spmv in a memory space, every case printed as one line
// of hexadecimal floats.  The five formats are laid out by hand exactly as tests/semiring_refs.py lays them out (ELL and HYB pitch: rows
// rounded up to 16; DIA: the file's offsets and pitch; HYB: the first `width` entries of a row in the ELL part), so the Python loops restate
// the very arrays the library sees.
//
// File: `T rows cols nnz width ndiag dia_pitch`, then Ap, Aj, Ax, x, y0, the diagonal offsets, the number of cases and per case
// `format combine reduce start`: format csr / coo / ell / dia / hyb, or g:<format> for generalized_spmv(A, x, y0, z); start "y0" (identity) or
// a constant in hexadecimal.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include <cusp/array1d.h>
#include <cusp/coo_matrix.h>
#include <cusp/csr_matrix.h>
#include <cusp/dia_matrix.h>
#include <cusp/ell_matrix.h>
#include <cusp/functional.h>
#include <cusp/gallery/poisson.h>
#include <cusp/hyb_matrix.h>
#include <cusp/multiply.h>

#include "unittest.h"

namespace semiring_check {

typedef cusp::host_memory Host;

template <typename T> struct deck {
    size_t rows = 0, cols = 0, nnz = 0, width = 0, ndiag = 0, dia_pitch = 0;
    std::vector<int> Ap, Aj, offsets;
    std::vector<T> Ax, x, y0;
    struct one { std::string format, combine, reduce, start; };
    std::vector<one> cases;
};

template <typename T> void read_deck(std::istream &in, deck<T> &d)
{
    in >> d.rows >> d.cols >> d.nnz >> d.width >> d.ndiag >> d.dia_pitch;
    auto ints = [&](std::vector<int> &v, size_t n) { v.resize(n); for (auto &e : v) in >> e; };
    auto reals = [&](std::vector<T> &v, size_t n) { v.resize(n); std::string s; for (auto &e : v) { in >> s; e = (T)std::strtod(s.c_str(), nullptr); } };
    ints(d.Ap, d.rows + 1);
    ints(d.Aj, d.nnz);
    reals(d.Ax, d.nnz);
    reals(d.x, d.cols);
    reals(d.y0, d.rows);
    ints(d.offsets, d.ndiag);
    size_t n = 0;
    in >> n;
    d.cases.resize(n);
    for (auto &c : d.cases) in >> c.format >> c.combine >> c.reduce >> c.start;
}

// ---- the five formats on the host, laid out as tests/semiring_refs.py does ----------------------------------------------------------
template <typename T> cusp::csr_matrix<int, T, Host> make_csr(const deck<T> &d)
{
    cusp::csr_matrix<int, T, Host> A(d.rows, d.cols, d.nnz);
    for (size_t i = 0; i <= d.rows; i++) A.row_offsets[i] = d.Ap[i];
    for (size_t e = 0; e < d.nnz; e++) { A.column_indices[e] = d.Aj[e]; A.values[e] = d.Ax[e]; }
    return A;
}
// entries [first, first + count) of every row into a COO matrix, row by row
template <typename T> cusp::coo_matrix<int, T, Host> make_coo(const deck<T> &d, size_t skip = 0)
{
    size_t n = 0;
    for (size_t i = 0; i < d.rows; i++) n += (size_t)(d.Ap[i + 1] - d.Ap[i]) > skip ? (size_t)(d.Ap[i + 1] - d.Ap[i]) - skip : 0;
    cusp::coo_matrix<int, T, Host> A(d.rows, d.cols, n);
    size_t at = 0;
    for (size_t i = 0; i < d.rows; i++)
        for (size_t e = (size_t)d.Ap[i] + skip; e < (size_t)d.Ap[i + 1]; e++, at++) { A.row_indices[at] = (int)i; A.column_indices[at] = d.Aj[e]; A.values[at] = d.Ax[e]; }
    return A;
}
template <typename T> void fill_ell(const deck<T> &d, size_t width, cusp::ell_matrix<int, T, Host> &A)
{
    for (size_t i = 0; i < d.rows; i++)
        for (size_t n = 0; n < width; n++) {
            const size_t e = (size_t)d.Ap[i] + n;
            const bool there = e < (size_t)d.Ap[i + 1];
            A.column_indices(i, n) = there ? d.Aj[e] : -1;
            A.values(i, n) = there ? d.Ax[e] : T(0);
        }
}
template <typename T> cusp::ell_matrix<int, T, Host> make_ell(const deck<T> &d)
{
    size_t width = 0;
    for (size_t i = 0; i < d.rows; i++) width = std::max(width, (size_t)(d.Ap[i + 1] - d.Ap[i]));
    cusp::ell_matrix<int, T, Host> A(d.rows, d.cols, d.nnz, width, 16);
    fill_ell(d, width, A);
    return A;
}
template <typename T> cusp::hyb_matrix<int, T, Host> make_hyb(const deck<T> &d)
{
    cusp::hyb_matrix<int, T, Host> A;
    A.coo = make_coo(d, d.width);
    A.resize(d.rows, d.cols, d.nnz - A.coo.num_entries, A.coo.num_entries, d.width, 16);
    A.coo = make_coo(d, d.width);
    fill_ell(d, d.width, A.ell);
    return A;
}
template <typename T> cusp::dia_matrix<int, T, Host> make_dia(const deck<T> &d)
{
    cusp::dia_matrix<int, T, Host> A(d.rows, d.cols, d.nnz, d.ndiag, d.dia_pitch ? d.dia_pitch : 1);
    for (size_t k = 0; k < d.ndiag; k++) {
        A.diagonal_offsets[k] = d.offsets[k];
        for (size_t i = 0; i < d.rows; i++) A.values(i, k) = T(0);
    }
    for (size_t i = 0; i < d.rows; i++)
        for (int e = d.Ap[i]; e < d.Ap[i + 1]; e++)
            for (size_t k = 0; k < d.ndiag; k++)
                if (d.offsets[k] == d.Aj[e] - (int)i) A.values(i, k) = d.Ax[e];
    return A;
}

// ---- names -> functor types --------------------------------------------------------------------------------------------------------
template <typename T, typename F> bool with_combine(const std::string &name, F &&f)
{
    if (name == "plus") f(cusp::plus<T>());
    else if (name == "multiplies") f(cusp::multiplies<T>());
    else if (name == "minimum") f(cusp::minimum<T>());
    else if (name == "maximum") f(cusp::maximum<T>());
    else if (name == "project1st") f(cusp::project1st<T>());
    else if (name == "project2nd") f(cusp::project2nd<T>());
    else return false;
    return true;
}
template <typename T, typename F> bool with_reduce(const std::string &name, F &&f)
{
    if (name == "plus") f(cusp::plus<T>());
    else if (name == "multiplies") f(cusp::multiplies<T>());
    else if (name == "minimum") f(cusp::minimum<T>());
    else if (name == "maximum") f(cusp::maximum<T>());
    else return false;
    return true;
}

// one case on matrix A (in `Space`): y starts as y0, the result comes back to the host
template <typename Space, typename T, typename Matrix>
std::vector<T> run_case(const Matrix &A, const deck<T> &d, const typename deck<T>::one &c, bool generalized)
{
    const cusp::array1d<T, Space> x(cusp::array1d<T, Host>(d.x.begin(), d.x.end()));
    cusp::array1d<T, Space> y(cusp::array1d<T, Host>(d.y0.begin(), d.y0.end()));
    std::vector<T> out;
    const bool ok = with_combine<T>(c.combine, [&](auto comb) {
        with_reduce<T>(c.reduce, [&](auto red) {
            if (generalized) {
                cusp::array1d<T, Space> z(d.rows, T(-77));
                cusp::generalized_spmv(A, x, y, z, comb, red);
                out = cusp::detail::host_copy(z);
            } else {
                if (c.start == "y0") cusp::multiply(A, x, y, cusp::identity_function<T>(), comb, red);
                else cusp::multiply(A, x, y, cusp::constant_functor<T>((T)std::strtod(c.start.c_str(), nullptr)), comb, red);
                out = cusp::detail::host_copy(y);
            }
        });
    });
    if (!ok || out.size() != d.rows) throw std::runtime_error("bad case: " + c.combine + " " + c.reduce);
    return out;
}

template <typename Space, typename T> struct formats {
    typename cusp::csr_matrix<int, T, Host>::template rebind<Space>::type csr;
    typename cusp::coo_matrix<int, T, Host>::template rebind<Space>::type coo;
    typename cusp::ell_matrix<int, T, Host>::template rebind<Space>::type ell;
    typename cusp::dia_matrix<int, T, Host>::template rebind<Space>::type dia;
    typename cusp::hyb_matrix<int, T, Host>::template rebind<Space>::type hyb;
    explicit formats(const deck<T> &d) : csr(make_csr(d)), coo(make_coo(d)), ell(make_ell(d)), dia(make_dia(d)), hyb(make_hyb(d)) {}
};

template <typename Space, typename T> std::vector<std::vector<T>> run_deck(const deck<T> &d)
{
    const formats<Space, T> f(d);
    std::vector<std::vector<T>> out;
    for (const auto &c : d.cases) {
        const bool g = c.format.compare(0, 2, "g:") == 0;
        const std::string fmt = g ? c.format.substr(2) : c.format;
        if (fmt == "csr") out.push_back(run_case<Space>(f.csr, d, c, g));
        else if (fmt == "coo") out.push_back(run_case<Space>(f.coo, d, c, g));
        else if (fmt == "ell") out.push_back(run_case<Space>(f.ell, d, c, g));
        else if (fmt == "dia") out.push_back(run_case<Space>(f.dia, d, c, g));
        else if (fmt == "hyb") out.push_back(run_case<Space>(f.hyb, d, c, g));
        else throw std::runtime_error("bad format: " + c.format);
    }
    return out;
}

// NaN against NaN is equal whatever the payload; everything else by bit pattern (tests/special_values.py same_bits)
template <typename T> bool same_bits(const std::vector<T> &a, const std::vector<T> &b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++) {
        if (a[i] != a[i] || b[i] != b[i]) {
            if ((a[i] != a[i]) != (b[i] != b[i])) return false;
        } else if (std::memcmp(&a[i], &b[i], sizeof(T)) != 0) return false;
    }
    return true;
}

template <typename T> void print_line(const std::vector<T> &v)
{
    for (size_t i = 0; i < v.size(); i++) std::printf("%s%a", i ? " " : "", (double)v[i]);
    std::printf("\n");
}

} // namespace semiring_check

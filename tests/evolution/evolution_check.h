// Shared by the evolution-strength test programs: decks written by the Python side (bits as hex), the measure's result printed
// the same way, bitwise comparisons and the preconditioned-cg case that both memory spaces run.
#pragma once
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <set>
#include <string>
#include <vector>

#include <cusp/coo_matrix.h>
#include <cusp/csr_matrix.h>
#include <cusp/dia_matrix.h>
#include <cusp/ell_matrix.h>
#include <cusp/gallery/diffusion.h>
#include <cusp/gallery/stencil.h>
#include <cusp/hyb_matrix.h>
#include <cusp/krylov/cg.h>
#include <cusp/monitor.h>
#include <cusp/precond/aggregation/smoothed_aggregation.h>

#include "unittest.h"

namespace evolution_check {

namespace agg = cusp::precond::aggregation;
template <typename V> using host_csr = cusp::csr_matrix<int, V, cusp::host_memory>;

template <typename V> uint64_t bits_of(V v)
{
    typename std::conditional<sizeof(V) == 8, uint64_t, uint32_t>::type u;
    std::memcpy(&u, &v, sizeof(V));
    return u;
}
template <typename V> V from_bits(uint64_t b)
{
    typename std::conditional<sizeof(V) == 8, uint64_t, uint32_t>::type u = (decltype(u))b;
    V v;
    std::memcpy(&v, &u, sizeof(V));
    return v;
}

template <typename V> struct deck {
    host_csr<V> A;
    cusp::array1d<V, cusp::host_memory> B;
    double rho = 0.0, epsilon = 4.0;
};

// the file: "n entries rho epsilon" / the offsets / the columns / the values as hex / B as hex (rho and epsilon as hex doubles)
template <typename V> deck<V> read_deck(const char *path)
{
    std::ifstream in(path);
    if (!in) throw std::runtime_error(std::string("cannot read ") + path);
    size_t n = 0, entries = 0;
    std::string rho, epsilon, word;
    in >> n >> entries >> rho >> epsilon;
    deck<V> d;
    d.rho = from_bits<double>(std::strtoull(rho.c_str(), nullptr, 16));
    d.epsilon = from_bits<double>(std::strtoull(epsilon.c_str(), nullptr, 16));
    d.A.resize(n, n, entries);
    d.B.resize(n);
    for (size_t i = 0; i <= n; i++) in >> d.A.row_offsets[i];
    for (size_t e = 0; e < entries; e++) in >> d.A.column_indices[e];
    for (size_t e = 0; e < entries; e++) { in >> word; d.A.values[e] = from_bits<V>(std::strtoull(word.c_str(), nullptr, 16)); }
    for (size_t i = 0; i < n; i++) { in >> word; d.B[i] = from_bits<V>(std::strtoull(word.c_str(), nullptr, 16)); }
    if (!in) throw std::runtime_error(std::string("short deck ") + path);
    return d;
}

template <typename V> void print_csr(const char *name, const host_csr<V> &m)
{
    std::printf("%s %zu %zu\n", name, m.num_rows, m.num_entries);
    for (size_t i = 0; i <= m.num_rows; i++) std::printf("%d ", (int)m.row_offsets[i]);
    std::printf("\n");
    for (size_t e = 0; e < m.num_entries; e++) std::printf("%d %" PRIx64 "\n", (int)m.column_indices[e], bits_of<V>(m.values[e]));
}

// "--measure f64|f32 deck ...": the measure of every deck in Space, printed; a refusal prints "refused"
template <typename V, typename Space> int print_measures(int argc, char **argv)
{
    for (int i = 3; i < argc; i++) {
        const deck<V> d = read_deck<V>(argv[i]);
        cusp::csr_matrix<int, V, Space> A(d.A), S;
        cusp::array1d<V, Space> B(d.B);
        try {
            agg::evolution_strength_of_connection(A, S, B, d.rho, d.epsilon);
        } catch (const cusp::invalid_input_exception &) {
            std::printf("refused\n");
            continue;
        }
        print_csr<V>("S", host_csr<V>(S));
    }
    return 0;
}

// NaNs compare equal to NaNs here (sign and payload of a NaN differ between x86 and gfx950), everything else by its bits
template <typename V> bool same_values(const std::vector<V> &a, const std::vector<V> &b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (!(a[i] != a[i] && b[i] != b[i]) && bits_of<V>(a[i]) != bits_of<V>(b[i])) return false;
    return true;
}
template <typename MA, typename MB> bool csr_bits_equal(const MA &a, const MB &b)
{
    typedef typename MA::value_type V;
    return a.num_rows == b.num_rows && a.num_cols == b.num_cols && a.num_entries == b.num_entries &&
           cusp::detail::host_copy(a.row_offsets) == cusp::detail::host_copy(b.row_offsets) &&
           cusp::detail::host_copy(a.column_indices) == cusp::detail::host_copy(b.column_indices) &&
           same_values<V>(cusp::detail::host_copy(a.values), cusp::detail::host_copy(b.values));
}

// the diagonals (column - row) that a CSR matrix holds
template <typename M> std::set<long> diagonals_of(const M &m)
{
    const host_csr<typename M::value_type> h(m);
    std::set<long> out;
    for (size_t i = 0; i < h.num_rows; i++)
        for (int e = h.row_offsets[i]; e < h.row_offsets[i + 1]; e++) out.insert((long)h.column_indices[e] - (long)i);
    return out;
}

// b[i] from a fixed hash in [-1, 1)
template <typename V, typename Space> cusp::array1d<V, Space> seeded_rhs(size_t n)
{
    cusp::array1d<V, cusp::host_memory> b(n);
    for (size_t i = 0; i < n; i++) {
        uint64_t z = (i + 1) * 0x9E3779B97F4A7C15ull;
        z ^= z >> 31; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 29;
        b[i] = V((double)(z % 65536) / 32768.0 - 1.0);
    }
    return cusp::array1d<V, Space>(b);
}

struct sa_run {
    long iterations = -1; // of cg to a relative residual of 1e-8; -1: not converged in 500
    std::vector<size_t> level_rows;
};

// smoothed aggregation (levels down to 100 rows) as the preconditioner of cg on diffusion<FD> 40 x 30, eps 1e-3, angle 0
template <typename Space> sa_run anisotropic_cg(bool evolution, bool mis = false)
{
    cusp::csr_matrix<int, double, Space> A;
    cusp::gallery::diffusion<cusp::gallery::FD>(A, 40, 30, 1e-3, 0.0);
    agg::smoothed_aggregation<int, double, Space> M;
    M.min_level_size = 100;
    M.evolution_strength = evolution;
    M.mis_aggregation = mis;
    M.initialize(A);
    sa_run out;
    for (size_t l = 0; l < M.sa_levels.size(); l++) out.level_rows.push_back(M.sa_levels[l].A_.num_rows);
    const cusp::array1d<double, Space> b = seeded_rhs<double, Space>(A.num_rows);
    cusp::array1d<double, Space> x(A.num_rows, 0.0);
    cusp::monitor<double> monitor(b, 500, 1e-8);
    cusp::krylov::cg(A, x, b, monitor, M);
    if (monitor.converged()) out.iterations = (long)monitor.iteration_count();
    return out;
}

inline void print_run(const char *what, const sa_run &r)
{
    std::printf("%s: %ld iterations, levels", what, r.iterations);
    for (size_t rows : r.level_rows) std::printf(" %zu", rows);
    std::printf("\n");
}

} // namespace evolution_check

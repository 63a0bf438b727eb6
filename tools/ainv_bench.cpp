// tools/ainv_bench.cpp -- the AINV preconditioners (cusp/precond/ainv.h) on poisson5pt(g, g) with values[0] = 10, f64, device_memory:
//   ainv_bench [--grids=1000] [--rounds=9] [--reps=200]
// Per grid and per dropping setting (drop tolerance .1; ten entries per row):
//   set-up        host wall time of the constructor (the factorisation is sequential host code, then two conversions and a transpose)
//   apply         z = M r through the scaled plan (two launches) against multiply, xmy, multiply (three launches) of the same object
//                 (row_scale_route on / off), in ALTERNATED rounds of --reps applies between two device synchronisations; per apply,
//                 median of the rounds [min, max].  The verdict line applies the rule of DESIGN 3.18: the scaled plan is the default
//                 only if it is faster than the three steps by more than twice the three steps' own spread (max - min).
//   cg            per MARGINAL iteration ((t(60) - t(20)) / 40, relative tolerance 0 so the limit ends the solve; median of the
//                 rounds [min, max]) and iterations to the monitor's default tolerance (1e-5 relative, b = 1, x0 = 0), for the fused
//                 branch, cg_plain (CMI_CG_FUSED_AINV=0) and no preconditioner.
#include <cusp/csr_matrix.h>
#include <cusp/gallery/poisson.h>
#include <cusp/krylov/cg.h>
#include <cusp/monitor.h>
#include <cusp/precond/ainv.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

typedef cusp::device_memory D;
using cusp::detail::check;

static double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct stats { double med, lo, hi; };
static stats summarise(std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    return {v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]), v.front(), v.back()};
}
static void report(const char *what, const stats &s, size_t rounds) { std::printf("    %-44s %9.2f us [%.2f, %.2f] over %zu rounds\n", what, s.med, s.lo, s.hi, rounds); }

template <typename M> double time_applies(const M &m, const cusp::array1d<double, D> &x, cusp::array1d<double, D> &y, int reps)
{
    check(cmi_device_synchronize());
    const double t0 = now_us();
    for (int i = 0; i < reps; i++) m(x, y);
    check(cmi_device_synchronize());
    return (now_us() - t0) / reps;
}

// wall time of one cg solve that the iteration limit ends
template <typename A, typename M> double time_cg(const A &a, const cusp::array1d<double, D> &b, M &m, size_t limit, size_t *iterations = nullptr, double rel = 0.0)
{
    cusp::array1d<double, D> x(a.num_rows, 0.0);
    cusp::monitor<double> monitor(b, limit, rel);
    check(cmi_device_synchronize());
    const double t0 = now_us();
    cusp::krylov::cg(a, x, b, monitor, m);
    check(cmi_device_synchronize());
    if (iterations) *iterations = monitor.converged() ? monitor.iteration_count() : 0;
    return now_us() - t0;
}
template <typename A, typename M> void cg_figures(const char *what, const A &a, const cusp::array1d<double, D> &b, M &m, int rounds)
{
    std::vector<double> marginal;
    time_cg(a, b, m, 20); // warm-up: plans, code objects
    for (int r = 0; r < rounds; r++) {
        const double t20 = time_cg(a, b, m, 20), t60 = time_cg(a, b, m, 60);
        marginal.push_back((t60 - t20) / 40.0);
    }
    size_t its = 0;
    const double total = time_cg(a, b, m, 20000, &its, 1e-5);
    const stats s = summarise(marginal);
    std::printf("    cg %-41s %9.2f us per marginal iteration [%.2f, %.2f]; %zu iterations to 1e-5 in %.1f ms\n", what, s.med, s.lo, s.hi, its, total / 1000.0);
}

template <typename Hyb> void shape(const char *name, const Hyb &m)
{
    std::printf("    %-4s %zu entries: ELL width %zu, %zu COO entries (%.2f per row)\n", name, (size_t)m.num_entries, (size_t)m.ell.column_indices.num_cols, (size_t)m.coo.num_entries,
                (double)m.coo.num_entries / (double)m.num_rows);
}

static void run(size_t g, int rounds, int reps, double tol, int per_row)
{
    cusp::csr_matrix<int, double, cusp::host_memory> Ah;
    cusp::gallery::poisson5pt(Ah, g, g);
    Ah.values[0] = 10;
    const cusp::csr_matrix<int, double, D> A(Ah);
    std::printf("  poisson5pt %zu x %zu (values[0] = 10), f64: %zu rows, %zu entries; bridson_ainv(A, %g, %d)\n", g, g, A.num_rows, A.num_entries, tol, per_row);
    double t0 = now_us();
    cusp::precond::bridson_ainv<double, D> M(A, tol, per_row);
    std::printf("    set-up (host factorisation, conversions, transpose) %.2f s\n", (now_us() - t0) / 1e6);
    shape("w", M.w);
    shape("w_t", M.w_t);
    const cusp::array1d<double, D> x(A.num_rows, 1.0), b(A.num_rows, 1.0);
    cusp::array1d<double, D> y(A.num_rows);
    M(x, y); // warm-up of the scaled route; makes the second plan
    std::printf("    the second plan %s the row scale\n", M.row_scale_in_use() ? "carries" : "REFUSED (two launches per multiply):");
    M.row_scale_route = false;
    M(x, y); // ... and of the three steps (their kernels' code objects are loaded outside the timed rounds too)
    time_applies(M, x, y, reps);
    M.row_scale_route = true;
    time_applies(M, x, y, reps);
    std::vector<double> scaled, three;
    for (int r = 0; r < rounds; r++) { // alternated: both see the same drift of the machine
        M.row_scale_route = true;
        scaled.push_back(time_applies(M, x, y, reps));
        M.row_scale_route = false;
        three.push_back(time_applies(M, x, y, reps));
    }
    const stats s = summarise(scaled), t = summarise(three);
    report("apply, scaled plan (2 launches)", s, scaled.size());
    report("apply, multiply + xmy + multiply (3 launches)", t, three.size());
    const double gain = t.med - s.med, spread = t.hi - t.lo;
    std::printf("    verdict: the scaled plan is %.2f us (%.1f %%) %s; twice the three steps' spread is %.2f us -> default %s\n", gain < 0 ? -gain : gain, 100.0 * gain / t.med,
                gain < 0 ? "slower" : "faster", 2 * spread, gain > 2 * spread ? "SCALED PLAN" : "THREE STEPS");
    M.row_scale_route = true;
    setenv("CMI_CG_FUSED_AINV", "1", 1);
    cg_figures("bridson_ainv, fused branch, scaled plan", A, b, M, rounds);
    M.row_scale_route = false;
    cg_figures("bridson_ainv, fused branch, three steps", A, b, M, rounds);
    setenv("CMI_CG_FUSED_AINV", "0", 1);
    cg_figures("bridson_ainv, cg_plain, three steps", A, b, M, rounds);
    unsetenv("CMI_CG_FUSED_AINV");
    cusp::identity_operator<double, D> I(A.num_rows, A.num_cols);
    cg_figures("no preconditioner (fused)", A, b, I, rounds);
}

int main(int argc, char **argv)
{
    std::string grids = "1000";
    int rounds = 9, reps = 200;
    for (int i = 1; i < argc; i++) {
        if (!std::strncmp(argv[i], "--grids=", 8)) grids = argv[i] + 8;
        else if (!std::strncmp(argv[i], "--rounds=", 9)) rounds = std::atoi(argv[i] + 9);
        else if (!std::strncmp(argv[i], "--reps=", 7)) reps = std::atoi(argv[i] + 7);
        else { std::fprintf(stderr, "usage: ainv_bench [--grids=1000,3162] [--rounds=9] [--reps=200]\n"); return 2; }
    }
    std::printf("ainv_bench: rounds %d, %d applies per round\n", rounds, reps);
    for (size_t pos = 0; pos < grids.size();) {
        const size_t comma = grids.find(',', pos);
        const size_t g = (size_t)std::atol(grids.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos).c_str());
        run(g, rounds, reps, .1, -1);
        run(g, rounds, reps, 0, 10);
        if (comma == std::string::npos) break;
        pos = comma + 1;
    }
    return 0;
}

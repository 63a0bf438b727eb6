// tools/multishift_bench.cpp -- cusp::krylov::cg_m on poisson5pt(grid, grid) CSR in device_memory: the fused iteration (speculative multiply + <y,p>,
// cmi_cg_update_*, cmi_cg_m_coefficients_*, cmi_cg_m_update_xp_*: four launches, one host read) against the operation-by-operation path of the same
// build ($CMI_CG_M_FUSED=0: three host reads per iteration, the per-shift coefficients formed on the host and uploaded), interleaved in one process.
//   multishift_bench [--grids=1000,3162] [--rounds=5] [--short=10] [--long=50]
// For every grid x {f64, f32} x num_shifts {1, 4, 16} it prints two figures, each the median of the rounds with [min, max]:
//   * the MARGINAL iteration: (wall time of `long` iterations - wall time of `short` iterations) / (long - short), so set-up, the allocation
//     of the work vectors and the final synchronisation cancel; sigma_s = 0.1 (s + 1), b = 1, the monitor never satisfied (tolerance 0);
//   * cmi_cg_m_update_xp_* alone, event-timed over 20 back-to-back calls, against its byte model (4 num_shifts + 3) N sizeof(T): x_s and p_s read and
//     written, r read, p0 read and written.
#include <cusp/csr_matrix.h>
#include <cusp/gallery/poisson.h>
#include <cusp/krylov/cg_m.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

typedef std::map<std::string, std::vector<double>> samples;

static double median(std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    return v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]);
}
static void report(const char *what, const std::vector<double> &v, const char *unit)
{
    std::printf("  %-34s %10.2f %s [%10.2f, %10.2f]", what, median(v), unit, *std::min_element(v.begin(), v.end()), *std::max_element(v.begin(), v.end()));
}

template <typename V> struct bench {
    typedef cusp::array1d<V, cusp::device_memory> Vec;
    cusp::csr_matrix<int, V, cusp::device_memory> A;
    Vec b;

    explicit bench(size_t grid)
    {
        cusp::gallery::poisson5pt(A, grid, grid);
        b = Vec(A.num_rows, V(1));
        A.plan(); // made once, outside the timings
    }
    // wall ms of `iterations` iterations through the public call
    double solve_ms(Vec &x, const Vec &sigma, size_t iterations, bool fused)
    {
        setenv("CMI_CG_M_FUSED", fused ? "1" : "0", 1);
        cusp::monitor<V> monitor(b, iterations, V(0));
        cusp::detail::check(cmi_device_synchronize());
        const auto t0 = std::chrono::steady_clock::now();
        cusp::krylov::cg_m(A, x, b, sigma, monitor);
        cusp::detail::check(cmi_device_synchronize());
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (monitor.iteration_count() != iterations) throw cusp::runtime_exception("multishift_bench: the solver stopped early");
        return ms;
    }
    // cmi_cg_m_update_xp_* alone: us per call
    double update_xp_us(Vec &x, Vec &ps, Vec &p0, const Vec &r, const Vec &state, const Vec &coef, size_t ns, int reps)
    {
        void *e0 = nullptr, *e1 = nullptr;
        cusp::detail::check(cmi_event_create(&e0));
        cusp::detail::check(cmi_event_create(&e1));
        auto once = [&] {
            cusp::detail::check(cusp::detail::by_type<V>(cmi_cg_m_update_xp_f64, cmi_cg_m_update_xp_f32)(
                A.num_rows, ns, A.num_rows, state.data(), coef.data(), coef.data() + ns, coef.data() + 2 * ns, r.data(), p0.data(), x.data(), ps.data(), nullptr));
        };
        once();
        cusp::detail::check(cmi_event_record(e0, nullptr));
        for (int k = 0; k < reps; k++) once();
        cusp::detail::check(cmi_event_record(e1, nullptr));
        float ms = 0;
        cusp::detail::check(cmi_event_elapsed_ms(e0, e1, &ms));
        cmi_event_destroy(e0);
        cmi_event_destroy(e1);
        return 1000.0 * ms / reps;
    }
    void run(size_t grid, const char *tag, int rounds, size_t k_short, size_t k_long)
    {
        const size_t N = A.num_rows;
        for (size_t ns : {size_t(1), size_t(4), size_t(16)}) {
            cusp::array1d<V, cusp::host_memory> hs(ns), hc(3 * ns);
            for (size_t s = 0; s < ns; s++) hs[s] = V(0.1 * (s + 1));
            for (size_t s = 0; s < 3 * ns; s++) hc[s] = V(s < ns ? 1e-3 : s < 2 * ns ? 0.5 : 0.25); // beta_s, alpha_s, zeta_0: values that stay bounded over the repetitions
            const Vec sigma(hs), coef(hc), state(std::vector<V>{V(1), V(0.5)});
            Vec x(N * ns), ps(N * ns, V(1)), p0(N, V(1));
            samples out;
            for (int r = -1; r < rounds; r++) { // round -1: warm-up
                if (r == 0) out.clear();
                for (bool fused : {true, false}) {
                    const double a = solve_ms(x, sigma, k_short, fused), c = solve_ms(x, sigma, k_long, fused);
                    out[fused ? "fused" : "generic"].push_back(1000.0 * (c - a) / double(k_long - k_short));
                }
                cusp::blas::fill(x, V(0));
                out["xp"].push_back(update_xp_us(x, ps, p0, b, state, coef, ns, 20));
            }
            const double spread = 0.5 * ((*std::max_element(out["fused"].begin(), out["fused"].end()) - *std::min_element(out["fused"].begin(), out["fused"].end())) +
                                         (*std::max_element(out["generic"].begin(), out["generic"].end()) - *std::min_element(out["generic"].begin(), out["generic"].end())));
            const double bytes = (4.0 * ns + 3.0) * N * sizeof(V);
            std::printf("poisson5pt %zu^2 %s num_shifts %zu\n", grid, tag, ns);
            report("marginal iteration, fused", out["fused"], "us");
            std::printf("\n");
            report("marginal iteration, CMI_CG_M_FUSED=0", out["generic"], "us");
            std::printf("   generic - fused %+.2f us, run-to-run spread %.2f us\n", median(out["generic"]) - median(out["fused"]), spread);
            report("cmi_cg_m_update_xp alone", out["xp"], "us");
            std::printf("   byte model %.1f MB -> %.2f TB/s\n", bytes / 1e6, bytes / median(out["xp"]) / 1e6);
            std::fflush(stdout);
        }
    }
};

int main(int argc, char **argv)
{
    std::vector<size_t> grids = {1000, 3162};
    int rounds = 5;
    size_t k_short = 10, k_long = 50;
    for (int i = 1; i < argc; i++) {
        if (!std::strncmp(argv[i], "--grids=", 8)) {
            grids.clear();
            for (const char *p = argv[i] + 8; *p;) {
                char *end = nullptr;
                grids.push_back(std::strtoull(p, &end, 10));
                p = *end == ',' ? end + 1 : end;
            }
        } else if (!std::strncmp(argv[i], "--rounds=", 9)) rounds = std::atoi(argv[i] + 9);
        else if (!std::strncmp(argv[i], "--short=", 8)) k_short = std::strtoull(argv[i] + 8, nullptr, 10);
        else if (!std::strncmp(argv[i], "--long=", 7)) k_long = std::strtoull(argv[i] + 7, nullptr, 10);
        else { std::fprintf(stderr, "usage: multishift_bench [--grids=1000,3162] [--rounds=5] [--short=10] [--long=50]\n"); return 2; }
    }
    if (rounds < 1 || k_long <= k_short || grids.empty()) { std::fprintf(stderr, "multishift_bench: need rounds >= 1, long > short and a grid\n"); return 2; }
    try {
        std::printf("multishift_bench: cusp::krylov::cg_m, CSR through its plan, device_memory; %d interleaved rounds behind one warm-up round; median [min, max]\n", rounds);
        std::printf("marginal iteration = (t(%zu iterations) - t(%zu iterations)) / %zu\n", k_long, k_short, k_long - k_short);
        for (size_t grid : grids) {
            { bench<double> d(grid); d.run(grid, "f64", rounds, k_short, k_long); }
            { bench<float> f(grid); f.run(grid, "f32", rounds, k_short, k_long); }
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "multishift_bench: %s\n", e.what());
        return 1;
    }
    return 0;
}

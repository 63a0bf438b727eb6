// tools/lobpcg_bench.cpp -- cusp::eigen::lobpcg (smallest eigenvalue, identity M) on poisson5pt(grid, grid) CSR in device_memory: the fused
// iteration (cmi_blas_scal_recip_*, the planned multiply, cmi_lobpcg_gram_*, one read of eight doubles, cmi_lobpcg_update_*) against the
// operation-by-operation path of the same build ($CMI_LOBPCG_FUSED=0: 33 vector reads, 9 writes and 12 host reads), interleaved in one process.
//   lobpcg_bench [--grids=1000,3162] [--rounds=5] [--short=10] [--long=50]
// For every grid x {f64, f32} it prints, each the median of the rounds with [min, max]:
//   * the MARGINAL iteration: (wall time of `long` iterations - wall time of `short` iterations) / (long - short), so set-up, the allocation of
//     the work vectors and the final synchronisation cancel; the start vector is cusp::random_array<T>(N, 7), the tolerance 0 (never met);
//   * cmi_lobpcg_gram_* and cmi_lobpcg_update_* alone, event-timed over 20 back-to-back calls, against their byte models 7 N sizeof(T) (x, w, aw
//     read; p, ap read and written) and 11 N sizeof(T) (w, aw read; p, ap, x, ax read and written; r written).
#include <cusp/copy.h>
#include <cusp/csr_matrix.h>
#include <cusp/eigen/lobpcg.h>
#include <cusp/gallery/poisson.h>

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
    std::printf("  %-38s %10.2f %s [%10.2f, %10.2f]", what, median(v), unit, *std::min_element(v.begin(), v.end()), *std::max_element(v.begin(), v.end()));
}

template <typename V> struct bench {
    typedef cusp::array1d<V, cusp::device_memory> Vec;
    cusp::csr_matrix<int, V, cusp::device_memory> A;

    explicit bench(size_t grid)
    {
        cusp::gallery::poisson5pt(A, grid, grid);
        A.plan(); // made once, outside the timings
    }
    // wall ms of `iterations` iterations through the public call
    double solve_ms(size_t iterations, bool fused)
    {
        setenv("CMI_LOBPCG_FUSED", fused ? "1" : "0", 1);
        Vec X(A.num_rows), S(1);
        cusp::copy(cusp::random_array<V>(A.num_rows, 7), X);
        const cusp::array1d<V, cusp::host_memory> ones(1, V(1));
        cusp::monitor<V> monitor(ones, iterations, V(0));
        cusp::detail::check(cmi_device_synchronize());
        const auto t0 = std::chrono::steady_clock::now();
        cusp::eigen::lobpcg(A, S, X, monitor, false);
        cusp::detail::check(cmi_device_synchronize());
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (monitor.iteration_count() != iterations) throw cusp::runtime_exception("lobpcg_bench: the solver stopped early");
        return ms;
    }
    template <typename Call> double alone_us(Call once, int reps)
    {
        void *e0 = nullptr, *e1 = nullptr;
        cusp::detail::check(cmi_event_create(&e0));
        cusp::detail::check(cmi_event_create(&e1));
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
        using cusp::detail::by_type;
        const size_t N = A.num_rows;
        Vec x(N, V(0.5)), ax(N, V(0.25)), w(N, V(1)), aw(N, V(2)), p(N, V(1)), ap(N, V(1)), r(N);
        cusp::array1d<double, cusp::device_memory> sc(std::vector<double>{0, 0, 1.0}), gram(8); // sc[2] = <p, p> = 1: s = 1, the values stay where they are
        void *ws = cusp::blas::detail::workspace().ws;
        samples out;
        for (int k = -1; k < rounds; k++) { // round -1: warm-up
            if (k == 0) out.clear();
            for (bool fused : {true, false}) {
                const double a = solve_ms(k_short, fused), c = solve_ms(k_long, fused);
                out[fused ? "fused" : "plain"].push_back(1000.0 * (c - a) / double(k_long - k_short));
            }
            out["gram"].push_back(alone_us([&] {
                cusp::detail::check(by_type<V>(cmi_lobpcg_gram_f64, cmi_lobpcg_gram_f32)(N, sc.data() + 2, x.data(), w.data(), aw.data(), p.data(), ap.data(), gram.data(), ws, nullptr));
            }, 20));
            out["update"].push_back(alone_us([&] { // coefficients that keep every vector bounded over the repetitions
                cusp::detail::check(by_type<V>(cmi_lobpcg_update_f64, cmi_lobpcg_update_f32)(N, V(0.5), V(1e-3), V(0.25), 0, V(0.125), w.data(), aw.data(), p.data(), ap.data(),
                                                                                             x.data(), ax.data(), r.data(), sc.data(), nullptr, ws, nullptr));
            }, 20));
            cusp::blas::fill(p, V(1));
            cusp::blas::fill(ap, V(1));
        }
        const double gram_bytes = 7.0 * N * sizeof(V), update_bytes = 11.0 * N * sizeof(V);
        std::printf("poisson5pt %zu^2 %s\n", grid, tag);
        report("marginal iteration, fused", out["fused"], "us");
        std::printf("\n");
        report("marginal iteration, CMI_LOBPCG_FUSED=0", out["plain"], "us");
        std::printf("   fused / plain %.3f\n", median(out["fused"]) / median(out["plain"]));
        report("cmi_lobpcg_gram alone", out["gram"], "us");
        std::printf("   byte model %.1f MB -> %.2f TB/s\n", gram_bytes / 1e6, gram_bytes / median(out["gram"]) / 1e6);
        report("cmi_lobpcg_update alone", out["update"], "us");
        std::printf("   byte model %.1f MB -> %.2f TB/s\n", update_bytes / 1e6, update_bytes / median(out["update"]) / 1e6);
        std::fflush(stdout);
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
        else { std::fprintf(stderr, "usage: lobpcg_bench [--grids=1000,3162] [--rounds=5] [--short=10] [--long=50]\n"); return 2; }
    }
    if (rounds < 1 || k_long <= k_short || grids.empty()) { std::fprintf(stderr, "lobpcg_bench: need rounds >= 1, long > short and a grid\n"); return 2; }
    try {
        std::printf("lobpcg_bench: cusp::eigen::lobpcg, smallest eigenvalue, CSR through its plan, device_memory; %d interleaved rounds behind one warm-up round; median [min, max]\n", rounds);
        std::printf("marginal iteration = (t(%zu iterations) - t(%zu iterations)) / %zu\n", k_long, k_short, k_long - k_short);
        for (size_t grid : grids) {
            { bench<double> d(grid); d.run(grid, "f64", rounds, k_short, k_long); }
            { bench<float> f(grid); f.run(grid, "f32", rounds, k_short, k_long); }
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "lobpcg_bench: %s\n", e.what());
        return 1;
    }
    return 0;
}

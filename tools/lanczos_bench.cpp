// tools/lanczos_bench.cpp -- cusp::eigen::lanczos on poisson5pt(grid, grid) CSR in device_memory and cmi_dense_gemm_* alone.
//   lanczos_bench [--grids=1000,3162] [--rounds=3] [--profiles=profiles] [--out-dir=DIR]
// Everything printed also goes to the next free record <out-dir>/rNN_lanczos_bench.txt, NN one past the highest rNN_* in the --profiles
// directory; --out-dir defaults to the --profiles directory; no record is written when that directory cannot be read.
// For every grid x {f64, f32}, each the median of the rounds with [min, max], the two paths interleaved in one process:
//   * the MARGINAL iteration, fused against $CMI_LANCZOS_FUSED=0 (operation by operation): reorth = None as (t(50 steps) - t(10 steps)) / 40,
//     reorth = Full round m = 50 as (t(70) - t(30)) / 40 and round m = 100 as (t(130) - t(70)) / 60 (a step's cost grows linearly with
//     the number of stored vectors, so the mean over a window is the cost at its centre; a window of ten steps drowned in the run-to-run
//     spread of two whole calls) -- minIter = maxIter = the step count, so no convergence test runs, and set-up, allocation and the final
//     synchronisation cancel; no eigenvectors (Full keeps V anyway);
//   * cmi_dense_gemm_* alone by events for (m, k, n) = (N, 50, 5), (N, 100, 5), (N, 100, 16): time, and the byte model (m k + m n) sizeof(T) per
//     second -- beside it the same product as n k cusp::blas::axpy calls on the columns (what the library had before: A read n times), timed
//     in turn in the same process, and the share of the 8 TB/s peak, printed beside the 0.89-0.91 of peak the README records for one nt
//     16-byte read stream.
#include <cusp/array2d.h>
#include <cusp/csr_matrix.h>
#include <cusp/eigen/lanczos.h>
#include <cusp/gallery/poisson.h>

#include <dirent.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

typedef std::map<std::string, std::vector<double>> samples;
static const double kPeakBytesPerSecond = 8e12;

static const char *const kRecordedStream = "0.89-0.91"; // README: one nt 16-byte read stream, share of peak
static std::FILE *record = nullptr;

// printf to stdout and to the record
static void say(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static void say(const char *fmt, ...)
{
    va_list args, copy;
    va_start(args, fmt);
    va_copy(copy, args);
    std::vprintf(fmt, args);
    if (record) std::vfprintf(record, fmt, copy);
    va_end(copy);
    va_end(args);
}
// one past the highest NN of the rNN_* files in `dir`; -1 when it cannot be read
static int next_free_round(const char *dir)
{
    DIR *d = opendir(dir);
    if (!d) return -1;
    int highest = 0;
    while (const dirent *e = readdir(d)) {
        int nn = 0;
        if (std::sscanf(e->d_name, "r%d_", &nn) == 1) highest = std::max(highest, nn);
    }
    closedir(d);
    return highest + 1;
}

static double median(std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    return v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]);
}
static void report(const char *what, const std::vector<double> &v, const char *unit)
{
    say("  %-44s %11.2f %s [%11.2f, %11.2f]", what, median(v), unit, *std::min_element(v.begin(), v.end()), *std::max_element(v.begin(), v.end()));
}

template <typename V> struct bench {
    cusp::csr_matrix<int, V, cusp::device_memory> A;

    explicit bench(size_t grid)
    {
        cusp::gallery::poisson5pt(A, grid, grid);
        A.plan(); // made once, outside the timings
    }
    // wall ms of exactly `steps` Lanczos steps through the public call
    double solve_ms(size_t steps, bool fused, cusp::eigen::ReorthStrategy reorth)
    {
        setenv("CMI_LANCZOS_FUSED", fused ? "1" : "0", 1);
        cusp::eigen::lanczos_options<V> o;
        o.reorth = reorth;
        o.minIter = o.maxIter = steps;
        cusp::array1d<V, cusp::device_memory> values(1);
        cusp::array2d<V, cusp::device_memory, cusp::column_major> none;
        cusp::detail::check(cmi_device_synchronize());
        const auto t0 = std::chrono::steady_clock::now();
        cusp::eigen::lanczos(A, values, none, o);
        cusp::detail::check(cmi_device_synchronize());
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (cusp::eigen::detail::lanczos_detail::last_run().iterations != steps) throw cusp::runtime_exception("lanczos_bench: the solver stopped early");
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
    void marginal(samples &out, const char *name, size_t k_short, size_t k_long, cusp::eigen::ReorthStrategy reorth)
    {
        for (bool fused : {true, false}) {
            const double a = solve_ms(k_short, fused, reorth), c = solve_ms(k_long, fused, reorth);
            out[std::string(name) + (fused ? " fused" : " plain")].push_back(1000.0 * (c - a) / double(k_long - k_short));
        }
    }
    void run(size_t grid, const char *tag, int rounds)
    {
        const size_t N = A.num_rows;
        samples out;
        for (int k = -1; k < rounds; k++) { // round -1: warm-up
            if (k == 0) out.clear();
            marginal(out, "None", 10, 50, cusp::eigen::None);
            marginal(out, "Full m=50", 30, 70, cusp::eigen::Full);
            marginal(out, "Full m=100", 70, 130, cusp::eigen::Full);
        }
        say("poisson5pt %zu^2 %s, marginal Lanczos step\n", grid, tag);
        for (const char *name : {"None", "Full m=50", "Full m=100"}) {
            const std::string f = std::string(name) + " fused", p = std::string(name) + " plain";
            report(f.c_str(), out[f], "us");
            say("\n");
            report((p + " (CMI_LANCZOS_FUSED=0)").c_str(), out[p], "us");
            say("   fused / plain %.3f\n", median(out[f]) / median(out[p]));
        }
        const size_t shapes[3][2] = {{50, 5}, {100, 5}, {100, 16}};
        for (const auto &shape : shapes) {
            const size_t k = shape[0], n = shape[1];
            cusp::array2d<V, cusp::device_memory, cusp::column_major> Vm(N, k), S(k, n, V(0.25)), E(N, n);
            cusp::blas::fill(Vm.values, V(0.5)); // (filled where they live: the constructor's fill stages through the host)
            cusp::blas::fill(E.values, V(0));
            samples alone;
            for (int r = -1; r < rounds; r++) {
                if (r == 0) alone.clear();
                alone["gemm"].push_back(alone_us([&] { cusp::blas::gemm(Vm, S, E); }, 5));
                alone["axpy"].push_back(alone_us([&] {
                    for (size_t c = 0; c < n; c++) {
                        auto e = E.column(c);
                        for (size_t j = 0; j < k; j++) cusp::blas::axpy(Vm.column(j), e, V(0.25));
                    }
                }, 1));
            }
            const double bytes = double(N) * double(k + n) * sizeof(V), rate = bytes / (median(alone["gemm"]) * 1e-6);
            char what[96];
            std::snprintf(what, sizeof what, "cmi_dense_gemm (m, k, n) = (%zu, %zu, %zu)", N, k, n);
            report(what, alone["gemm"], "us");
            say("   byte model %.1f MB -> %.2f TB/s = %.2f of peak (a plain nt read stream, on record: %s)\n", bytes / 1e6, rate / 1e12, rate / kPeakBytesPerSecond, kRecordedStream);
            std::snprintf(what, sizeof what, "  the same as %zu cusp::blas::axpy calls", n * k);
            report(what, alone["axpy"], "us");
            say("   gemm / axpy %.3f\n", median(alone["gemm"]) / median(alone["axpy"]));
            std::fflush(stdout);
            if (record) std::fflush(record);
        }
    }
};

int main(int argc, char **argv)
{
    std::vector<size_t> grids = {1000, 3162};
    int rounds = 3;
    std::string profiles = "profiles", out_dir;
    for (int i = 1; i < argc; i++) {
        if (!std::strncmp(argv[i], "--grids=", 8)) {
            grids.clear();
            for (const char *p = argv[i] + 8; *p;) {
                char *end = nullptr;
                grids.push_back(std::strtoull(p, &end, 10));
                p = *end == ',' ? end + 1 : end;
            }
        } else if (!std::strncmp(argv[i], "--rounds=", 9)) rounds = std::atoi(argv[i] + 9);
        else if (!std::strncmp(argv[i], "--profiles=", 11)) profiles = argv[i] + 11;
        else if (!std::strncmp(argv[i], "--out-dir=", 10)) out_dir = argv[i] + 10;
        else { std::fprintf(stderr, "usage: lanczos_bench [--grids=1000,3162] [--rounds=3] [--profiles=profiles] [--out-dir=DIR]\n"); return 2; }
    }
    if (rounds < 1 || grids.empty()) { std::fprintf(stderr, "lanczos_bench: need rounds >= 1 and a grid\n"); return 2; }
    const int round = next_free_round(profiles.c_str());
    if (round > 0) {
        char name[32];
        std::snprintf(name, sizeof name, "/r%02d_lanczos_bench.txt", round);
        const std::string path = (out_dir.empty() ? profiles : out_dir) + name;
        record = std::fopen(path.c_str(), "w");
        if (!record) std::fprintf(stderr, "lanczos_bench: cannot write %s\n", path.c_str());
    } else {
        std::fprintf(stderr, "lanczos_bench: no directory %s: no record is written\n", profiles.c_str());
    }
    try {
        say("lanczos_bench: cusp::eigen::lanczos, CSR through its plan, device_memory; %d interleaved rounds behind one warm-up round; median [min, max]\n", rounds);
        for (size_t grid : grids) {
            { bench<double> d(grid); d.run(grid, "f64", rounds); }
            { bench<float> f(grid); f.run(grid, "f32", rounds); }
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "lanczos_bench: %s\n", e.what());
        return 1;
    }
    if (record) std::fclose(record);
    return 0;
}

// tools/eigen_bench.cpp -- cusp::eigen's spectral-radius estimators on poisson5pt(grid, grid) in device_memory, f64 and f32 interleaved:
// each estimator through the fused device path (the public call) and through the generic operation-by-operation sequence of the same
// build (the std::false_type overloads of cusp/eigen/*.h: one cusp::blas call and one host read per operation; the row sums: a host copy).
//   eigen_bench [--grid=3162] [--rounds=5]
// Prints, per estimator and value type, the median wall time of the rounds with min and max (as tools/relax_bench.py reports), the ratio
// generic / fused, and for the row sums the event-timed launches alone (row sums + amax, no allocation, no read) against the byte model
// Ap + Ax + row_sums written + the amax read, as a fraction of 8 TB/s.
#include <cusp/csr_matrix.h>
#include <cusp/eigen/spectral_radius.h>
#include <cusp/gallery/poisson.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

typedef std::map<std::string, std::vector<double>> samples;

static double wall_ms(const std::function<double()> &f, double *value)
{
    cusp::detail::check(cmi_device_synchronize());
    const auto t0 = std::chrono::steady_clock::now();
    *value = f();
    cusp::detail::check(cmi_device_synchronize());
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

template <typename V> struct bench {
    typedef cusp::csr_matrix<int, V, cusp::device_memory> Csr;
    Csr A;
    const char *tag;
    cusp::array1d<V, cusp::device_memory> sums;
    std::map<std::string, double> values;

    bench(size_t grid, const char *t) : tag(t)
    {
        cusp::gallery::poisson5pt(A, grid, grid);
        sums.resize(A.num_rows);
        A.plan(); // made once, outside the timings
    }
    void time(samples &out, const std::string &name, const std::function<double()> &f)
    {
        double v = 0;
        out[name + " " + tag].push_back(wall_ms(f, &v));
        values[name] = v;
    }
    double generic_ritz(bool symmetric, size_t k)
    {
        cusp::array2d<V, cusp::host_memory> H;
        if (symmetric) cusp::eigen::detail::lanczos_estimate(A, H, k, std::false_type());
        else cusp::eigen::detail::arnoldi(A, H, k, std::false_type());
        return cusp::eigen::estimate_spectral_radius(H);
    }
    double generic_dinv()
    {
        cusp::eigen::detail::Dinv_A<Csr> DA(A);
        cusp::array2d<V, cusp::host_memory> H;
        cusp::eigen::detail::arnoldi(DA, H, 8, std::false_type());
        return cusp::eigen::estimate_spectral_radius(H);
    }
    // the two launches alone, event-timed over `reps` calls: us per call
    double launches_us(int reps)
    {
        cusp::blas::detail::device_workspace &w = cusp::blas::detail::workspace();
        void *e0 = nullptr, *e1 = nullptr;
        cusp::detail::check(cmi_event_create(&e0));
        cusp::detail::check(cmi_event_create(&e1));
        auto once = [&] {
            cusp::detail::check(cusp::detail::by_type<V>(cmi_csr_abs_row_sums_f64, cmi_csr_abs_row_sums_f32)(
                A.num_rows, A.row_offsets.data(), A.values.data(), sums.data(), 0, nullptr));
            cusp::detail::check(cusp::detail::by_type<V>(cmi_blas_amax_f64, cmi_blas_amax_f32)(sums.size(), sums.data(), static_cast<V *>(w.result), nullptr, w.ws, nullptr));
        };
        once();
        cusp::detail::check(cmi_event_record(e0, nullptr));
        for (int r = 0; r < reps; r++) once();
        cusp::detail::check(cmi_event_record(e1, nullptr));
        float ms = 0;
        cusp::detail::check(cmi_event_elapsed_ms(e0, e1, &ms));
        cmi_event_destroy(e0);
        cmi_event_destroy(e1);
        return 1000.0 * ms / reps;
    }
    void round(samples &out)
    {
        out[std::string("row sums + amax launches (us) ") + tag].push_back(launches_us(20));
        time(out, "disks fused", [&] { return cusp::eigen::disks_spectral_radius(A); });
        time(out, "disks generic", [&] { return cusp::eigen::detail::disks_spectral_radius(A, std::false_type()); });
        time(out, "power(20) fused", [&] { return cusp::eigen::estimate_spectral_radius(A, 20); });
        time(out, "power(20) generic", [&] { return cusp::eigen::detail::power_iteration(A, 20, std::false_type()); });
        time(out, "ritz(10) fused", [&] { return cusp::eigen::ritz_spectral_radius(A, 10, false); });
        time(out, "ritz(10) generic", [&] { return generic_ritz(false, 10); });
        time(out, "ritz(10,sym) fused", [&] { return cusp::eigen::ritz_spectral_radius(A, 10, true); });
        time(out, "ritz(10,sym) generic", [&] { return generic_ritz(true, 10); });
        time(out, "rho_Dinv_A fused", [&] { return cusp::eigen::estimate_rho_Dinv_A(A); });
        time(out, "rho_Dinv_A generic", [&] { return generic_dinv(); });
    }
};

static double median(std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    return v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]);
}

int main(int argc, char **argv)
{
    size_t grid = 3162;
    int rounds = 5;
    for (int i = 1; i < argc; i++) {
        if (!std::strncmp(argv[i], "--grid=", 7)) grid = std::strtoull(argv[i] + 7, nullptr, 10);
        else if (!std::strncmp(argv[i], "--rounds=", 9)) rounds = std::atoi(argv[i] + 9);
        else { std::fprintf(stderr, "usage: eigen_bench [--grid=3162] [--rounds=5]\n"); return 2; }
    }
    try {
        bench<double> d(grid, "f64");
        bench<float> f(grid, "f32");
        samples out;
        d.round(out); // warm-up round: plans, workspaces, the first launches
        f.round(out);
        std::fprintf(stderr, "warm-up round done\n");
        out.clear();
        for (int r = 0; r < rounds; r++) {
            d.round(out);
            f.round(out);
            std::fprintf(stderr, "round %d of %d done\n", r + 1, rounds);
        }
        const double N = (double)d.A.num_rows, nnz = (double)d.A.num_entries;
        std::printf("eigen_bench: poisson5pt %zu^2 (%.0f rows, %.0f entries), device_memory, %d interleaved rounds; ms = median of the rounds [min, max]\n", grid, N, nnz, rounds);
        const char *names[5] = {"disks", "power(20)", "ritz(10)", "ritz(10,sym)", "rho_Dinv_A"};
        for (const char *tag : {"f64", "f32"})
            for (const char *n : names) {
                const std::vector<double> &a = out[std::string(n) + " fused " + tag], &b = out[std::string(n) + " generic " + tag];
                const std::map<std::string, double> &vals = !std::strcmp(tag, "f64") ? d.values : f.values;
                std::printf("  %-13s %s  fused %9.3f [%9.3f, %9.3f]  generic %9.3f [%9.3f, %9.3f]  generic/fused %5.2f   values %.6f / %.6f\n", n, tag, median(a),
                            *std::min_element(a.begin(), a.end()), *std::max_element(a.begin(), a.end()), median(b), *std::min_element(b.begin(), b.end()),
                            *std::max_element(b.begin(), b.end()), median(b) / median(a), vals.at(std::string(n) + " fused"), vals.at(std::string(n) + " generic"));
            }
        for (const char *tag : {"f64", "f32"}) {
            const std::vector<double> &a = out[std::string("row sums + amax launches (us) ") + tag];
            const double vb = !std::strcmp(tag, "f64") ? 8 : 4, bytes = 4 * (N + 1) + vb * nnz + vb * N + vb * N;
            std::printf("  row sums + amax launches alone %s: %8.2f us [%8.2f, %8.2f]; byte model Ap + Ax + row_sums written + amax read = %.1f MB -> %.2f TB/s = %.2f of 8 TB/s\n",
                        tag, median(a), *std::min_element(a.begin(), a.end()), *std::max_element(a.begin(), a.end()), bytes / 1e6, bytes / median(a) / 1e6,
                        bytes / median(a) / 1e6 / 8.0);
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "eigen_bench: %s\n", e.what());
        return 1;
    }
    return 0;
}

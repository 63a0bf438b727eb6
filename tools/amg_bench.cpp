// tools/amg_bench.cpp -- cusp::precond::aggregation::smoothed_aggregation on device_memory, f64 and f32, on poisson5pt(g, g) for
// every --grids value:
//   amg_bench [--grids=1000,3162] [--rounds=3] [--host=1]
// Per case: the set-up (constructor, stream synchronised) and one V-cycle as the median wall time of the rounds [min, max]; the
// levels; iterations and wall time of cusp::krylov::cg to a relative residual of 1e-8 with this preconditioner and with
// cusp::precond::diagonal of the same build; and (--host=1) the same set-up, cycle and solve through the header layer's
// host_memory path on one core -- the baseline, not the code under test.
#include <cusp/csr_matrix.h>
#include <cusp/gallery/poisson.h>
#include <cusp/krylov/cg.h>
#include <cusp/monitor.h>
#include <cusp/precond/aggregation/smoothed_aggregation.h>
#include <cusp/precond/diagonal.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static void report(const char *what, std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    const double med = v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]);
    std::printf("    %-28s %10.3f ms [%.3f, %.3f] over %zu rounds\n", what, med, v.front(), v.back(), v.size());
}
template <typename Space> void sync(Space) {}
template <> void sync(cusp::device_memory) { cusp::detail::check(cmi_stream_synchronize(nullptr)); }

template <typename V, typename Space> void run(size_t g, int rounds, const char *space)
{
    namespace agg = cusp::precond::aggregation;
    cusp::csr_matrix<int, V, Space> A;
    cusp::gallery::poisson5pt(A, g, g);
    std::printf("  %s %s poisson5pt %zu x %zu: %zu rows, %zu entries\n", space, sizeof(V) == 8 ? "f64" : "f32", g, g, A.num_rows, A.num_entries);
    std::vector<double> setup, cycle;
    agg::smoothed_aggregation<int, V, Space> M;
    for (int r = 0; r < rounds; r++) {
        const double t0 = now_ms();
        M = agg::smoothed_aggregation<int, V, Space>(A);
        sync(Space());
        setup.push_back(now_ms() - t0);
    }
    report("set-up", setup);
    M.print();
    cusp::array1d<V, Space> b(A.num_rows, V(1)), x(A.num_rows, V(0));
    M(b, x); // warm-up: plans
    sync(Space());
    for (int r = 0; r < std::max(rounds, 5); r++) {
        const double t0 = now_ms();
        M(b, x);
        sync(Space());
        cycle.push_back(now_ms() - t0);
    }
    report("V-cycle", cycle);
    {
        cusp::blas::fill(x, V(0));
        cusp::monitor<V> monitor(b, 5000, 1e-8);
        const double t0 = now_ms();
        cusp::krylov::cg(A, x, b, monitor, M);
        sync(Space());
        std::printf("    cg + smoothed_aggregation: %zu iterations, %.3f ms, converged %d\n", monitor.iteration_count(), now_ms() - t0, (int)monitor.converged());
    }
    {
        cusp::precond::diagonal<V, Space> D(A);
        cusp::blas::fill(x, V(0));
        cusp::monitor<V> monitor(b, 20000, 1e-8);
        const double t0 = now_ms();
        cusp::krylov::cg(A, x, b, monitor, D);
        sync(Space());
        std::printf("    cg + diagonal:             %zu iterations, %.3f ms, converged %d\n", monitor.iteration_count(), now_ms() - t0, (int)monitor.converged());
    }
}

int main(int argc, char **argv)
{
    std::vector<size_t> grids = {1000, 3162};
    int rounds = 3, host = 1;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a.rfind("--grids=", 0) == 0) {
            grids.clear();
            for (char *tok = std::strtok(argv[i] + 8, ","); tok; tok = std::strtok(nullptr, ",")) grids.push_back((size_t)std::atol(tok));
        } else if (a.rfind("--rounds=", 0) == 0) rounds = std::atoi(argv[i] + 9);
        else if (a.rfind("--host=", 0) == 0) host = std::atoi(argv[i] + 7);
        else {
            std::fprintf(stderr, "usage: amg_bench [--grids=1000,3162] [--rounds=3] [--host=1]\n");
            return 2;
        }
    }
    std::printf("amg_bench: smoothed aggregation, rounds %d\n", rounds);
    for (size_t g : grids) {
        run<double, cusp::device_memory>(g, rounds, "device");
        run<float, cusp::device_memory>(g, rounds, "device");
        if (host) {
            run<double, cusp::host_memory>(g, 1, "host  ");
            run<float, cusp::host_memory>(g, 1, "host  ");
        }
    }
    return 0;
}

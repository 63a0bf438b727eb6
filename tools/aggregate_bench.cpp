// tools/aggregate_bench.cpp -- the two aggregations of one strength matrix on device_memory, timed in turn in one process:
//   aggregate_bench [--grids=1000,3162] [--rounds=5]
// Per grid g: C = the strength pattern (theta 0) of poisson5pt(g, g), f64, on the device.  Every round times
//   mis_aggregate(C, aggregates, mis)    cmi_csr_mis_aggregate: MIS(2) rounds with one host read each, no copy of the structure
//   standard_aggregate(C, aggregates)    what it replaces: the structure copied to the host, three sequential passes on one core,
//                                        the aggregates copied back
// as host wall time around calls that end synchronised; the median of the rounds with [min, max], the MIS rounds, and both
// aggregate counts.  Run by tools/mis_bench.py, which adds the sweep kernel against its byte model.
#include <cusp/csr_matrix.h>
#include <cusp/gallery/poisson.h>
#include <cusp/graph/maximal_independent_set.h>
#include <cusp/precond/aggregation/aggregate.h>
#include <cusp/precond/aggregation/strength.h>

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
    std::printf("    %-34s %10.3f ms [%.3f, %.3f] over %zu rounds\n", what, med, v.front(), v.back(), v.size());
}
static int count_of(const cusp::array1d<int, cusp::device_memory> &aggregates)
{
    const std::vector<int> h = cusp::detail::host_copy(aggregates);
    return h.empty() ? 0 : *std::max_element(h.begin(), h.end()) + 1;
}

static void run(size_t g, int rounds)
{
    namespace agg = cusp::precond::aggregation;
    typedef cusp::device_memory Dev;
    cusp::csr_matrix<int, double, Dev> A, C;
    cusp::gallery::poisson5pt(A, g, g);
    agg::symmetric_strength_of_connection(A, C, 0.0);
    std::printf("  strength pattern of poisson5pt %zu x %zu: %zu rows, %zu entries\n", g, g, C.num_rows, C.num_entries);
    cusp::array1d<int, Dev> by_mis, by_standard, mis;
    agg::mis_aggregate(C, by_mis, mis); // warm-up: code objects
    agg::standard_aggregate(C, by_standard);
    cusp::detail::check(cmi_stream_synchronize(nullptr));
    std::vector<double> t_mis, t_standard;
    for (int r = 0; r < rounds; r++) {
        double t0 = now_ms();
        agg::mis_aggregate(C, by_mis, mis);
        cusp::detail::check(cmi_stream_synchronize(nullptr));
        t_mis.push_back(now_ms() - t0);
        t0 = now_ms();
        agg::standard_aggregate(C, by_standard);
        cusp::detail::check(cmi_stream_synchronize(nullptr));
        t_standard.push_back(now_ms() - t0);
    }
    size_t mis_rounds = 0;
    cusp::array1d<int, Dev> stencil;
    const size_t set_size = cusp::graph::detail::maximal_independent_set(C, stencil, 2, 0, &mis_rounds);
    report("mis_aggregate (device)", t_mis);
    report("standard_aggregate (host + copies)", t_standard);
    std::printf("    MIS(2): %zu nodes in %zu rounds; aggregates: %d by mis_aggregate, %d by standard_aggregate\n", set_size, mis_rounds, count_of(by_mis),
                count_of(by_standard));
}

int main(int argc, char **argv)
{
    std::vector<size_t> grids = {1000, 3162};
    int rounds = 5;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a.rfind("--grids=", 0) == 0) {
            grids.clear();
            for (char *tok = std::strtok(argv[i] + 8, ","); tok; tok = std::strtok(nullptr, ",")) grids.push_back((size_t)std::atol(tok));
        } else if (a.rfind("--rounds=", 0) == 0) rounds = std::atoi(argv[i] + 9);
        else {
            std::fprintf(stderr, "usage: aggregate_bench [--grids=1000,3162] [--rounds=5]\n");
            return 2;
        }
    }
    std::printf("aggregate_bench: mis_aggregate and standard_aggregate in turn, %d rounds\n", rounds);
    for (size_t g : grids) run(g, rounds);
    return 0;
}

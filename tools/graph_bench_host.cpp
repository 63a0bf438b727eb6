// The host_memory paths of the graph headers on one core, for tools/graph_bench.py: breadth_first_search (levels and
// predecessors), symmetric_rcm and permutation_matrix::symmetric_permute of a CSR pattern read from two raw int32 files.
//   graph_bench_host Ap.bin Aj.bin num_rows src rounds [bfs] [rcm]
// Prints one line per measurement: name, median ms, [min, max], and what identifies the result (depth, reached, bandwidth).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <cusp/csr_matrix.h>
#include <cusp/graph/breadth_first_search.h>
#include <cusp/graph/symmetric_rcm.h>
#include <cusp/permutation_matrix.h>

typedef cusp::host_memory Host;

static std::vector<int> read_ints(const char *path)
{
    std::FILE *f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(2); }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<int> v((size_t)bytes / sizeof(int));
    if (std::fread(v.data(), sizeof(int), v.size(), f) != v.size()) { std::fprintf(stderr, "short read of %s\n", path); std::exit(2); }
    std::fclose(f);
    return v;
}

template <typename F> static void timed(const char *name, int rounds, F &&f, const std::string &what)
{
    std::vector<double> ms;
    for (int r = 0; r < rounds; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        f();
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    std::printf("    %-44s %10.3f ms [%.3f, %.3f] over %d rounds  %s\n", name, ms[ms.size() / 2], ms.front(), ms.back(), rounds, what.c_str());
    std::fflush(stdout);
}

int main(int argc, char **argv)
{
    if (argc < 6) { std::fprintf(stderr, "usage: %s Ap.bin Aj.bin num_rows src rounds [bfs] [rcm]\n", argv[0]); return 2; }
    const std::vector<int> Ap = read_ints(argv[1]), Aj = read_ints(argv[2]);
    const size_t n = (size_t)std::atol(argv[3]);
    const long src = std::atol(argv[4]);
    const int rounds = std::atoi(argv[5]);
    if (Ap.size() != n + 1 || (size_t)Ap[n] != Aj.size()) { std::fprintf(stderr, "the files do not hold a CSR pattern of %zu rows\n", n); return 2; }
    cusp::csr_matrix<int, double, Host> A(n, n, Aj.size());
    std::copy(Ap.begin(), Ap.end(), A.row_offsets.begin());
    std::copy(Aj.begin(), Aj.end(), A.column_indices.begin());
    std::fill(A.values.begin(), A.values.end(), 1.0);
    for (int a = 6; a < argc; a++) {
        if (!std::strcmp(argv[a], "bfs")) {
            cusp::array1d<int, Host> labels;
            size_t reached = 0;
            int depth = 0;
            cusp::graph::detail::breadth_first_search(A, src, labels, true, &reached, &depth);
            const std::string what = "depth " + std::to_string(depth) + ", reached " + std::to_string(reached);
            timed("host breadth_first_search, levels", rounds, [&] { cusp::graph::detail::breadth_first_search(A, src, labels, true, &reached, &depth); }, what);
            timed("host breadth_first_search, predecessors", rounds, [&] { cusp::graph::detail::breadth_first_search(A, src, labels, false, &reached, &depth); }, what);
        } else if (!std::strcmp(argv[a], "rcm")) {
            cusp::permutation_matrix<int, Host> P;
            int vertex = 0;
            timed("host symmetric_rcm", rounds, [&] { vertex = cusp::graph::detail::symmetric_rcm(A, P, src); }, "");
            cusp::csr_matrix<int, double, Host> B;
            timed("host symmetric_permute (CSR in, CSR out)", rounds, [&] { B = A; P.symmetric_permute(B); }, "(includes one copy of the matrix)");
            long band = 0;
            for (size_t i = 0; i < n; i++)
                for (int jj = B.row_offsets[i]; jj < B.row_offsets[i + 1]; jj++) band = std::max(band, std::labs((long)i - (long)B.column_indices[jj]));
            std::printf("    host ordering: pseudo-peripheral vertex %d, bandwidth after %ld\n", vertex, band);
        }
    }
    return 0;
}

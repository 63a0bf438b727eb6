// tools/evolution_bench.cpp -- cusp::precond::aggregation::evolution_strength_of_connection on cusp::gallery::diffusion<FD>(g, g,
// eps 1e-3, angle 0) for every --grids value, f64 and f32:
//   evolution_bench [--grids=1000,3162] [--rounds=5] [--host=1]
// Per case, with rho(D^-1 A) estimated once and supplied to both: the measure on device_memory and on host_memory of the same build
// (one core; the baseline, not the code under test), timed in turn in one process -- host wall time around the synchronising
// calls, median of the rounds [min, max]; and cmi_csr_masked_product_* alone between two HIP events (the call reads the entry
// count back before it launches, so the figure includes one 4-byte host read), with the bytes of its model:
//   streamed once: the offsets, the columns, the two value arrays and the output;
//   gathered:      per entry the columns of its partner row (4 bytes each) and one value of Wx per matched column -- counted
//                  here on the host, reported separately and NOT part of the TB/s figure (neighbouring entries share their
//                  partner rows, so most of it should come from the cache; that is an assumption, not a measurement).
#include <cusp/csr_matrix.h>
#include <cusp/eigen/spectral_radius.h>
#include <cusp/gallery/diffusion.h>
#include <cusp/precond/aggregation/strength.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static double median(std::vector<double> &v)
{
    std::sort(v.begin(), v.end());
    return v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]);
}
static void report(const char *what, std::vector<double> v)
{
    const double med = median(v);
    std::printf("    %-34s %10.3f ms [%.3f, %.3f] over %zu rounds\n", what, med, v.front(), v.back(), v.size());
}

template <typename V> void run(size_t g, int rounds, int host)
{
    namespace agg = cusp::precond::aggregation;
    using cusp::detail::check;
    cusp::csr_matrix<int, V, cusp::host_memory> A, Sh;
    cusp::gallery::diffusion<cusp::gallery::FD>(A, g, g, 1e-3, 0.0);
    cusp::csr_matrix<int, V, cusp::device_memory> dA(A), Sd;
    const cusp::array1d<V, cusp::host_memory> B(A.num_rows, V(1));
    const cusp::array1d<V, cusp::device_memory> dB(B);
    const double rho = cusp::eigen::estimate_rho_Dinv_A(dA);
    std::printf("  %s diffusion<FD> %zu x %zu, eps 1e-3, angle 0: %zu rows, %zu entries, rho(D^-1 A) %.6f\n", sizeof(V) == 8 ? "f64" : "f32", g, g, A.num_rows,
                A.num_entries, rho);
    agg::evolution_strength_of_connection(dA, Sd, dB, rho); // warm-up: code objects
    std::vector<double> device_ms, host_ms;
    for (int r = 0; r < rounds; r++) { // in turn: both see the same drift of the machine
        double t0 = now_ms();
        agg::evolution_strength_of_connection(dA, Sd, dB, rho);
        device_ms.push_back(now_ms() - t0);
        if (host) {
            t0 = now_ms();
            agg::evolution_strength_of_connection(A, Sh, B, rho);
            host_ms.push_back(now_ms() - t0);
        }
    }
    report("measure, device_memory", device_ms);
    if (host) {
        report("measure, host_memory (one core)", host_ms);
        std::printf("    kept entries: device %zu, host %zu; host / device (medians) %.1f\n", Sd.num_entries, Sh.num_entries, median(host_ms) / median(device_ms));
    } else std::printf("    kept entries: device %zu\n", Sd.num_entries);

    // the masked product alone: Vx = the values of A, Wx = the same gathered through the transpose map
    const int64_t n = (int64_t)A.num_rows;
    cusp::array1d<int, cusp::device_memory> tpos(A.num_entries);
    int conforming = 0;
    check(cmi_csr_transpose_positions(n, dA.row_offsets.data(), dA.column_indices.data(), tpos.data(), &conforming, nullptr));
    if (!conforming) throw cusp::runtime_exception("evolution_bench: the generated pattern does not conform");
    std::vector<int> t = cusp::detail::host_copy(tpos);
    cusp::array1d<V, cusp::host_memory> W(A.num_entries);
    double partner_columns = 0, matches = 0;
    for (size_t i = 0; i < A.num_rows; i++)
        for (int e = A.row_offsets[i]; e < A.row_offsets[i + 1]; e++) {
            W[e] = A.values[t[e]];
            const int j = A.column_indices[e];
            partner_columns += A.row_offsets[j + 1] - A.row_offsets[j];
            int p = A.row_offsets[i], q = A.row_offsets[j];
            while (p < A.row_offsets[i + 1] && q < A.row_offsets[j + 1]) {
                const int cp = A.column_indices[p], cq = A.column_indices[q];
                if (cp == cq) { matches++; p++; q++; }
                else if (cp < cq) p++;
                else q++;
            }
        }
    const cusp::array1d<V, cusp::device_memory> dW(W);
    cusp::array1d<V, cusp::device_memory> out(A.num_entries);
    void *start = nullptr, *stop = nullptr;
    check(cmi_event_create(&start));
    check(cmi_event_create(&stop));
    auto product = [&] {
        check(cusp::detail::by_type<V>(cmi_csr_masked_product_f64, cmi_csr_masked_product_f32)(n, dA.row_offsets.data(), dA.column_indices.data(), dA.values.data(), dW.data(),
                                                                                            out.data(), nullptr));
    };
    product(); // warm-up
    std::vector<double> product_ms;
    for (int r = 0; r < rounds; r++) {
        float ms = 0;
        check(cmi_event_record(start, nullptr));
        product();
        check(cmi_event_record(stop, nullptr));
        check(cmi_event_elapsed_ms(start, stop, &ms));
        product_ms.push_back(ms);
    }
    check(cmi_event_destroy(start));
    check(cmi_event_destroy(stop));
    const double streamed = 4.0 * (double)(A.num_rows + 1) + (4.0 + 3.0 * sizeof(V)) * (double)A.num_entries;
    const double gathered = 4.0 * partner_columns + (double)sizeof(V) * matches;
    report("masked product (HIP events)", product_ms);
    std::printf("    streamed %.1f MB => %.3f TB/s at the median; gathered besides (not in that figure): %.1f MB (%.1f partner columns and %.1f matches per entry)\n",
                streamed / 1e6, streamed / (median(product_ms) * 1e-3) / 1e12, gathered / 1e6, partner_columns / (double)A.num_entries, matches / (double)A.num_entries);
}

int main(int argc, char **argv)
{
    std::vector<size_t> grids = {1000, 3162};
    int rounds = 5, host = 1;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a.rfind("--grids=", 0) == 0) {
            grids.clear();
            for (char *tok = std::strtok(argv[i] + 8, ","); tok; tok = std::strtok(nullptr, ",")) grids.push_back((size_t)std::atol(tok));
        } else if (a.rfind("--rounds=", 0) == 0) rounds = std::atoi(argv[i] + 9);
        else if (a.rfind("--host=", 0) == 0) host = std::atoi(argv[i] + 7);
        else {
            std::fprintf(stderr, "usage: evolution_bench [--grids=1000,3162] [--rounds=5] [--host=1]\n");
            return 2;
        }
    }
    std::printf("evolution_bench: evolution strength of connection, rounds %d\n", rounds);
    for (size_t g : grids) {
        run<double>(g, rounds, host);
        run<float>(g, rounds, host);
        std::fflush(stdout);
    }
    return 0;
}

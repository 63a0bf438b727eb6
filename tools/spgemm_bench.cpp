// tools/spgemm_bench.cpp -- the CSR x CSR multiply (cmi_spgemm_csr_* + cmi_spgemm_take_*) on device_memory, f64 and f32:
//   A A on poisson5pt(g, g) for every --grids value, and the Galerkin pair A P, then P^T (A P), on the last grid with the piecewise-constant
//   2 x 2 aggregation (g even).
//   spgemm_bench [--grids=1000,3162] [--rounds=5] [--host-rounds=1] [--workspace=0]
// Per case: the whole device call (create + num_entries + take into arrays sized for it + destroy, stream synchronised) as the median wall
// time of the rounds [min, max], products per second, the scratch model in bytes per product (keys in and out 8 + 8, position 4, segment
// index 4, the value, plus the sort's own temporary storage, which the library does not report), what cmi_spgemm_info returned, and the
// same product through the header layer's host_memory path of the same build on one core (--host-rounds, 0 to skip): what a device user
// had before, to which two copies would be added -- the baseline, not the code under test.  This build has no LDS tile path, so there is
// no tiles-on / tiles-off comparison to interleave.
#include <cusp/csr_matrix.h>
#include <cusp/gallery/poisson.h>
#include <cusp/multiply.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static double median(std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    return v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]);
}

template <typename V> using host_csr = cusp::csr_matrix<int, V, cusp::host_memory>;
template <typename V> using dev_csr = cusp::csr_matrix<int, V, cusp::device_memory>;

// P (N x N / 4, one 1 per row) and its transpose (four 1s per row) for 2 x 2 aggregates on a g x g grid
template <typename V> void aggregation(size_t g, host_csr<V> &P, host_csr<V> &Pt)
{
    const size_t N = g * g, h = g / 2;
    P.resize(N, h * h, N);
    Pt.resize(h * h, N, N);
    for (size_t r = 0; r < N; r++) {
        P.row_offsets[r] = (int)r;
        P.column_indices[r] = (int)((r / g / 2) * h + (r % g) / 2);
        P.values[r] = V(1);
    }
    P.row_offsets[N] = (int)N;
    for (size_t a = 0; a < h * h; a++) {
        const size_t x = 2 * (a % h), y = 2 * (a / h), at = 4 * a;
        const size_t fine[4] = {y * g + x, y * g + x + 1, (y + 1) * g + x, (y + 1) * g + x + 1};
        Pt.row_offsets[a] = (int)at;
        for (int t = 0; t < 4; t++) { Pt.column_indices[at + t] = (int)fine[t]; Pt.values[at + t] = V(1); }
    }
    Pt.row_offsets[h * h] = (int)N;
}

struct call_info { int64_t entries = 0, products = 0, slabs = 0, in_tiles = 0, in_slabs = 0; };

inline int create(int64_t m, int64_t k, int64_t n, int64_t na, const int *Ap, const int *Aj, const double *Ax, int64_t nb, const int *Bp, const int *Bj, const double *Bx, cmi_spgemm **r)
{ return cmi_spgemm_csr_f64(m, k, n, na, Ap, Aj, Ax, nb, Bp, Bj, Bx, r, nullptr); }
inline int create(int64_t m, int64_t k, int64_t n, int64_t na, const int *Ap, const int *Aj, const float *Ax, int64_t nb, const int *Bp, const int *Bj, const float *Bx, cmi_spgemm **r)
{ return cmi_spgemm_csr_f32(m, k, n, na, Ap, Aj, Ax, nb, Bp, Bj, Bx, r, nullptr); }
inline int take(cmi_spgemm *r, int *Cp, int *Cj, double *Cx, int64_t cap) { return cmi_spgemm_take_f64(r, Cp, Cj, Cx, cap, nullptr); }
inline int take(cmi_spgemm *r, int *Cp, int *Cj, float *Cx, int64_t cap) { return cmi_spgemm_take_f32(r, Cp, Cj, Cx, cap, nullptr); }

// the whole device call into C; returns its wall time in ms
template <typename V> double device_call(const dev_csr<V> &A, const dev_csr<V> &B, dev_csr<V> &C, call_info &info)
{
    using cusp::detail::check;
    check(cmi_device_synchronize());
    const double t0 = now_ms();
    cmi_spgemm *h = nullptr;
    check(create((int64_t)A.num_rows, (int64_t)A.num_cols, (int64_t)B.num_cols, (int64_t)A.num_entries, A.row_offsets.data(), A.column_indices.data(), A.values.data(),
                 (int64_t)B.num_entries, B.row_offsets.data(), B.column_indices.data(), B.values.data(), &h));
    check(cmi_spgemm_num_entries(h, &info.entries));
    C.resize(A.num_rows, B.num_cols, (size_t)info.entries);
    check(take(h, C.row_offsets.data(), C.column_indices.data(), C.values.data(), info.entries));
    check(cmi_device_synchronize());
    check(cmi_spgemm_info(h, &info.products, &info.slabs, &info.in_tiles, &info.in_slabs));
    check(cmi_spgemm_destroy(h));
    return now_ms() - t0;
}

template <typename V>
void run_case(const std::string &name, const char *tag, const host_csr<V> &hA, const host_csr<V> &hB, int rounds, int host_rounds, dev_csr<V> *keep = nullptr)
{
    dev_csr<V> A(hA), B(hB), C;
    call_info info;
    device_call(A, B, C, info); // warm-up: code objects, the first allocations
    std::vector<double> ms;
    for (int r = 0; r < rounds; r++) ms.push_back(device_call(A, B, C, info));
    const double med = median(ms), lo = *std::min_element(ms.begin(), ms.end()), hi = *std::max_element(ms.begin(), ms.end());
    std::printf("%-34s %s  %zu x %zu . %zu x %zu  nnz(C) %lld  products %lld  slabs %lld  rows in tiles %lld / slabs %lld\n", name.c_str(), tag, hA.num_rows, hA.num_cols,
                hB.num_rows, hB.num_cols, (long long)info.entries, (long long)info.products, (long long)info.slabs, (long long)info.in_tiles, (long long)info.in_slabs);
    std::printf("    device call  %10.2f ms [%10.2f, %10.2f]   %8.1f M products/s   scratch model %d + sort temp bytes/product\n", med, lo, hi,
                (double)info.products / med / 1e3, (int)(8 + 8 + 4 + 4 + sizeof(V)));
    if (host_rounds > 0) {
        std::vector<double> hs;
        host_csr<V> hC;
        for (int r = 0; r < host_rounds; r++) {
            const double t0 = now_ms();
            cusp::multiply(hA, hB, hC);
            hs.push_back(now_ms() - t0);
        }
        const double hm = median(hs);
        std::printf("    host path    %10.2f ms [%10.2f, %10.2f]   (1 core, %d round%s, nnz %zu with zeros dropped)   host / device %.2f\n", hm, *std::min_element(hs.begin(), hs.end()),
                    *std::max_element(hs.begin(), hs.end()), host_rounds, host_rounds == 1 ? "" : "s", hC.num_entries, hm / med);
    } else {
        std::printf("    host path    not run\n");
    }
    std::fflush(stdout);
    if (keep) *keep = C;
}

template <typename V> void run_type(const char *tag, const std::vector<size_t> &grids, int rounds, int host_rounds)
{
    for (size_t g : grids) {
        host_csr<V> A;
        cusp::gallery::poisson5pt(A, g, g);
        run_case<V>("A A, poisson5pt " + std::to_string(g) + "^2", tag, A, A, rounds, host_rounds);
    }
    const size_t g = grids.back();
    if (g % 2) {
        std::printf("Galerkin pair: not run (grid %zu is odd)\n", g);
        return;
    }
    host_csr<V> A, P, Pt;
    cusp::gallery::poisson5pt(A, g, g);
    aggregation<V>(g, P, Pt);
    dev_csr<V> dAP;
    run_case<V>("Galerkin A P, " + std::to_string(g) + "^2, 2x2 aggregates", tag, A, P, rounds, host_rounds, &dAP);
    host_csr<V> AP(dAP);
    run_case<V>("Galerkin P^T (A P)", tag, Pt, AP, rounds, host_rounds);
}

int main(int argc, char **argv)
{
    std::vector<size_t> grids = {1000, 3162};
    int rounds = 5, host_rounds = 1;
    long long workspace = 0;
    for (int i = 1; i < argc; i++) {
        if (!std::strncmp(argv[i], "--grids=", 8)) {
            grids.clear();
            for (char *p = argv[i] + 8; *p;) {
                grids.push_back(std::strtoull(p, &p, 10));
                if (*p == ',') p++;
            }
        } else if (!std::strncmp(argv[i], "--rounds=", 9)) rounds = std::atoi(argv[i] + 9);
        else if (!std::strncmp(argv[i], "--host-rounds=", 14)) host_rounds = std::atoi(argv[i] + 14);
        else if (!std::strncmp(argv[i], "--workspace=", 12)) workspace = std::atoll(argv[i] + 12);
        else { std::fprintf(stderr, "usage: spgemm_bench [--grids=1000,3162] [--rounds=5] [--host-rounds=1] [--workspace=0]\n"); return 2; }
    }
    if (grids.empty() || rounds < 1) return 2;
    try {
        cusp::detail::check(cmi_spgemm_set_workspace(workspace));
        int64_t T = 0, W = 0;
        cusp::detail::check(cmi_spgemm_limits(&T, &W));
        std::printf("spgemm_bench: device_memory, whole call (cmi_spgemm_csr + take), %d rounds, ms = median [min, max]; tile_products %lld, workspace_products %lld%s\n", rounds,
                    (long long)T, (long long)W, workspace ? "" : " (the default's cap; also bounded by a third of the free memory)");
        run_type<double>("f64", grids, rounds, host_rounds);
        run_type<float>("f32", grids, rounds, host_rounds);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "spgemm_bench: %s\n", e.what());
        return 1;
    }
    return 0;
}

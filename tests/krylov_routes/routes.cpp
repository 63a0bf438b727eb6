// Records which route every Krylov solver of the header layer takes on device_memory, as results: for each (value type, operator form,
// solver) the iteration count, the bits of the monitor's last residual norm and a 64-bit FNV-1a hash of x's bytes, one line per case.
// tests/test_krylov_routes_gpu.py compares the lines with tests/golden/krylov_routes.json bit for bit: the kernels and their launch order
// are fixed, so a different line is a changed route or a changed argument.  Public API only (cusp::detail::forced_config() is what
// cusp::ktt::tune sets), so the same source builds against any revision of the headers.
//
// The system: poisson5pt(33, 31), N = 1023 (every format's kernel has full and partial tiles), b = ones, x0 = 0, monitor (b, 30, 1e-30):
// every case runs exactly 30 iterations.  $CMI_CG_FOLD_AHEAD is not set here.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include <cusp/coo_matrix.h>
#include <cusp/csr_matrix.h>
#include <cusp/dia_matrix.h>
#include <cusp/ell_matrix.h>
#include <cusp/gallery/poisson.h>
#include <cusp/hyb_matrix.h>
#include <cusp/krylov/bicgstab.h>
#include <cusp/krylov/bicgstab_m.h>
#include <cusp/krylov/cg.h>
#include <cusp/krylov/cg_m.h>
#include <cusp/krylov/cr.h>
#include <cusp/krylov/gmres.h>
#include <cusp/linear_operator.h>
#include <cusp/monitor.h>
#include <cusp/precond/diagonal.h>

template <typename V> using hcsr = cusp::csr_matrix<int, V, cusp::host_memory>;
template <typename V> using dcsr = cusp::csr_matrix<int, V, cusp::device_memory>;
template <typename V> using dvec = cusp::array1d<V, cusp::device_memory>;
template <typename V> using jacobi = cusp::precond::diagonal<V, cusp::device_memory>;

template <typename V> const char *type_name() { return sizeof(V) == 8 ? "f64" : "f32"; }

static uint64_t fnv1a(const void *p, size_t bytes)
{
    uint64_t h = 14695981039346656037ull;
    for (size_t i = 0; i < bytes; i++) h = (h ^ static_cast<const unsigned char *>(p)[i]) * 1099511628211ull;
    return h;
}
template <typename V> unsigned long long bits_of(V v)
{
    typename std::conditional<sizeof(V) == 8, uint64_t, uint32_t>::type u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

// a linear operator WITHOUT a format tag that forwards to the CSR multiply
template <typename V> struct csr_operator : cusp::linear_operator<V, cusp::device_memory> {
    const dcsr<V> &A;
    explicit csr_operator(const dcsr<V> &a) : cusp::linear_operator<V, cusp::device_memory>(a.num_rows, a.num_cols, a.num_entries), A(a) {}
    template <typename X, typename Y> void operator()(const X &x, Y &y) const { cusp::multiply(A, x, y); }
};

// one case: solve(x, b, monitor) from x0 = 0 with b = ones; x holds `shifts` solutions (a shift with a non-finite value prints "-")
template <typename V, typename Solve> void record(const std::string &form, const char *solver, size_t N, size_t shifts, Solve solve)
{
    const dvec<V> b(N, V(1));
    dvec<V> x(N * shifts, V(0));
    cusp::monitor<V> monitor(b, 30, V(1e-30));
    solve(x, b, monitor);
    const cusp::array1d<V, cusp::host_memory> h(x);
    std::printf("%s/%s/%s %zu %llx", type_name<V>(), form.c_str(), solver, monitor.iteration_count(), bits_of(monitor.residual_norm()));
    for (size_t s = 0; s < shifts; s++) {
        bool finite = true;
        for (size_t i = 0; i < N; i++) finite = finite && std::isfinite(h[s * N + i]);
        if (finite) std::printf(" %016llx", (unsigned long long)fnv1a(h.data() + s * N, N * sizeof(V)));
        else std::printf(" -");
    }
    std::printf("\n");
    std::fflush(stdout);
}

struct env_switch { // NAME=0 for the length of one case
    const char *name;
    explicit env_switch(const char *n) : name(n) { setenv(name, "0", 1); }
    ~env_switch() { unsetenv(name); }
};

template <typename V> dvec<V> the_shifts()
{
    cusp::array1d<V, cusp::host_memory> s(2);
    s[0] = V(0.1);
    s[1] = V(1);
    return dvec<V>(s);
}

// the five solvers every operator form runs; M is the Jacobi preconditioner of the same matrix
template <typename V, typename Operator> void run_form(const std::string &form, const Operator &A, const jacobi<V> &M)
{
    const size_t N = A.num_rows;
    const dvec<V> sigma = the_shifts<V>();
    record<V>(form, "cg", N, 1, [&](dvec<V> &x, const dvec<V> &b, cusp::monitor<V> &m) { cusp::krylov::cg(A, x, b, m); });
    record<V>(form, "cg_jacobi", N, 1, [&](dvec<V> &x, const dvec<V> &b, cusp::monitor<V> &m) { cusp::krylov::cg(A, x, b, m, M); });
    record<V>(form, "cr", N, 1, [&](dvec<V> &x, const dvec<V> &b, cusp::monitor<V> &m) { cusp::krylov::cr(A, x, b, m); });
    record<V>(form, "bicgstab", N, 1, [&](dvec<V> &x, const dvec<V> &b, cusp::monitor<V> &m) { cusp::krylov::bicgstab(A, x, b, m); });
    record<V>(form, "cg_m", N, 2, [&](dvec<V> &x, const dvec<V> &b, cusp::monitor<V> &m) { cusp::krylov::cg_m(A, x, b, sigma, m); });
}

template <typename V> hcsr<V> with_arrow(const hcsr<V> &H) // + 20 entries of -0.01 in row 0 and 20 in column 0 (columns / rows 2..21): still diagonally dominant
{
    struct entry { int i, j; V v; };
    std::vector<entry> e;
    for (size_t i = 0; i < H.num_rows; i++) {
        if (i >= 2 && i < 22) e.push_back({(int)i, 0, V(-0.01)});
        for (int jj = H.row_offsets[i]; jj < H.row_offsets[i + 1]; jj++) {
            e.push_back({(int)i, H.column_indices[jj], H.values[jj]});
            if (i == 0 && H.column_indices[jj] == 1)
                for (int j = 2; j < 22; j++) e.push_back({0, j, V(-0.01)});
        }
    }
    cusp::coo_matrix<int, V, cusp::host_memory> C(H.num_rows, H.num_cols, e.size());
    for (size_t k = 0; k < e.size(); k++) { C.row_indices[k] = e[k].i; C.column_indices[k] = e[k].j; C.values[k] = e[k].v; }
    return hcsr<V>(C);
}

template <typename V> void run_type()
{
    hcsr<V> H;
    cusp::gallery::poisson5pt(H, 33, 31);
    const size_t N = H.num_rows;
    if (N != 1023) throw std::runtime_error("poisson5pt(33, 31) is not 1023 x 1023");
    const dcsr<V> A(H);
    const jacobi<V> M(A);
    const dvec<V> sigma = the_shifts<V>();

    run_form<V>("csr_plan", A, M);
    {
        cmi_config stream = {};
        stream.kernel = CMI_CSR_STREAM;
        cusp::detail::forced_config() = &stream; // no plan: the entry points that take a configuration
        try { run_form<V>("csr_forced_config", A, M); } catch (...) { cusp::detail::forced_config() = nullptr; throw; }
        cusp::detail::forced_config() = nullptr;
    }
    run_form<V>("coo", cusp::coo_matrix<int, V, cusp::device_memory>(A), M);
    run_form<V>("ell", cusp::ell_matrix<int, V, cusp::device_memory>(A), M);
    run_form<V>("dia", cusp::dia_matrix<int, V, cusp::device_memory>(A), M);
    {
        const cusp::hyb_matrix<int, V, cusp::device_memory> Y(A);
        if (Y.coo.num_entries != 0) throw std::runtime_error("hyb_matrix(poisson5pt) has a COO part");
        run_form<V>("hyb_ell_only", Y, M);
    }
    {
        const dcsr<V> B(with_arrow(H));
        const cusp::hyb_matrix<int, V, cusp::device_memory> Y(B);
        if (Y.coo.num_entries == 0) throw std::runtime_error("hyb_matrix(poisson5pt + arrow) has no COO part");
        run_form<V>("hyb_arrow", Y, jacobi<V>(B));
    }
    // (cusp::array2d has no matrix-vector multiply on device_memory: it is no operator form here)
    run_form<V>("operator", csr_operator<V>(A), M);

    // CSR only: the solvers without a fused iteration, and each fused solver with its switch off
    record<V>("csr_plan", "bicgstab_m", N, 2, [&](dvec<V> &x, const dvec<V> &b, cusp::monitor<V> &m) { cusp::krylov::bicgstab_m(A, x, b, sigma, m); });
    record<V>("csr_plan", "gmres5", N, 1, [&](dvec<V> &x, const dvec<V> &b, cusp::monitor<V> &m) { cusp::krylov::gmres(A, x, b, 5, m); });
    {
        env_switch off("CMI_CG_FUSED_JACOBI");
        record<V>("csr_plan", "cg_jacobi,CMI_CG_FUSED_JACOBI=0", N, 1, [&](dvec<V> &x, const dvec<V> &b, cusp::monitor<V> &m) { cusp::krylov::cg(A, x, b, m, M); });
    }
    {
        env_switch off("CMI_CR_FUSED");
        record<V>("csr_plan", "cr,CMI_CR_FUSED=0", N, 1, [&](dvec<V> &x, const dvec<V> &b, cusp::monitor<V> &m) { cusp::krylov::cr(A, x, b, m); });
    }
    {
        env_switch off("CMI_BICGSTAB_FUSED");
        record<V>("csr_plan", "bicgstab,CMI_BICGSTAB_FUSED=0", N, 1, [&](dvec<V> &x, const dvec<V> &b, cusp::monitor<V> &m) { cusp::krylov::bicgstab(A, x, b, m); });
    }
    {
        env_switch off("CMI_CG_M_FUSED");
        record<V>("csr_plan", "cg_m,CMI_CG_M_FUSED=0", N, 2, [&](dvec<V> &x, const dvec<V> &b, cusp::monitor<V> &m) { cusp::krylov::cg_m(A, x, b, sigma, m); });
    }
}

int main()
{
    try { // the first failure ends the program: nothing more is launched behind it
        run_type<double>();
        run_type<float>();
    } catch (const std::exception &e) {
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    std::printf("done\n");
    return 0;
}

// The AINV preconditioners on device_memory (built and run once by tests/test_ainv_gpu.py): the reference's three tests in float and double, the
// factors and the apply against host_memory bit for bit -- through the scaled plan and through the three steps --, cusp::multiply(M.w) untouched by
// the second plan, cg through the fused branch and through cg_plain, and the four solves of the reference's example.
#include "ainv_check.h"

using namespace ainv_check;
namespace precond = cusp::precond;
typedef cusp::device_memory D;
typedef cusp::host_memory H;

template <typename V> void TestFactorization() { exact_factorisation_case<V, D>(); }
template <typename V> void TestSymmetry() { symmetry_case<V, D>(); }
template <typename V> void TestConvergence()
{
    convergence_cases<V, D, precond::scaled_bridson_ainv>("scaled_bridson_ainv");
    convergence_cases<V, D, precond::bridson_ainv>("bridson_ainv");
}
void TestAINVFactorizationF32() { TestFactorization<float>(); }
void TestAINVFactorizationF64() { TestFactorization<double>(); }
void TestAINVSymmetryF32() { TestSymmetry<float>(); }
void TestAINVSymmetryF64() { TestSymmetry<double>(); }
void TestAINVConvergenceF32() { TestConvergence<float>(); }
void TestAINVConvergenceF64() { TestConvergence<double>(); }
DECLARE_UNITTEST(TestAINVFactorizationF32);
DECLARE_UNITTEST(TestAINVFactorizationF64);
DECLARE_UNITTEST(TestAINVSymmetryF32);
DECLARE_UNITTEST(TestAINVSymmetryF64);
DECLARE_UNITTEST(TestAINVConvergenceF32);
DECLARE_UNITTEST(TestAINVConvergenceF64);

// NaNs aside (none arise here), bit for bit
template <typename V, typename A, typename B> bool same_array(const A &a, const B &b)
{
    const cusp::array1d<V, H> x(a), y(b);
    if (x.size() != y.size()) return false;
    for (size_t i = 0; i < x.size(); i++)
        if (bits_of<V>(x[i]) != bits_of<V>(y[i])) return false;
    return true;
}
template <typename V, typename MA, typename MB> bool same_matrix(const MA &a, const MB &b)
{
    const host_csr<V> x(a), y(b);
    return x.num_rows == y.num_rows && x.num_entries == y.num_entries && x.row_offsets == y.row_offsets && x.column_indices == y.column_indices &&
           same_array<V>(x.values, y.values);
}

// y = M x on the device against the host class, both routes where there are two; then cusp::multiply(first factor) must still be the plain product
template <typename V, bool HasScale, typename Dev, typename Host, typename Hyb, typename HostHyb> void check_apply(Dev &Md, const Host &Mh, const Hyb &first, const HostHyb &first_host)
{
    const size_t n = Mh.num_rows;
    const cusp::array1d<V, H> xh = start_vector<V, H>(n);
    const cusp::array1d<V, D> xd(xh);
    cusp::array1d<V, H> yh(n);
    cusp::array1d<V, D> yd(n);
    Mh(xh, yh);
    Md(xd, yd);
    ASSERT_TRUE(same_array<V>(yd, yh));
    if constexpr (HasScale) {
        // the plan takes the scale exactly where it multiplies in one launch: a COO part of at most three entries per row on average (no tile of
        // these small factors comes near the per-tile ceiling)
        const bool light = first.coo.num_entries <= 3 * n;
        std::printf("  %zu rows, ELL width %zu, %zu COO entries: %s\n", n, (size_t)first.ell.column_indices.num_cols, (size_t)first.coo.num_entries,
                    Md.row_scale_in_use() ? "scaled plan" : "three steps");
        ASSERT_EQUAL(Md.row_scale_in_use(), light);
        Md.row_scale_route = false;
        cusp::blas::fill(yd, V(-7));
        Md(xd, yd);
        ASSERT_TRUE(!Md.row_scale_in_use());
        ASSERT_TRUE(same_array<V>(yd, yh));
        Md.row_scale_route = true;
        Md(xd, yd);
        ASSERT_EQUAL(Md.row_scale_in_use(), light);
        ASSERT_TRUE(same_array<V>(yd, yh));
    }
    cusp::multiply(first_host, xh, yh);
    cusp::multiply(first, xd, yd);
    ASSERT_TRUE(same_array<V>(yd, yh));
}
template <typename V> void TestDeviceEqualsHost()
{
    const host_csr<V> Ah = problem<host_csr<V>>(33, 31), Bh = nonsymmetric_problem<V>(7, 5);
    const cusp::csr_matrix<int, V, D> Ad(Ah), Bd(Bh);
    for (const setting &s : settings()) {
        {
            const precond::scaled_bridson_ainv<V, H> h(Ah, (V)s.tol, s.per_row, s.lin, s.lin_param);
            precond::scaled_bridson_ainv<V, D> d(Ad, (V)s.tol, s.per_row, s.lin, s.lin_param);
            ASSERT_TRUE(same_matrix<V>(d.w, h.w) && same_matrix<V>(d.w_t, h.w_t));
            check_apply<V, false>(d, h, d.w, h.w);
        }
        {
            const precond::bridson_ainv<V, H> h(Ah, (V)s.tol, s.per_row, s.lin, s.lin_param);
            precond::bridson_ainv<V, D> d(Ad, (V)s.tol, s.per_row, s.lin, s.lin_param);
            ASSERT_TRUE(same_matrix<V>(d.w, h.w) && same_matrix<V>(d.w_t, h.w_t) && same_array<V>(d.diagonals, h.diagonals));
            check_apply<V, true>(d, h, d.w, h.w);
            precond::bridson_ainv<V, D> copy(d); // a copy owns its diagonals: its plan must carry ITS array
            check_apply<V, true>(copy, h, copy.w, h.w);
        }
        for (int which = 0; which < 2; which++) {
            const precond::nonsym_bridson_ainv<V, H> h(which ? Bh : Ah, (V)s.tol, s.per_row, s.lin, s.lin_param);
            precond::nonsym_bridson_ainv<V, D> d(which ? Bd : Ad, (V)s.tol, s.per_row, s.lin, s.lin_param);
            ASSERT_TRUE(same_matrix<V>(d.z, h.z) && same_matrix<V>(d.w_t, h.w_t) && same_array<V>(d.diagonals, h.diagonals));
            check_apply<V, true>(d, h, d.z, h.z);
        }
    }
}
void TestDeviceEqualsHostF32() { TestDeviceEqualsHost<float>(); }
void TestDeviceEqualsHostF64() { TestDeviceEqualsHost<double>(); }
DECLARE_UNITTEST(TestDeviceEqualsHostF32);
DECLARE_UNITTEST(TestDeviceEqualsHostF64);

// cg through the fused branch and, with CMI_CG_FUSED_AINV=0, through cg_plain: both within the reference's limit; the device matrix in two formats
template <typename V, typename Matrix> void fused_and_plain()
{
    const Matrix A = problem<Matrix>(100, 100);
    precond::bridson_ainv<V, D> M1(A, 0, 10);
    precond::scaled_bridson_ainv<V, D> M2(A, 0, 10);
    precond::nonsym_bridson_ainv<V, D> M3(A, 0, 10);
    for (int plain = 0; plain < 2; plain++) {
        setenv("CMI_CG_FUSED_AINV", plain ? "0" : "1", 1);
        const solve_result r1 = solve<V, D>(A, M1, 70), r2 = solve<V, D>(A, M2, 70), r3 = solve<V, D>(A, M3, 70);
        std::printf("%s cg, limit 70: bridson %zu, scaled %zu, nonsym %zu iterations\n", plain ? "plain" : "fused", r1.iterations, r2.iterations, r3.iterations);
        ASSERT_TRUE(r1.converged && r2.converged && r3.converged);
    }
    unsetenv("CMI_CG_FUSED_AINV");
}
void TestFusedAndPlainCg()
{
    fused_and_plain<float, cusp::csr_matrix<int, float, D>>();
    fused_and_plain<double, cusp::csr_matrix<int, double, D>>();
    fused_and_plain<double, cusp::hyb_matrix<int, double, D>>();
}
DECLARE_UNITTEST(TestFusedAndPlainCg);

// the four solves of the reference's example (examples/Preconditioners/ainv.cu): poisson5pt 256 x 256 as coo_matrix in float, b = 1, x0 = 0, the
// default monitor; all converge and every preconditioned solve takes fewer iterations than the plain one
void TestExampleSolves()
{
    typedef cusp::coo_matrix<int, float, D> Matrix;
    Matrix A;
    cusp::gallery::poisson5pt(A, 256, 256);
    const cusp::array1d<float, D> x0(A.num_rows, 0), b(A.num_rows, 1);
    cusp::monitor<float> monitor(b);
    size_t plain = 0;
    {
        cusp::array1d<float, D> x(x0);
        cusp::krylov::cg(A, x, b, monitor);
        ASSERT_TRUE(monitor.converged());
        plain = monitor.iteration_count();
    }
    auto run = [&](auto &M, const char *what) {
        cusp::array1d<float, D> x(x0);
        monitor.reset(b);
        cusp::krylov::cg(A, x, b, monitor, M);
        std::printf("example: %s %zu iterations (no preconditioner: %zu)\n", what, monitor.iteration_count(), plain);
        ASSERT_TRUE(monitor.converged());
        ASSERT_TRUE(monitor.iteration_count() < plain);
    };
    { precond::scaled_bridson_ainv<float, D> M(A, .1); run(M, "scaled_bridson_ainv(.1)"); }
    { precond::scaled_bridson_ainv<float, D> M(A, 0, 10); run(M, "scaled_bridson_ainv(0, 10)"); }
    { precond::bridson_ainv<float, D> M(A, 0, -1, true, 2); run(M, "bridson_ainv(0, -1, true, 2)"); }
}
DECLARE_UNITTEST(TestExampleSolves);

// the refusals reach the device classes too
void TestDeviceRefusals()
{
    cusp::csr_matrix<int, double, H> S(2, 2, 4);
    S.row_offsets[0] = 0; S.row_offsets[1] = 2; S.row_offsets[2] = 4;
    for (int e = 0; e < 4; e++) { S.column_indices[e] = e % 2; S.values[e] = 1; }
    const cusp::csr_matrix<int, double, D> Sd(S);
    ASSERT_THROWS((precond::bridson_ainv<double, D>(Sd, 0)), cusp::invalid_input_exception);
    ASSERT_THROWS((precond::scaled_bridson_ainv<double, D>(Sd, 0)), cusp::invalid_input_exception);
}
DECLARE_UNITTEST(TestDeviceRefusals);

int main(int argc, char **argv) { return unittest::run_all(argc, argv); }

// cusp/eigen/lanczos.h -- cusp::eigen::lanczos(A, eigVals, eigVecs[, options]): several extreme eigenpairs of a symmetric operator by the Lanczos
// process with optional full reorthogonalisation (reference cusp/eigen/lanczos.h, detail/lanczos.inl, detail/gram_schmidt.inl,
// lanczos_options.h).  eigVals.size() is the number of eigenvalues wanted; options.eigPart chooses the smallest (SA), the largest (LA) or both
// ends (BE: wanted / 2 at the low end, the rest at the high end).  On exit eigVals holds the values FOUND -- the low end ascending, then the
// high end ascending -- and is resized to their count; with options.computeEigVecs, eigVecs (column_major, in A's memory space) is resized to
// N x found and holds the Ritz vectors E = V S in the same order.  A is any of the five formats or a cusp::linear_operator, in either space.
//
// The algorithm is the reference's: the option defaults and the min / max iteration rules; the three-term step; the convergence test every
// `stride` steps from `minIter` on -- the relative change of the SUM of the wanted Ritz values between T_iter and T_iter+1 against `tol`, at
// both ends -- confirmed by a second test `extraIter` steps later; with reorth == Full, modified Gram-Schmidt of the new vector against the
// stored ones, repeated when the norm dropped below doubleReorthGamma times what it was (always when doubleReorthGamma >= 1); a restart from
// a fresh random vector when the new norm is below betaSum * eps, with beta stored as 0.  When that vector too has norm exactly 0 after its
// orthogonalisation (N = 1; the vectors kept span the space) the loop ends with that step -- the reference divides by the norm.
//
// Departures from the reference, all deliberate:
//   (a) Index ranges.  The reference writes subarray(first, last) where its own array1d::subarray takes (start, num_entries); its loops
//       (ritzVal[iter], ritzVal0[iter - 1]) assume the inclusive reading, which is what is implemented: at step iter (0-based, alphas[iter]
//       known) ritzVal0 are the eigenvalues of T_iter (alphas[0 .. iter - 1], betas[0 .. iter - 2]) and ritzVal those of T_iter+1; after the
//       loop, T_m with m = the final iter.  A test that would index past the iter values T_iter has (a wanted count on one side > iter) is
//       skipped, not run out of range.  The wanted count is clipped to N in both reorthogonalisation modes, and when the loop ends
//       unconverged with fewer steps than wanted values the two ends share the m values there are (the low end first).
//   (b) Full means ALL stored vectors.  The reference's modifiedGramSchmidt starts at max(num_cols - 10, 0), with `start = 0` commented out
//       beside it, while its own counters assume every column.  The window of ten loses orthogonality in float to the point of returning a
//       Ritz pair twice (tests/test_lanczos_refs.py keeps that variant as a mutant, with figures).
//   (c) V is kept whenever it is needed: with reorth == Full OR computeEigVecs (the reference allocates it with Full only and, with
//       computeEigVecs and None, multiplies an empty V).  A restart with nothing stored orthogonalises the new vector against v0 and v1 only.
//   (d) The restart vector.  The reference draws random_array<T>(N) again with its default seed -- the start vector itself.  Here restart
//       number r = 1, 2, ... draws cusp::random_array<T>(N, r): the start vector's seed (0) + r, the same bits in both memory spaces.
//   (e) Every normalisation multiplies by T(1) / T(norm), formed once in T (cmi_blas_scal_recip_*'s rule), as in lobpcg.h.
//   (f) cusp::lapack::stev is replaced by cusp/detail/tridiagonal_eigen.h (implicit QL in double, no LAPACK); when it does not converge,
//       lanczos throws runtime_exception.  The reference's shape asserts throw invalid_input_exception; eigVecs must be column_major and
//       live in A's memory space.
//   (g) options.verbose prints the same quantities as the reference; none of its text is part of the contract.
//
// Two paths:
//   plain  any memory space, any value type: operation by operation through cusp::multiply and cusp::blas, with three work vectors and a
//          copy of v1 into V per step.  On device_memory a step without reorthogonalisation is the multiply, 5 cusp::blas calls (6 with the
//          copy into V) and 2 host reads (dot, nrm2); Full adds 2 (iter + 1) + 1 calls and iter + 2 host reads per Gram-Schmidt pass.
//   fused  device_memory, float or double ($CMI_LANCZOS_FUSED=0 selects plain).  When V is kept the step runs INSIDE V's columns -- v0, v1
//          and w are columns iter - 1, iter and iter + 1, nothing is copied -- otherwise in three rotating vectors.  The coefficients stay in
//          device memory (cmi_blas_axpy_dot_*, cmi_blas_scal_recip_*, as cusp::eigen::arnoldi):
//            None  the multiply, w -= beta v0 with alpha = <v1, w>, w -= alpha v1 with <w, w>, the normalise launch: 1 + 3 launches and ONE
//                  host read (alpha and the norm's square; the restart test is made on them).
//            Full  the multiply, the same two launches, then the Gram-Schmidt chain over the iter + 1 stored columns (iter + 2 launches: the
//                  first dot has no axpy in front, the last axpy carries the norm's square), queued BEFORE the step's one host read -- alpha
//                  and both squared norms together, which decide the doubling and the restart -- and the normalise launch: iter + 6 launches
//                  and ONE host read; a doubled pass adds iter + 2 launches and one read.  The chain is not queued on the step that ends at
//                  maxIter.
//          The Ritz vectors are one cusp::blas::gemm on the device (csrc/dense.hip), the selected columns of S copied down once.
//          Growing V by memoryExpansionFactor copies the stored columns and changes no result.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <iomanip>
#include <iostream>
#include <limits>
#include <type_traits>
#include <vector>

#include "../array1d.h"
#include "../array2d.h"
#include "../blas/blas.h"
#include "../copy.h"
#include "../detail/tridiagonal_eigen.h"
#include "../multiply.h"
#include "arnoldi.h" // device_coefficients
#include "lanczos_options.h"

namespace cusp {
namespace eigen {
namespace detail {
namespace lanczos_detail {

// what the last call of this thread did (the reference only prints it): steps taken, whether the confirming convergence test passed, restarts
struct run_info { size_t iterations; bool converged; size_t restarts; };
inline run_info &last_run()
{
    static thread_local run_info info = {0, false, 0};
    return info;
}

// the pitch of V: N rounded up so that every column starts on the 16-byte grid the device kernels' wide accesses need (cmi_dense_gemm_*, the
// cmi_blas_axpy_dot_* chain); the padding is never read or written, so no result changes.  Types that do not tile 16 bytes keep N.
template <typename T> size_t column_pitch(size_t N)
{
    const size_t per = 16 % sizeof(T) == 0 ? 16 / sizeof(T) : 1;
    return (N + per - 1) / per * per;
}

// the vectors of the process, operation by operation (any memory space, any value type)
template <typename LinearOperator> class plain_engine {
public:
    typedef typename LinearOperator::value_type T;
    typedef typename LinearOperator::memory_space Space;
    typedef cusp::array1d_view<T, Space> View;

    plain_engine(const LinearOperator &A_, bool keep) : A(A_), N(A_.num_cols), keep_v(keep), v0(N, T(0)), v1(N), v2(N), bb_prev(0)
    {
        cusp::copy(cusp::random_array<T>(N), v1);
        cusp::blas::scal(v1, T(1) / T(cusp::blas::nrm2(v1)));
    }
    void reserve(size_t columns) { if (keep_v) V.resize(N, columns, column_pitch<T>(N)); }
    // v2 <- A v1 - bb v0; aa = <v1, v2>; v2 <- v2 - aa v1; bb = ||v2||
    void step(size_t iter, bool, T &aa, T &bb)
    {
        if (keep_v) { View column = V.column(iter); cusp::blas::copy(v1, column); }
        cusp::multiply(A, v1, v2);
        if (iter > 0) cusp::blas::axpy(v0, v2, -bb_prev);
        aa = cusp::blas::dot(v1, v2);
        cusp::blas::axpy(v1, v2, -aa);
        bb = cusp::blas::nrm2(v2);
    }
    // modified Gram-Schmidt against the iter + 1 stored vectors, once more when the norm dropped below gamma x what it was
    T reorthogonalise(size_t iter, T bb_old, T gamma, bool &doubled)
    {
        gram_schmidt(iter + 1);
        T bb = cusp::blas::nrm2(v2);
        doubled = gamma >= T(1) || bb < gamma * bb_old;
        if (doubled) {
            gram_schmidt(iter + 1);
            bb = cusp::blas::nrm2(v2);
        }
        return bb;
    }
    T restart(size_t iter, size_t number)
    {
        cusp::copy(cusp::random_array<T>(N, number), v2);
        if (keep_v) gram_schmidt(iter + 1);
        else {
            if (iter > 0) against(v0);
            against(v1);
        }
        return cusp::blas::nrm2(v2);
    }
    void normalise(size_t, T bb)
    {
        cusp::blas::scal(v2, T(1) / T(bb));
        v0.swap(v1); // [v0 v1 v2] -> [v1 v2 v0]
        v1.swap(v2);
        bb_prev = bb;
    }
    template <typename Array2d> void ritz_vectors(size_t m, const cusp::array2d<T, cusp::host_memory, cusp::column_major> &S_host, Array2d &eigVecs)
    {
        const cusp::array2d<T, Space, cusp::column_major> S(S_host);
        cusp::blas::gemm(V.columns(0, m), S, eigVecs);
    }
    void finish() {}

private:
    template <typename X> void against(const X &q)
    {
        const T d = cusp::blas::dot(q, v2);
        cusp::blas::axpy(q, v2, -d);
    }
    void gram_schmidt(size_t columns)
    {
        for (size_t i = 0; i < columns; i++) against(V.column(i));
    }
    const LinearOperator &A;
    size_t N;
    bool keep_v;
    cusp::array2d<T, Space, cusp::column_major> V;
    cusp::array1d<T, Space> v0, v1, v2;
    T bb_prev;
};

// device_memory, float / double: the schedule at the head of this file.  Column j of the process lives in V's column j when V is kept, in
// slot j mod 3 of three vectors otherwise; v0, v1, w are columns iter - 1, iter, iter + 1.
// Device scalars c: [0] alpha  [1] <w, w> behind the three-term step  [2] <w, w> behind a Gram-Schmidt chain  [3] beta, as the normalise
// launch leaves it for the next step  [4 ...] the coefficients of a chain.
template <typename LinearOperator> class fused_engine {
public:
    typedef typename LinearOperator::value_type T;
    typedef cusp::array1d_view<T, cusp::device_memory> View;

    fused_engine(const LinearOperator &A_, bool keep, size_t max_columns)
        : A(A_), N(A_.num_cols), keep_v(keep), ws(cusp::blas::detail::workspace()), c(cusp::eigen::detail::device_coefficients(max_columns + 8)), final_ww(c + 1),
          chain_ww(0), chain_done(false)
    {
        if (!keep_v) V.resize(N, 3, column_pitch<T>(N));
    }
    void reserve(size_t columns)
    {
        if (!keep_v) return;
        const bool first = V.num_cols == 0;
        V.resize(N, columns + 1, column_pitch<T>(N)); // w of the last step is column `columns`
        if (first) start();
    }
    void step(size_t iter, bool reorthogonalisation_follows, T &aa, T &bb)
    {
        if (!keep_v && iter == 0) start();
        View x(column(iter), N), y(column(iter + 1), N);
        cusp::multiply(A, x, y);
        axpy_dot(iter > 0 ? c + 3 : nullptr, iter > 0 ? column(iter - 1) : y.data(), y.data(), x.data(), c);
        axpy_dot(c, x.data(), y.data(), y.data(), c + 1);
        chain_done = reorthogonalisation_follows;
        if (chain_done) chain(iter, iter + 1);
        double host[3] = {0.0, 0.0, 0.0};
        cusp::detail::check(cmi_memcpy_d2h(host, c, (chain_done ? 3 : 2) * sizeof(double), nullptr)); // the step's one host read
        aa = static_cast<T>(host[0]);
        bb = static_cast<T>(std::sqrt(host[1]));
        chain_ww = host[2];
        final_ww = c + 1;
    }
    T reorthogonalise(size_t iter, T bb_old, T gamma, bool &doubled)
    {
        if (!chain_done) chain_ww = chain_and_read(iter, iter + 1);
        T bb = static_cast<T>(std::sqrt(chain_ww));
        doubled = gamma >= T(1) || bb < gamma * bb_old;
        if (doubled) bb = static_cast<T>(std::sqrt(chain_and_read(iter, iter + 1)));
        final_ww = c + 2;
        return bb;
    }
    T restart(size_t iter, size_t number)
    {
        cusp::detail::check(cusp::detail::by_type<T>(cmi_random_fill_f64, cmi_random_fill_f32)(N, number, column(iter + 1), nullptr));
        // everything stored, or v0 and v1 alone: the columns first .. iter
        const size_t first = keep_v ? 0 : (iter > 0 ? iter - 1 : iter);
        const double ww = chain_and_read(iter, iter + 1 - first, first);
        final_ww = c + 2;
        return static_cast<T>(std::sqrt(ww));
    }
    void normalise(size_t iter, T)
    {
        cusp::detail::check(cusp::detail::by_type<T>(cmi_blas_scal_recip_f64, cmi_blas_scal_recip_f32)(N, final_ww, 1, column(iter + 1), c + 3, nullptr));
    }
    template <typename Array2d> void ritz_vectors(size_t m, const cusp::array2d<T, cusp::host_memory, cusp::column_major> &S_host, Array2d &eigVecs)
    {
        const cusp::array2d<T, cusp::device_memory, cusp::column_major> S(S_host); // copied down once
        cusp::blas::gemm(V.columns(0, m), S, eigVecs);
    }
    void finish() { cusp::detail::check(cmi_device_synchronize()); } // nothing queued may outlive the temporaries

private:
    T *column(size_t j) { return V.column_pointer(keep_v ? j : j % 3); }
    void start()
    {
        View x(column(0), N);
        cusp::copy(cusp::random_array<T>(N), x);
        cusp::eigen::detail::normalize_on_device(x, c, ws.ws);
    }
    // w <- w - (*h) v (h == null: skipped); *out <- <w, u>
    void axpy_dot(const double *h, const T *v, T *w, const T *u, double *out)
    {
        cusp::detail::check(cusp::detail::by_type<T>(cmi_blas_axpy_dot_f64, cmi_blas_axpy_dot_f32)(N, h, v, w, u, out, ws.ws, nullptr));
    }
    // modified Gram-Schmidt of column iter + 1 against the `count` columns from `first`: count + 1 launches, <w, w> to c[2]
    void chain(size_t iter, size_t count, size_t first = 0)
    {
        T *w = column(iter + 1);
        double *g = c + 4;
        axpy_dot(nullptr, w, w, column(first), g);
        for (size_t i = 0; i + 1 < count; i++) axpy_dot(g + i, column(first + i), w, column(first + i + 1), g + i + 1);
        axpy_dot(g + count - 1, column(first + count - 1), w, w, c + 2);
    }
    double chain_and_read(size_t iter, size_t count, size_t first = 0)
    {
        chain(iter, count, first);
        double ww;
        cusp::detail::check(cmi_memcpy_d2h(&ww, c + 2, sizeof(double), nullptr));
        return ww;
    }
    const LinearOperator &A;
    size_t N;
    bool keep_v;
    cusp::array2d<T, cusp::device_memory, cusp::column_major> V;
    cusp::blas::detail::device_workspace &ws;
    double *c, *final_ww;
    double chain_ww;
    bool chain_done;
};

inline std::vector<double> ritz_values(const std::vector<double> &alphas, const std::vector<double> &betas, size_t n, cusp::array2d<double, cusp::host_memory, cusp::column_major> *S)
{
    std::vector<double> w(n);
    if (S) S->resize(n, n);
    if (!cusp::detail::tridiagonal_eigen(n, alphas.data(), betas.data(), w.data(), S ? S->values.data() : nullptr))
        throw cusp::runtime_exception("lanczos: the tridiagonal eigen-solver did not converge");
    return w;
}

// the loop of reference detail/lanczos.inl over an engine (plain_engine or fused_engine)
template <typename Engine, typename Array1d, typename Array2d, typename Options>
void run(Engine &engine, size_t N, Array1d &eigVals, Array2d &eigVecs, Options &options, size_t low, size_t high)
{
    typedef typename Engine::T T;
    const T eps = std::numeric_limits<T>::epsilon();
    const bool full = options.reorth == cusp::eigen::Full;
    size_t iter = 0, restarts = 0, min_iter = options.minIter, memory = options.minIter;
    size_t low_found = 0, high_found = 0, low_converged = 0, high_converged = 0;
    size_t reorth_steps = 0, reorth_vectors = 0;
    bool converged = false;
    std::vector<double> alphas(memory), betas(memory);
    T aa = 0, bb = 0, beta_sum = 0;
    engine.reserve(memory);
    while (true) {
        if (iter == memory) {
            if (options.verbose) std::cout << "At iteration #" << iter + 1 << ", memory expanded for storing Lanczos vectors" << std::endl;
            memory = static_cast<size_t>(memory * options.memoryExpansionFactor);
            if (memory <= iter) memory = iter + 1;
            alphas.resize(memory);
            betas.resize(memory);
            engine.reserve(memory);
        }
        const bool last = iter + 1 == options.maxIter;
        engine.step(iter, full && !last, aa, bb);
        alphas[iter] = aa;
        if (last) {
            betas[iter] = bb;
            iter++;
            break;
        }
        if ((full || iter + 1 < N) && iter + 1 >= min_iter && (iter + 1 - min_iter) % options.stride == 0 && low <= iter && high <= iter) {
            const std::vector<double> ritz0 = ritz_values(alphas, betas, iter, nullptr), ritz = ritz_values(alphas, betas, iter + 1, nullptr);
            size_t i = 0, left = low;
            T sum = 0, sum0 = 0, abs0 = 0;
            while (left && ritz[i] <= options.eigLowCut) {
                abs0 += static_cast<T>(std::abs(ritz0[i]));
                sum0 += static_cast<T>(ritz0[i]);
                sum += static_cast<T>(ritz[i]);
                left--;
                i++;
            }
            low_found = low - left;
            T low_error = std::abs((sum - sum0) / abs0);
            if (abs0 == T(0) && sum == T(0)) low_error = 0;
            if (options.verbose && low)
                std::cout << "At iteration #" << iter + 1 << " estimated eigen error (low end) is " << low_error << " (" << low_found << " eigenvalues)" << std::endl;
            i = iter;
            left = high;
            sum = sum0 = abs0 = 0;
            while (left && ritz[i] >= options.eigHighCut) {
                abs0 += static_cast<T>(std::abs(ritz0[i - 1]));
                sum0 += static_cast<T>(ritz0[i - 1]);
                sum += static_cast<T>(ritz[i]);
                left--;
                i--;
            }
            high_found = high - left;
            T high_error = std::abs((sum - sum0) / abs0);
            if (abs0 == T(0) && sum == T(0)) high_error = 0;
            if (options.verbose && high)
                std::cout << "At iteration #" << iter + 1 << " estimated eigen error (high end) is " << high_error << " (" << high_found << " eigenvalues)" << std::endl;
            if (low_error <= options.tol && high_error <= options.tol) {
                if (options.extraIter == 0) {
                    low_converged = low_found;
                    high_converged = high_found;
                }
                if (low_converged < low_found || high_converged < high_found) {
                    low_converged = low_found;
                    high_converged = high_found;
                    min_iter = std::min(iter + options.extraIter + 1, options.maxIter);
                    if (options.verbose) std::cout << "At iteration #" << iter + 1 << ", eigenvalues are deemed converged, running extra iterations." << std::endl;
                } else {
                    converged = true;
                    betas[iter] = bb;
                    iter++;
                    break;
                }
            }
        }
        betas[iter] = bb;
        beta_sum += bb;
        if (full) {
            bool doubled = false;
            bb = engine.reorthogonalise(iter, bb, options.doubleReorthGamma, doubled);
            reorth_steps += doubled ? 2 : 1;
            reorth_vectors += (doubled ? 2 : 1) * (iter + 1);
            if (doubled && options.verbose) std::cout << "At iteration #" << iter + 1 << ", reorthogonalization is doubled" << std::endl;
            betas[iter] = bb;
        }
        if (bb < beta_sum * eps || bb == T(0)) {
            if (options.verbose) std::cout << "bb deemed zero!" << std::endl;
            bb = engine.restart(iter, ++restarts);
            betas[iter] = 0.0;
            if (bb == T(0)) { // nothing is left outside the span of the vectors kept: T_iter+1 is complete, its values are eigenvalues of A
                iter++;
                break;
            }
        }
        engine.normalise(iter, bb);
        iter++;
    }

    const size_t m = iter;
    last_run() = run_info{m, converged, restarts};
    cusp::array2d<double, cusp::host_memory, cusp::column_major> S;
    const std::vector<double> ritz = ritz_values(alphas, betas, m, options.computeEigVecs ? &S : nullptr);
    if (!converged) {
        if (options.verbose && (full || options.maxIter < N) && options.minIter != options.maxIter)
            std::cout << "Maximum number of Lanczos iterations " << iter << " is met, but the desired eigenvalues may not be converged!" << std::endl;
        low_found = 0;
        while (low_found < low && low_found < m && ritz[low_found] <= options.eigLowCut) low_found++;
        high_found = 0;
        while (high_found < high && low_found + high_found < m && ritz[m - 1 - high_found] >= options.eigHighCut) high_found++;
    }
    const size_t found = low_found + high_found;
    std::vector<size_t> chosen; // the low end ascending, then the high end ascending
    for (size_t i = 0; i < low_found; i++) chosen.push_back(i);
    for (size_t i = 0; i < high_found; i++) chosen.push_back(m - high_found + i);
    cusp::array1d<typename Array1d::value_type, cusp::host_memory> values(found);
    for (size_t i = 0; i < found; i++) values[i] = static_cast<typename Array1d::value_type>(ritz[chosen[i]]);
    eigVals = values;
    double max_absolute = 0, max_relative = 0;
    if (found == 0) {
        eigVecs.resize(0, 0);
    } else if (options.computeEigVecs) {
        cusp::array2d<T, cusp::host_memory, cusp::column_major> selected(m, found);
        for (size_t col = 0; col < found; col++) {
            for (size_t row = 0; row < m; row++) selected(row, col) = static_cast<T>(S(row, chosen[col]));
            const double estimate = std::abs(betas[m - 1] * S(m - 1, chosen[col])); // the residual norm of a Ritz pair: |beta_m s_m|
            max_absolute = std::max(max_absolute, estimate);
            max_relative = std::max(max_relative, std::abs(estimate / ritz[chosen[col]]));
        }
        eigVecs.resize(N, found);
        engine.ritz_vectors(m, selected, eigVecs);
    }
    engine.finish();
    if (options.verbose) {
        std::cout << "\nMax absolute eigenvalue error   : " << max_absolute << "\nMax relative eigenvalue error   : " << max_relative << "\nEigenvalues :" << std::endl;
        for (size_t i = 0; i < found; i++) std::cout << std::setw(6) << i << std::setw(17) << std::scientific << std::setprecision(7) << ritz[chosen[i]] << std::endl;
        std::cout.unsetf(std::ios::floatfield);
        const double rate = iter > 1 ? 2.0 * (double(reorth_vectors) / double(iter) / double(iter - 1)) : 0.0;
        std::cout << "\nIteration Count                     : " << iter << "\nReorthogonalization Iteration Count : " << reorth_steps
                  << "\nReorthogonalization Vector Count    : " << reorth_vectors << " (" << 100.0 * rate << "%)\n" << std::endl;
    }
}

template <typename Array2d> struct is_column_major : std::is_same<typename Array2d::orientation, cusp::column_major> {};

} // namespace lanczos_detail
} // namespace detail

template <typename LinearOperator, typename Array1d, typename Array2d, typename LanczosOptions>
void lanczos(const LinearOperator &A, Array1d &eigVals, Array2d &eigVecs, LanczosOptions &options)
{
    namespace d = detail::lanczos_detail;
    typedef typename LinearOperator::value_type T;
    typedef typename LinearOperator::memory_space Space;
    if (A.num_rows != A.num_cols) throw cusp::invalid_input_exception("lanczos: matrix must be square");
    if constexpr (!d::is_column_major<Array2d>::value || !std::is_same<typename Array2d::memory_space, Space>::value ||
                  !std::is_same<typename Array2d::value_type, T>::value) {
        throw cusp::invalid_input_exception("lanczos: eigVecs must be a column_major array2d of A's value type in A's memory space");
    } else {
        const size_t N = A.num_cols;
        const size_t wanted = std::min(eigVals.size(), N);
        if (options.eigPart != SA && options.eigPart != LA && options.eigPart != BE) throw cusp::runtime_exception("Invalid spectrum part specified!");
        const size_t ends = options.eigPart == BE ? (wanted + 1) / 2 : wanted;
        if (options.minIter == 0) {
            options.minIter = options.defaultMinIterFactor * ends;
            if (options.maxIter) options.minIter = std::min(options.maxIter, options.minIter);
        }
        if (options.maxIter == 0) options.maxIter = 500 + options.defaultMaxIterFactor * ends;
        if (options.reorth) {
            options.minIter = std::min(options.minIter, N);
            options.maxIter = std::min(options.maxIter, N);
        }
        options.maxIter = std::max(options.maxIter, options.minIter);
        if (options.stride == 0) options.stride = 10;
        if (options.memoryExpansionFactor <= 1.0) options.memoryExpansionFactor = 1.2;
        if (options.tol < 0.0) options.tol = std::sqrt(std::numeric_limits<T>::epsilon());
        if (options.verbose) options.print();
        if (N == 0 || wanted == 0 || options.maxIter == 0) {
            eigVals.resize(0);
            eigVecs.resize(0, 0);
            d::last_run() = d::run_info{0, false, 0};
            return;
        }
        const size_t low = options.eigPart == SA ? wanted : (options.eigPart == BE ? wanted / 2 : 0), high = wanted - low;
        const bool keep_v = options.reorth == Full || options.computeEigVecs;
        if constexpr (detail::fused_on_device<LinearOperator>::value) {
            const char *e = std::getenv("CMI_LANCZOS_FUSED");
            if (!(e && e[0] == '0')) {
                d::fused_engine<LinearOperator> engine(A, keep_v, options.maxIter);
                d::run(engine, N, eigVals, eigVecs, options, low, high);
                return;
            }
        }
        d::plain_engine<LinearOperator> engine(A, keep_v); // (measurements on the device: the operation-by-operation path)
        d::run(engine, N, eigVals, eigVecs, options, low, high);
    }
}

template <typename LinearOperator, typename Array1d, typename Array2d> void lanczos(const LinearOperator &A, Array1d &eigVals, Array2d &eigVecs)
{
    cusp::eigen::lanczos_options<typename LinearOperator::value_type> options;
    options.computeEigVecs = eigVecs.num_cols > 0;
    cusp::eigen::lanczos(A, eigVals, eigVecs, options);
}

template <typename LinearOperator, typename Array1d> void lanczos(const LinearOperator &A, Array1d &eigVals)
{
    cusp::array2d<typename LinearOperator::value_type, typename LinearOperator::memory_space, cusp::column_major> eigVecs;
    cusp::eigen::lanczos(A, eigVals, eigVecs);
}

} // namespace eigen
} // namespace cusp

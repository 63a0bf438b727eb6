// krylov_m.hip -- the vector and coefficient steps of the multi-shift Krylov solvers cusp::krylov::cg_m and bicgstab_m, which solve
// (A + sigma_s I) x_s = b for num_shifts shifts with the multiplies of ONE system (B. Jegerlehner, "Krylov space solvers for shifted
// linear systems", hep-lat/9612014).
//
// Replaces (reference tree): cusp/krylov/detail/cg_m.inl and bicgstab_m.inl -- the functors KERNEL_ZB, KERNEL_A, KERNEL_XP, KERNEL_S,
// KERNEL_CHIRHO, KERNEL_XS, each run there as a thrust::for_each over num_shifts or over n x num_shifts elements (an integer division and
// a modulo per element, r read once per shift, the per-shift coefficients fetched per element).  Restated here, term for term and
// unfused (-ffp-contract=off), so a host loop over the same expressions gives the same bits.
//
// The shifted updates are the hot path: 4 num_shifts + 3 vector passes per CG-M iteration against ~1 for the multiply.  A lane owns one
// 16-byte piece of the position range, loads r (p0; r0, r1, w1) ONCE and walks the shifts kShiftUnroll at a time -- that many shifts'
// loads of x_s and p_s are in flight before the first store -- with the per-shift coefficients as wave-uniform reads.  Shift s lives at
// offset s * ld (64-bit: (num_shifts - 1) ld + n may pass 2^31); whether shift s can use 16-byte accesses is decided per shift, since an
// ld that is no multiple of the piece breaks the alignment from one shift to the next.
#include "blas1_shared.h" // + ld_piece / st_piece, any_overlap

namespace cmi {
namespace {

constexpr int kShiftUnroll = 4;    // shifts whose loads are in flight together: 8 x 16 bytes per lane
constexpr bool kShiftNtStores = true; // x_s and p_s (s_s) are not read again before the next iteration's multiply has streamed its matrix: nt, as CG's x
constexpr bool kShiftNtLoads = true;  // ... and each is read once per iteration

// ---- CG-M ------------------------------------------------------------------------------------------------------------------------------
// KERNEL_ZB (+ the clamp), KERNEL_A and the rotation of zeta for every shift; one workgroup, strided over the shifts, so that the store of
// the new (beta_0, alpha_0) into `state` comes behind every read of the old pair.
template <typename T>
__global__ void __launch_bounds__(kBlasBlock)
cg_m_coefficients_kernel(int64_t num_shifts, const double *__restrict__ rsq_old, const double *__restrict__ pAp, const double *__restrict__ rsq_new,
                         T *__restrict__ state, const T *__restrict__ sigma, T *__restrict__ zeta_m1, T *__restrict__ zeta_0, T *__restrict__ beta_s,
                         T *__restrict__ alpha_s)
{
    const T beta_m1 = state[0], alpha_old = state[1];
    const T beta_0 = -(T)(*rsq_old / *pAp);     // the -alpha of cmi_cg_update_*
    const T alpha_0 = (T)(*rsq_new / *rsq_old); // the beta of cmi_cg_direction_*
    for (int64_t s = threadIdx.x; s < num_shifts; s += kBlasBlock) {
        const T z0 = zeta_0[s], zm1 = zeta_m1[s], sg = sigma[s];
        T z1 = z0 * zm1 * beta_m1 / (beta_0 * alpha_old * (zm1 - z0) + beta_m1 * zm1 * (T(1) - beta_0 * sg));
        const T b0 = beta_0 * z1 / z0;
        if (fabs(z1) < T(1e-30)) z1 = T(1e-18);
        beta_s[s] = b0;
        alpha_s[s] = alpha_0 / beta_0 * z1 * b0 / z0;
        zeta_m1[s] = z0;
        zeta_0[s] = z1;
    }
    __syncthreads();
    if (threadIdx.x == 0) { state[0] = beta_0; state[1] = alpha_0; }
}

// U consecutive shifts of one piece: all 2 U loads are issued before the first store
template <typename T, int U>
__device__ __forceinline__ void xp_shifts(int64_t s, int64_t ld, int64_t e0, int cnt, bool full, const typename vec16<T>::type &rv, const T *__restrict__ beta_s,
                                          const T *__restrict__ alpha_s, const T *__restrict__ zeta_0, T *__restrict__ x, T *__restrict__ ps, bool x_wide, bool ps_wide)
{
    typedef typename vec16<T>::type V;
    constexpr int W = vec16<T>::n;
    V xv[U], pv[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int64_t base = (s + u) * ld;
        const bool w = full && base % W == 0;
        xv[u] = ld_piece(x + base + e0, cnt, w && x_wide, kShiftNtLoads);
        pv[u] = ld_piece(ps + base + e0, cnt, w && ps_wide, kShiftNtLoads);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int64_t base = (s + u) * ld;
        const bool w = full && base % W == 0;
        const T b = beta_s[s + u], a = alpha_s[s + u], z = zeta_0[s + u];
#pragma unroll
        for (int k = 0; k < W; k++) {
            xv[u][k] = xv[u][k] - b * pv[u][k];
            pv[u][k] = z * rv[k] + a * pv[u][k];
        }
        st_piece(x + base + e0, xv[u], cnt, w && x_wide, kShiftNtStores);
        st_piece(ps + base + e0, pv[u], cnt, w && ps_wide, kShiftNtStores);
    }
}

// p0 <- r + alpha_0 p0;  x_s <- x_s - beta_s p_s (the OLD p_s);  p_s <- zeta_s r + alpha_s p_s   (KERNEL_XP and the xpay in front of it)
template <typename T>
__global__ void __launch_bounds__(kBlasBlock)
cg_m_update_xp_kernel(int64_t n, int64_t num_shifts, int64_t ld, const T *__restrict__ state, const T *__restrict__ beta_s, const T *__restrict__ alpha_s,
                      const T *__restrict__ zeta_0, const T *__restrict__ r, T *__restrict__ p0 /* may be null */, T *__restrict__ x, T *__restrict__ ps,
                      int r_wide, int p0_wide, int x_wide, int ps_wide)
{
    typedef typename vec16<T>::type V;
    constexpr int W = vec16<T>::n;
    constexpr int U = kShiftUnroll;
    const int64_t npieces = (n + W - 1) / W;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const T alpha_0 = p0 ? state[1] : T(0);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npieces; i += stride) {
        const int64_t e0 = i * W;
        const int cnt = n - e0 < W ? (int)(n - e0) : W;
        const bool full = cnt == W;
        const V rv = ld_piece(r + e0, cnt, full && r_wide);
        if (p0) { // (uniform)
            V pv = ld_piece(p0 + e0, cnt, full && p0_wide);
#pragma unroll
            for (int k = 0; k < W; k++) pv[k] = rv[k] + alpha_0 * pv[k];
            st_piece(p0 + e0, pv, cnt, full && p0_wide, false); // gathered by the next multiply: plain
        }
        int64_t s = 0;
        for (; s + U <= num_shifts; s += U) xp_shifts<T, U>(s, ld, e0, cnt, full, rv, beta_s, alpha_s, zeta_0, x, ps, x_wide, ps_wide);
        for (; s < num_shifts; s++) xp_shifts<T, 1>(s, ld, e0, cnt, full, rv, beta_s, alpha_s, zeta_0, x, ps, x_wide, ps_wide);
    }
}

// ---- BiCGstab-M ------------------------------------------------------------------------------------------------------------------------
// KERNEL_S: s0 <- r1 + alpha_1 (s0 - chi_0 As)
template <typename T>
__global__ void __launch_bounds__(kBlasBlock)
bicgstab_m_s_kernel(int64_t n, T alpha_1, T chi_0, const T *__restrict__ r1, const T *__restrict__ As, T *__restrict__ s0, int wide)
{
    typedef typename vec16<T>::type V;
    constexpr int W = vec16<T>::n;
    const int64_t npieces = (n + W - 1) / W;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npieces; i += stride) {
        const int64_t e0 = i * W;
        const int cnt = n - e0 < W ? (int)(n - e0) : W;
        const bool w = cnt == W && wide;
        const V rv = ld_piece(r1 + e0, cnt, w), av = ld_piece(As + e0, cnt, w);
        V sv = ld_piece(s0 + e0, cnt, w);
#pragma unroll
        for (int k = 0; k < W; k++) sv[k] = rv[k] + alpha_1 * (sv[k] - chi_0 * av[k]);
        st_piece(s0 + e0, sv, cnt, w, false); // multiplied right away: plain
    }
}

// KERNEL_ZB (+ the clamp), KERNEL_CHIRHO and KERNEL_A for every shift; no rotation (KERNEL_XS needs both generations of zeta and rho)
template <typename T>
__global__ void __launch_bounds__(kBlasBlock)
bicgstab_m_coefficients_kernel(int64_t num_shifts, T beta_m1, T beta_0, T alpha_old, T alpha_new, T chi_0, const T *__restrict__ sigma,
                               const T *__restrict__ zeta_m1, const T *__restrict__ zeta_0, const T *__restrict__ rho_0, T *__restrict__ zeta_1,
                               T *__restrict__ beta_s, T *__restrict__ chi_s, T *__restrict__ rho_1, T *__restrict__ alpha_s)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < num_shifts; s += stride) {
        const T z0 = zeta_0[s], zm1 = zeta_m1[s], sg = sigma[s];
        T z1 = z0 * zm1 * beta_m1 / (beta_0 * alpha_old * (zm1 - z0) + beta_m1 * zm1 * (T(1) - beta_0 * sg));
        const T b0 = beta_0 * z1 / z0;
        if (fabs(z1) < T(1e-30)) z1 = T(1e-18);
        const T den = T(1) + chi_0 * sg;
        zeta_1[s] = z1;
        beta_s[s] = b0;
        chi_s[s] = chi_0 / den;
        rho_1[s] = rho_0[s] / den;
        alpha_s[s] = alpha_new / beta_0 * z1 * b0 / z0;
    }
}

// KERNEL_XS:  x_s <- x_s - beta_s s_s + chi_s rho0_s zeta1_s w1
//             s_s <- zeta1_s rho1_s r1 + alpha_s (s_s - chi_s rho0_s / beta_s (zeta1_s w1 - zeta0_s r0))       (the OLD s_s in both)
template <typename T> struct xs_coefficients { T b, c, rho0, z0, a, rho1, z1; };
template <typename T, typename V>
__device__ __forceinline__ void xs_piece(const xs_coefficients<T> &q, const V &r0v, const V &r1v, const V &w1v, V &xv, V &sv)
{
    constexpr int W = vec16<T>::n;
#pragma unroll
    for (int k = 0; k < W; k++) {
        const T s_0 = sv[k];
        xv[k] = xv[k] - q.b * s_0 + q.c * q.rho0 * q.z1 * w1v[k];
        sv[k] = q.z1 * q.rho1 * r1v[k] + q.a * (s_0 - q.c * q.rho0 / q.b * (q.z1 * w1v[k] - q.z0 * r0v[k]));
    }
}
template <typename T> struct xs_arrays { const T *beta_s, *chi_s, *rho_0, *zeta_0, *alpha_s, *rho_1, *zeta_1; };
template <typename T, int U>
__device__ __forceinline__ void xs_shifts(int64_t s, int64_t ld, int64_t e0, int cnt, bool full, const xs_arrays<T> &c, const typename vec16<T>::type &r0v,
                                          const typename vec16<T>::type &r1v, const typename vec16<T>::type &w1v, T *__restrict__ x, T *__restrict__ ss, bool x_wide,
                                          bool ss_wide)
{
    typedef typename vec16<T>::type V;
    constexpr int W = vec16<T>::n;
    V xv[U], sv[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int64_t base = (s + u) * ld;
        const bool w = full && base % W == 0;
        xv[u] = ld_piece(x + base + e0, cnt, w && x_wide, kShiftNtLoads);
        sv[u] = ld_piece(ss + base + e0, cnt, w && ss_wide, kShiftNtLoads);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int64_t base = (s + u) * ld, k = s + u;
        const bool w = full && base % W == 0;
        const xs_coefficients<T> q = {c.beta_s[k], c.chi_s[k], c.rho_0[k], c.zeta_0[k], c.alpha_s[k], c.rho_1[k], c.zeta_1[k]};
        xs_piece<T>(q, r0v, r1v, w1v, xv[u], sv[u]);
        st_piece(x + base + e0, xv[u], cnt, w && x_wide, kShiftNtStores);
        st_piece(ss + base + e0, sv[u], cnt, w && ss_wide, kShiftNtStores);
    }
}
template <typename T>
__global__ void __launch_bounds__(kBlasBlock)
bicgstab_m_update_xs_kernel(int64_t n, int64_t num_shifts, int64_t ld, const T *__restrict__ beta_s, const T *__restrict__ chi_s, const T *__restrict__ rho_0,
                            const T *__restrict__ zeta_0, const T *__restrict__ alpha_s, const T *__restrict__ rho_1, const T *__restrict__ zeta_1,
                            const T *__restrict__ r0, const T *__restrict__ r1, const T *__restrict__ w1, T *__restrict__ x, T *__restrict__ ss,
                            int r_wide, int x_wide, int ss_wide)
{
    typedef typename vec16<T>::type V;
    constexpr int W = vec16<T>::n;
    constexpr int U = kShiftUnroll;
    const xs_arrays<T> c = {beta_s, chi_s, rho_0, zeta_0, alpha_s, rho_1, zeta_1};
    const int64_t npieces = (n + W - 1) / W;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npieces; i += stride) {
        const int64_t e0 = i * W;
        const int cnt = n - e0 < W ? (int)(n - e0) : W;
        const bool full = cnt == W;
        const V r0v = ld_piece(r0 + e0, cnt, full && r_wide), r1v = ld_piece(r1 + e0, cnt, full && r_wide), w1v = ld_piece(w1 + e0, cnt, full && r_wide);
        int64_t s = 0;
        for (; s + U <= num_shifts; s += U) xs_shifts<T, U>(s, ld, e0, cnt, full, c, r0v, r1v, w1v, x, ss, x_wide, ss_wide);
        for (; s < num_shifts; s++) xs_shifts<T, 1>(s, ld, e0, cnt, full, c, r0v, r1v, w1v, x, ss, x_wide, ss_wide);
    }
}

// the rotation behind KERNEL_XS, a launch of its own (inside the update kernel it would race with the workgroups still reading zeta_0 / rho_0)
template <typename T>
__global__ void __launch_bounds__(kBlasBlock)
bicgstab_m_rotate_kernel(int64_t num_shifts, T *__restrict__ zeta_m1, T *__restrict__ zeta_0, const T *__restrict__ zeta_1, T *__restrict__ rho_0,
                         const T *__restrict__ rho_1)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < num_shifts; s += stride) {
        zeta_m1[s] = zeta_0[s];
        zeta_0[s] = zeta_1[s];
        rho_0[s] = rho_1[s];
    }
}

// ---- refusals, all made before any device call -------------------------------------------------------------------------------------------
template <typename T> size_t shifted_bytes(int64_t n, int64_t num_shifts, int64_t ld)
{
    return num_shifts > 0 && n > 0 ? ((size_t)(num_shifts - 1) * (size_t)ld + (size_t)n) * sizeof(T) : 0;
}
int small_grid(int64_t num_shifts) { const int64_t b = ceil_div(num_shifts, (int64_t)kBlasBlock); return b < 1 ? 1 : b > 1024 ? 1024 : (int)b; }

template <typename T>
int cg_m_coefficients_impl(int64_t num_shifts, const double *rsq_old, const double *pAp, const double *rsq_new, T *state, const T *sigma, T *zeta_m1,
                           T *zeta_0, T *beta_s, T *alpha_s, void *stream)
{
    if (num_shifts < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_cg_m_coefficients: negative num_shifts");
    if (!rsq_old || !pAp || !rsq_new || !state) return fail(CMI_ERROR_INVALID_VALUE, "cmi_cg_m_coefficients: null scalar or state");
    if (num_shifts > 0 && (!sigma || !zeta_m1 || !zeta_0 || !beta_s || !alpha_s)) return fail(CMI_ERROR_INVALID_VALUE, "cmi_cg_m_coefficients: null array");
    const size_t b = (size_t)num_shifts * sizeof(T);
    if (any_overlap({{state, 2 * sizeof(T)}, {zeta_m1, b}, {zeta_0, b}, {beta_s, b}, {alpha_s, b}},
                    {{rsq_old, sizeof(double)}, {pAp, sizeof(double)}, {rsq_new, sizeof(double)}, {sigma, b}}))
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_cg_m_coefficients: an output overlaps another array");
    hipLaunchKernelGGL((cg_m_coefficients_kernel<T>), dim3(1), dim3(kBlasBlock), 0, as_stream(stream), num_shifts, rsq_old, pAp, rsq_new, state, sigma, zeta_m1,
                       zeta_0, beta_s, alpha_s);
    CMI_LAUNCH_CHECK("cg_m_coefficients");
    return CMI_SUCCESS;
}

template <typename T>
int cg_m_update_xp_impl(int64_t n, int64_t num_shifts, int64_t ld, const T *state, const T *beta_s, const T *alpha_s, const T *zeta_0, const T *r, T *p0, T *x,
                        T *ps, void *stream)
{
    if (n < 0 || num_shifts < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_cg_m_update_xp: negative n or num_shifts");
    if (n == 0) return CMI_SUCCESS;
    if (num_shifts > 0 && (!beta_s || !alpha_s || !zeta_0 || !r || !x || !ps)) return fail(CMI_ERROR_INVALID_VALUE, "cmi_cg_m_update_xp: null array");
    if (p0 && (!state || !r)) return fail(CMI_ERROR_INVALID_VALUE, "cmi_cg_m_update_xp: p0 without state or r");
    if (num_shifts > 0 && ld < n) return fail(CMI_ERROR_INVALID_VALUE, "cmi_cg_m_update_xp: ld < n");
    if (num_shifts == 0 && !p0) return CMI_SUCCESS;
    const size_t vb = (size_t)n * sizeof(T), sb = (size_t)num_shifts * sizeof(T), xb = shifted_bytes<T>(n, num_shifts, ld);
    if (any_overlap({{p0, vb}, {x, xb}, {ps, xb}}, {{state, 2 * sizeof(T)}, {beta_s, sb}, {alpha_s, sb}, {zeta_0, sb}, {r, vb}}))
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_cg_m_update_xp: an output overlaps another array");
    hipLaunchKernelGGL((cg_m_update_xp_kernel<T>), dim3(fused_grid(n, vec16<T>::n)), dim3(kBlasBlock), 0, as_stream(stream), n, num_shifts, ld, state, beta_s,
                       alpha_s, zeta_0, r, p0, x, ps, (int)aligned16(r), (int)aligned16(p0), (int)aligned16(x), (int)aligned16(ps));
    CMI_LAUNCH_CHECK("cg_m_update_xp");
    return CMI_SUCCESS;
}

template <typename T> int bicgstab_m_s_impl(int64_t n, T alpha_1, T chi_0, const T *r1, const T *As, T *s0, void *stream)
{
    if (n < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_bicgstab_m_s: negative n");
    if (n == 0) return CMI_SUCCESS;
    if (!r1 || !As || !s0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_bicgstab_m_s: null array");
    const size_t vb = (size_t)n * sizeof(T);
    if (any_overlap({{s0, vb}}, {{r1, vb}, {As, vb}})) return fail(CMI_ERROR_INVALID_VALUE, "cmi_bicgstab_m_s: s_0 overlaps an input");
    hipLaunchKernelGGL((bicgstab_m_s_kernel<T>), dim3(stream_grid(n, vec16<T>::n)), dim3(kBlasBlock), 0, as_stream(stream), n, alpha_1, chi_0, r1, As, s0,
                       (int)aligned16(r1, As, s0));
    CMI_LAUNCH_CHECK("bicgstab_m_s");
    return CMI_SUCCESS;
}

template <typename T>
int bicgstab_m_coefficients_impl(int64_t num_shifts, T beta_m1, T beta_0, T alpha_old, T alpha_new, T chi_0, const T *sigma, const T *zeta_m1, const T *zeta_0,
                                 const T *rho_0, T *zeta_1, T *beta_s, T *chi_s, T *rho_1, T *alpha_s, void *stream)
{
    if (num_shifts < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_bicgstab_m_coefficients: negative num_shifts");
    if (num_shifts == 0) return CMI_SUCCESS;
    if (!sigma || !zeta_m1 || !zeta_0 || !rho_0 || !zeta_1 || !beta_s || !chi_s || !rho_1 || !alpha_s)
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_bicgstab_m_coefficients: null array");
    const size_t b = (size_t)num_shifts * sizeof(T);
    if (any_overlap({{zeta_1, b}, {beta_s, b}, {chi_s, b}, {rho_1, b}, {alpha_s, b}}, {{sigma, b}, {zeta_m1, b}, {zeta_0, b}, {rho_0, b}}))
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_bicgstab_m_coefficients: an output overlaps another array");
    hipLaunchKernelGGL((bicgstab_m_coefficients_kernel<T>), dim3(small_grid(num_shifts)), dim3(kBlasBlock), 0, as_stream(stream), num_shifts, beta_m1, beta_0,
                       alpha_old, alpha_new, chi_0, sigma, zeta_m1, zeta_0, rho_0, zeta_1, beta_s, chi_s, rho_1, alpha_s);
    CMI_LAUNCH_CHECK("bicgstab_m_coefficients");
    return CMI_SUCCESS;
}

template <typename T>
int bicgstab_m_update_xs_impl(int64_t n, int64_t num_shifts, int64_t ld, const T *beta_s, const T *chi_s, T *rho_0, T *zeta_m1, T *zeta_0, const T *alpha_s,
                              const T *rho_1, const T *zeta_1, const T *r0, const T *r1, const T *w1, T *x, T *ss, void *stream)
{
    if (n < 0 || num_shifts < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_bicgstab_m_update_xs: negative n or num_shifts");
    if (n == 0 || num_shifts == 0) return CMI_SUCCESS;
    if (!beta_s || !chi_s || !rho_0 || !zeta_m1 || !zeta_0 || !alpha_s || !rho_1 || !zeta_1 || !r0 || !r1 || !w1 || !x || !ss)
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_bicgstab_m_update_xs: null array");
    if (ld < n) return fail(CMI_ERROR_INVALID_VALUE, "cmi_bicgstab_m_update_xs: ld < n");
    const size_t vb = (size_t)n * sizeof(T), sb = (size_t)num_shifts * sizeof(T), xb = shifted_bytes<T>(n, num_shifts, ld);
    if (any_overlap({{x, xb}, {ss, xb}, {zeta_m1, sb}, {zeta_0, sb}, {rho_0, sb}},
                    {{beta_s, sb}, {chi_s, sb}, {alpha_s, sb}, {rho_1, sb}, {zeta_1, sb}, {r0, vb}, {r1, vb}, {w1, vb}}))
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_bicgstab_m_update_xs: an output overlaps another array");
    hipLaunchKernelGGL((bicgstab_m_update_xs_kernel<T>), dim3(fused_grid(n, vec16<T>::n)), dim3(kBlasBlock), 0, as_stream(stream), n, num_shifts, ld, beta_s,
                       chi_s, (const T *)rho_0, (const T *)zeta_0, alpha_s, rho_1, zeta_1, r0, r1, w1, x, ss, (int)aligned16(r0, r1, w1), (int)aligned16(x),
                       (int)aligned16(ss));
    hipLaunchKernelGGL((bicgstab_m_rotate_kernel<T>), dim3(small_grid(num_shifts)), dim3(kBlasBlock), 0, as_stream(stream), num_shifts, zeta_m1, zeta_0, zeta_1, rho_0,
                       rho_1);
    CMI_LAUNCH_CHECK("bicgstab_m_update_xs");
    return CMI_SUCCESS;
}

} // namespace
} // namespace cmi

using namespace cmi;

CMI_API int cmi_cg_m_coefficients_f64(int64_t num_shifts, const double *rsq_old_dev, const double *pAp_dev, const double *rsq_new_dev, double *state,
                                      const double *sigma, double *zeta_m1, double *zeta_0, double *beta_s, double *alpha_s, void *stream)
{ return cg_m_coefficients_impl<double>(num_shifts, rsq_old_dev, pAp_dev, rsq_new_dev, state, sigma, zeta_m1, zeta_0, beta_s, alpha_s, stream); }
CMI_API int cmi_cg_m_coefficients_f32(int64_t num_shifts, const double *rsq_old_dev, const double *pAp_dev, const double *rsq_new_dev, float *state,
                                      const float *sigma, float *zeta_m1, float *zeta_0, float *beta_s, float *alpha_s, void *stream)
{ return cg_m_coefficients_impl<float>(num_shifts, rsq_old_dev, pAp_dev, rsq_new_dev, state, sigma, zeta_m1, zeta_0, beta_s, alpha_s, stream); }
CMI_API int cmi_cg_m_update_xp_f64(int64_t n, int64_t num_shifts, int64_t ld, const double *state, const double *beta_s, const double *alpha_s, const double *zeta_0,
                                   const double *r, double *p0, double *x, double *p_s, void *stream)
{ return cg_m_update_xp_impl<double>(n, num_shifts, ld, state, beta_s, alpha_s, zeta_0, r, p0, x, p_s, stream); }
CMI_API int cmi_cg_m_update_xp_f32(int64_t n, int64_t num_shifts, int64_t ld, const float *state, const float *beta_s, const float *alpha_s, const float *zeta_0,
                                   const float *r, float *p0, float *x, float *p_s, void *stream)
{ return cg_m_update_xp_impl<float>(n, num_shifts, ld, state, beta_s, alpha_s, zeta_0, r, p0, x, p_s, stream); }
CMI_API int cmi_bicgstab_m_s_f64(int64_t n, double alpha_1, double chi_0, const double *r_1, const double *As, double *s_0, void *stream)
{ return bicgstab_m_s_impl<double>(n, alpha_1, chi_0, r_1, As, s_0, stream); }
CMI_API int cmi_bicgstab_m_s_f32(int64_t n, float alpha_1, float chi_0, const float *r_1, const float *As, float *s_0, void *stream)
{ return bicgstab_m_s_impl<float>(n, alpha_1, chi_0, r_1, As, s_0, stream); }
CMI_API int cmi_bicgstab_m_coefficients_f64(int64_t num_shifts, double beta_m1, double beta_0, double alpha_old, double alpha_new, double chi_0, const double *sigma,
                                            const double *zeta_m1, const double *zeta_0, const double *rho_0, double *zeta_1, double *beta_s, double *chi_s,
                                            double *rho_1, double *alpha_s, void *stream)
{ return bicgstab_m_coefficients_impl<double>(num_shifts, beta_m1, beta_0, alpha_old, alpha_new, chi_0, sigma, zeta_m1, zeta_0, rho_0, zeta_1, beta_s, chi_s, rho_1, alpha_s, stream); }
CMI_API int cmi_bicgstab_m_coefficients_f32(int64_t num_shifts, float beta_m1, float beta_0, float alpha_old, float alpha_new, float chi_0, const float *sigma,
                                            const float *zeta_m1, const float *zeta_0, const float *rho_0, float *zeta_1, float *beta_s, float *chi_s, float *rho_1,
                                            float *alpha_s, void *stream)
{ return bicgstab_m_coefficients_impl<float>(num_shifts, beta_m1, beta_0, alpha_old, alpha_new, chi_0, sigma, zeta_m1, zeta_0, rho_0, zeta_1, beta_s, chi_s, rho_1, alpha_s, stream); }
CMI_API int cmi_bicgstab_m_update_xs_f64(int64_t n, int64_t num_shifts, int64_t ld, const double *beta_s, const double *chi_s, double *rho_0, double *zeta_m1,
                                         double *zeta_0, const double *alpha_s, const double *rho_1, const double *zeta_1, const double *r_0, const double *r_1,
                                         const double *w_1, double *x, double *s_s, void *stream)
{ return bicgstab_m_update_xs_impl<double>(n, num_shifts, ld, beta_s, chi_s, rho_0, zeta_m1, zeta_0, alpha_s, rho_1, zeta_1, r_0, r_1, w_1, x, s_s, stream); }
CMI_API int cmi_bicgstab_m_update_xs_f32(int64_t n, int64_t num_shifts, int64_t ld, const float *beta_s, const float *chi_s, float *rho_0, float *zeta_m1, float *zeta_0,
                                         const float *alpha_s, const float *rho_1, const float *zeta_1, const float *r_0, const float *r_1, const float *w_1, float *x,
                                         float *s_s, void *stream)
{ return bicgstab_m_update_xs_impl<float>(n, num_shifts, ld, beta_s, chi_s, rho_0, zeta_m1, zeta_0, alpha_s, rho_1, zeta_1, r_0, r_1, w_1, x, s_s, stream); }

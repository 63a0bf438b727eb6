// lobpcg.hip -- the vector tail of cusp::eigen::lobpcg for one eigenpair (A. Knyazev, "Toward the optimal preconditioned eigensolver: locally
// optimal block preconditioned conjugate gradient method", SIAM J. Sci. Comput. 23 (2001)).
//
// Replaces (reference tree): cusp/eigen/detail/lobpcg.inl:67-180 -- per iteration, with identity M and after the first one, axpby, 3 nrm2,
// 3 scal, a copy, 8 dot and 4 axpby: 33 vector reads, 9 writes and 12 host reads around ONE multiply.  Here the same expressions, term for
// term and unfused (-ffp-contract=off), in three kernels:
//   residual  r <- T(-lambda) x + ax;  <r, r>                                                      (before the first iteration)
//   gram      p, ap <- s p, s ap with s = T(1) / T(sqrt(<p, p>));  the eight sums of the Gram pair from the SCALED values: 5 reads, 2 writes
//   update    p, ap <- c_R (w, aw) + c_P (p, ap);  x, ax <- c_X (x, ax) + (p, ap);  r <- T(-lambda) x + ax;  <r, r>, <p, p>: 6 reads, 5 writes
// A lane owns one 16-byte piece of the position range (vec16, ld_piece / st_piece of blas1_shared.h): 16-byte accesses when every operand
// is 16-byte aligned, element accesses otherwise.  Reductions: products and sums in double, one partial per workgroup and sum (a fixed DPP
// tree per wave, the waves in order), list j at workspace[j * kListCap ...); one workgroup per sum folds its list in a fixed order -- no
// atomics, the same bits on every run.  The grid is multi_sum_grid(n, W, kLists): one-shot up to kListCap workgroups, grid-strided past it.
#include "blas1_shared.h"

namespace cmi {
namespace {

constexpr int kLists = 8;                          // the Gram pair's eight sums; the other two kernels keep the same grid rule
constexpr int kListCap = multi_sum_cap(kLists);    // 16384 partials per list: all eight fit the first fold area of the workspace
constexpr int kWaves = kBlasBlock / kWave;
static_assert(kLists * kListCap <= kPartialCapacity, "the partial lists must fit one fold area");

// NS sums of one workgroup: lanes by the DPP tree, waves in order; thread j stores sum j as partial j of this workgroup
template <int NS> __device__ __forceinline__ void store_block_sums(const double (&acc)[NS], double (*slots)[kWaves], double *__restrict__ partial)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int j = 0; j < NS; j++) {
        const double v = wave_sum_to_last(acc[j]);
        if (lane == kWave - 1) slots[j][wave] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < NS) {
        double s = 0.0;
        for (int w = 0; w < kWaves; w++) s += slots[threadIdx.x][w];
        partial[(size_t)threadIdx.x * kListCap + blockIdx.x] = s;
    }
}

// workgroup b folds list first_list + b: lane t adds partials t, t + 256, ... in that order, then the block tree; npartial == 0 stores 0
__global__ void __launch_bounds__(kBlasBlock)
lobpcg_fold_kernel(int npartial, const double *__restrict__ partial, int first_list, double *__restrict__ out, double *__restrict__ mirror)
{
    __shared__ double slots[1][kWaves];
    const int list = first_list + blockIdx.x;
    const double *mine = partial + (size_t)list * kListCap;
    double acc = 0.0;
    for (int i = threadIdx.x; i < npartial; i += kBlasBlock) acc += mine[i];
    const double v = wave_sum_to_last(acc);
    if ((threadIdx.x & (kWave - 1)) == kWave - 1) slots[0][threadIdx.x / kWave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < kWaves; w++) s += slots[0][w];
        out[list] = s;
        if (mirror && list == 0) *mirror = s;
    }
}

// r <- T(-lambda) x + ax;  partials of <r, r>
template <typename T>
__global__ void __launch_bounds__(kBlasBlock)
lobpcg_residual_kernel(int64_t n, const double *__restrict__ lambda, const T *__restrict__ x, const T *__restrict__ ax, T *__restrict__ r,
                       double *__restrict__ partial, int wide)
{
    typedef typename vec16<T>::type V;
    constexpr int W = vec16<T>::n;
    __shared__ double slots[1][kWaves];
    const T neg = -(T)(*lambda);
    const int64_t npieces = (n + W - 1) / W;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    double acc[1] = {0.0};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npieces; i += stride) {
        const int64_t e0 = i * W;
        const int cnt = n - e0 < W ? (int)(n - e0) : W;
        const bool w16 = cnt == W && wide;
        const V xv = ld_piece(x + e0, cnt, w16), av = ld_piece(ax + e0, cnt, w16);
        V rv;
#pragma unroll
        for (int k = 0; k < W; k++) {
            rv[k] = neg * xv[k] + av[k];
            if (k < cnt) acc[0] += (double)rv[k] * (double)rv[k];
        }
        st_piece(r + e0, rv, cnt, w16, false);
    }
    store_block_sums<1>(acc, slots, partial);
}

// HasP: p, ap <- s p, s ap, then the eight sums; else the first three (x, w, aw only)
template <typename T, bool HasP>
__global__ void __launch_bounds__(kBlasBlock)
lobpcg_gram_kernel(int64_t n, const double *__restrict__ pp, const T *__restrict__ x, const T *__restrict__ w, const T *__restrict__ aw, T *__restrict__ p,
                   T *__restrict__ ap, double *__restrict__ partial, int wide)
{
    typedef typename vec16<T>::type V;
    constexpr int W = vec16<T>::n;
    constexpr int NS = HasP ? 8 : 3;
    __shared__ double slots[NS][kWaves];
    T s = T(0);
    if constexpr (HasP) s = T(1) / (T)sqrt(*pp); // the root in double, rounded to T once; the reciprocal formed once in T
    const int64_t npieces = (n + W - 1) / W;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    double acc[NS] = {};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npieces; i += stride) {
        const int64_t e0 = i * W;
        const int cnt = n - e0 < W ? (int)(n - e0) : W;
        const bool w16 = cnt == W && wide;
        const V xv = ld_piece(x + e0, cnt, w16), wv = ld_piece(w + e0, cnt, w16), awv = ld_piece(aw + e0, cnt, w16);
        V pv = {}, apv = {};
        if constexpr (HasP) {
            pv = ld_piece(p + e0, cnt, w16);
            apv = ld_piece(ap + e0, cnt, w16);
#pragma unroll
            for (int k = 0; k < W; k++) { pv[k] = s * pv[k]; apv[k] = s * apv[k]; }
            st_piece(p + e0, pv, cnt, w16, false);  // read again by the update kernel right behind the host's 3 x 3 problem: plain
            st_piece(ap + e0, apv, cnt, w16, false);
        }
#pragma unroll
        for (int k = 0; k < W; k++) {
            if (k < cnt) {
                const double xd = xv[k], wd = wv[k], awd = awv[k];
                acc[0] += xd * awd;
                acc[1] += wd * awd;
                acc[2] += xd * wd;
                if constexpr (HasP) {
                    const double pd = pv[k], apd = apv[k];
                    acc[3] += xd * apd;
                    acc[4] += wd * apd;
                    acc[5] += pd * apd;
                    acc[6] += xd * pd;
                    acc[7] += wd * pd;
                }
            }
        }
    }
    store_block_sums<NS>(acc, slots, partial);
}

// the Ritz update; list 0: <r, r> (r != null), list 1: <p, p> of the new p
template <typename T>
__global__ void __launch_bounds__(kBlasBlock)
lobpcg_update_kernel(int64_t n, T cx, T cr, T cp, int first, T neg_lambda, const T *__restrict__ w, const T *__restrict__ aw, T *__restrict__ p, T *__restrict__ ap,
                     T *__restrict__ x, T *__restrict__ ax, T *__restrict__ r /* may be null */, double *__restrict__ partial, int wide)
{
    typedef typename vec16<T>::type V;
    constexpr int W = vec16<T>::n;
    __shared__ double slots[2][kWaves];
    const int64_t npieces = (n + W - 1) / W;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    double acc[2] = {0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npieces; i += stride) {
        const int64_t e0 = i * W;
        const int cnt = n - e0 < W ? (int)(n - e0) : W;
        const bool w16 = cnt == W && wide;
        const V wv = ld_piece(w + e0, cnt, w16), awv = ld_piece(aw + e0, cnt, w16);
        V pv = ld_piece(p + e0, cnt, w16), apv = ld_piece(ap + e0, cnt, w16), xv = ld_piece(x + e0, cnt, w16), axv = ld_piece(ax + e0, cnt, w16);
        V rv = {};
#pragma unroll
        for (int k = 0; k < W; k++) {
            if (first) { // (uniform) the reference's axpy into the zero-initialised p
                pv[k] = cr * wv[k] + pv[k];
                apv[k] = cr * awv[k] + apv[k];
            } else {
                pv[k] = cr * wv[k] + cp * pv[k];
                apv[k] = cr * awv[k] + cp * apv[k];
            }
            xv[k] = cx * xv[k] + T(1) * pv[k];
            axv[k] = cx * axv[k] + T(1) * apv[k];
            if (k < cnt) acc[1] += (double)pv[k] * (double)pv[k];
            if (r) { // (uniform)
                rv[k] = neg_lambda * xv[k] + axv[k];
                if (k < cnt) acc[0] += (double)rv[k] * (double)rv[k];
            }
        }
        st_piece(p + e0, pv, cnt, w16, false);
        st_piece(ap + e0, apv, cnt, w16, false);
        st_piece(x + e0, xv, cnt, w16, false);
        st_piece(ax + e0, axv, cnt, w16, false);
        if (r) st_piece(r + e0, rv, cnt, w16, false);
    }
    store_block_sums<2>(acc, slots, partial);
}

template <typename T>
int residual_impl(int64_t n, const double *lambda_dev, const T *x, const T *ax, T *r, double *rr_dev, double *rr_host_mirror, void *workspace, void *stream)
{
    if (n < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_lobpcg_residual: negative n");
    if (!lambda_dev || !rr_dev || !workspace) return fail(CMI_ERROR_INVALID_VALUE, "cmi_lobpcg_residual: null scalar or workspace");
    if (n > 0 && (!x || !ax || !r)) return fail(CMI_ERROR_INVALID_VALUE, "cmi_lobpcg_residual: null array");
    const size_t vb = (size_t)n * sizeof(T);
    if (any_overlap({{r, vb}, {rr_dev, sizeof(double)}}, {{lambda_dev, sizeof(double)}, {x, vb}, {ax, vb}}))
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_lobpcg_residual: an output overlaps another array");
    const int grid = n > 0 ? multi_sum_grid(n, vec16<T>::n, kLists) : 0;
    double *part = (double *)workspace;
    if (n > 0)
        hipLaunchKernelGGL((lobpcg_residual_kernel<T>), dim3(grid), dim3(kBlasBlock), 0, as_stream(stream), n, lambda_dev, x, ax, r, part, (int)aligned16(x, ax, r));
    hipLaunchKernelGGL(lobpcg_fold_kernel, dim3(1), dim3(kBlasBlock), 0, as_stream(stream), grid, (const double *)part, 0, rr_dev, rr_host_mirror);
    CMI_LAUNCH_CHECK("lobpcg_residual");
    return CMI_SUCCESS;
}

template <typename T>
int gram_impl(int64_t n, const double *pp_dev, const T *x, const T *w, const T *aw, T *p, T *ap, double *gram_dev, void *workspace, void *stream)
{
    if (n < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_lobpcg_gram: negative n");
    if (!gram_dev || !workspace) return fail(CMI_ERROR_INVALID_VALUE, "cmi_lobpcg_gram: null result or workspace");
    if ((p == nullptr) != (ap == nullptr)) return fail(CMI_ERROR_INVALID_VALUE, "cmi_lobpcg_gram: null array (p and ap go together)");
    if (p && !pp_dev) return fail(CMI_ERROR_INVALID_VALUE, "cmi_lobpcg_gram: null scalar (p needs pp_dev)");
    if (n > 0 && (!x || !w || !aw)) return fail(CMI_ERROR_INVALID_VALUE, "cmi_lobpcg_gram: null array");
    const size_t vb = (size_t)n * sizeof(T);
    const int sums = p ? 8 : 3;
    if (any_overlap({{p, vb}, {ap, vb}, {gram_dev, sums * sizeof(double)}}, {{pp_dev, sizeof(double)}, {x, vb}, {w, vb}, {aw, vb}}))
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_lobpcg_gram: an output overlaps another array");
    const int grid = n > 0 ? multi_sum_grid(n, vec16<T>::n, kLists) : 0;
    double *part = (double *)workspace;
    if (n > 0) {
        if (p) hipLaunchKernelGGL((lobpcg_gram_kernel<T, true>), dim3(grid), dim3(kBlasBlock), 0, as_stream(stream), n, pp_dev, x, w, aw, p, ap, part,
                                  (int)aligned16(x, w, aw, p, ap));
        else hipLaunchKernelGGL((lobpcg_gram_kernel<T, false>), dim3(grid), dim3(kBlasBlock), 0, as_stream(stream), n, pp_dev, x, w, aw, p, ap, part,
                                (int)aligned16(x, w, aw));
    }
    hipLaunchKernelGGL(lobpcg_fold_kernel, dim3(sums), dim3(kBlasBlock), 0, as_stream(stream), grid, (const double *)part, 0, gram_dev, (double *)nullptr);
    CMI_LAUNCH_CHECK("lobpcg_gram");
    return CMI_SUCCESS;
}

template <typename T>
int update_impl(int64_t n, T cx, T cr, T cp, int first, T lambda_new, const T *w, const T *aw, T *p, T *ap, T *x, T *ax, T *r, double *scalars_dev,
                double *rr_host_mirror, void *workspace, void *stream)
{
    if (n < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_lobpcg_update: negative n");
    if (!scalars_dev || !workspace) return fail(CMI_ERROR_INVALID_VALUE, "cmi_lobpcg_update: null scalars or workspace");
    if (n > 0 && (!w || !aw || !p || !ap || !x || !ax)) return fail(CMI_ERROR_INVALID_VALUE, "cmi_lobpcg_update: null array");
    const size_t vb = (size_t)n * sizeof(T);
    if (any_overlap({{p, vb}, {ap, vb}, {x, vb}, {ax, vb}, {r, vb}, {scalars_dev, 2 * sizeof(double)}}, {{w, vb}, {aw, vb}}))
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_lobpcg_update: an output overlaps another array");
    const int grid = n > 0 ? multi_sum_grid(n, vec16<T>::n, kLists) : 0;
    double *part = (double *)workspace;
    if (n > 0)
        hipLaunchKernelGGL((lobpcg_update_kernel<T>), dim3(grid), dim3(kBlasBlock), 0, as_stream(stream), n, cx, cr, cp, first, -lambda_new, w, aw, p, ap, x, ax, r,
                           part, (int)(aligned16(w, aw, p, ap, x, ax) && aligned16(r)));
    // r == NULL: only <p, p> (list 1) is folded, scalars_dev[0] and the mirror stay as they are
    hipLaunchKernelGGL(lobpcg_fold_kernel, dim3(r ? 2 : 1), dim3(kBlasBlock), 0, as_stream(stream), grid, (const double *)part, r ? 0 : 1, scalars_dev,
                       r ? rr_host_mirror : (double *)nullptr);
    CMI_LAUNCH_CHECK("lobpcg_update");
    return CMI_SUCCESS;
}

} // namespace
} // namespace cmi

using namespace cmi;

CMI_API int cmi_lobpcg_residual_f64(int64_t n, const double *lambda_dev, const double *x, const double *ax, double *r, double *rr_dev, double *rr_host_mirror,
                                    void *workspace, void *stream)
{ return residual_impl<double>(n, lambda_dev, x, ax, r, rr_dev, rr_host_mirror, workspace, stream); }
CMI_API int cmi_lobpcg_residual_f32(int64_t n, const double *lambda_dev, const float *x, const float *ax, float *r, double *rr_dev, double *rr_host_mirror,
                                    void *workspace, void *stream)
{ return residual_impl<float>(n, lambda_dev, x, ax, r, rr_dev, rr_host_mirror, workspace, stream); }
CMI_API int cmi_lobpcg_gram_f64(int64_t n, const double *pp_dev, const double *x, const double *w, const double *aw, double *p, double *ap, double *gram_dev,
                                void *workspace, void *stream)
{ return gram_impl<double>(n, pp_dev, x, w, aw, p, ap, gram_dev, workspace, stream); }
CMI_API int cmi_lobpcg_gram_f32(int64_t n, const double *pp_dev, const float *x, const float *w, const float *aw, float *p, float *ap, double *gram_dev,
                                void *workspace, void *stream)
{ return gram_impl<float>(n, pp_dev, x, w, aw, p, ap, gram_dev, workspace, stream); }
CMI_API int cmi_lobpcg_update_f64(int64_t n, double cx, double cr, double cp, int first, double lambda_new, const double *w, const double *aw, double *p, double *ap,
                                  double *x, double *ax, double *r, double *scalars_dev, double *rr_host_mirror, void *workspace, void *stream)
{ return update_impl<double>(n, cx, cr, cp, first, lambda_new, w, aw, p, ap, x, ax, r, scalars_dev, rr_host_mirror, workspace, stream); }
CMI_API int cmi_lobpcg_update_f32(int64_t n, float cx, float cr, float cp, int first, float lambda_new, const float *w, const float *aw, float *p, float *ap, float *x,
                                  float *ax, float *r, double *scalars_dev, double *rr_host_mirror, void *workspace, void *stream)
{ return update_impl<float>(n, cx, cr, cp, first, lambda_new, w, aw, p, ap, x, ax, r, scalars_dev, rr_host_mirror, workspace, stream); }

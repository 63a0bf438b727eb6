// dense.hip -- cmi_dense_gemm_{f64,f32}: C (m x n) <- A (m x k) B (k x n), everything column-major, for m >> k, n: the product E = V S that
// turns the m Lanczos vectors of cusp::eigen::lanczos into Ritz vectors (cusp::blas::gemm on device_memory).
//
// Replaces (reference tree): cusp::blas::gemm of cusp/eigen/detail/lanczos.inl (a cuBLAS call there).  Without it the product is n k axpy
// launches that read A n times; here A is read ONCE per group of <= kCols = 8 columns of C.
//
// C(i, c) is the chain s = +0; for j = 0 .. k - 1: s = s + A(i, j) B(j, c) -- one multiply and one add per term, unfused (-ffp-contract=off),
// j ascending: the bits of the host triple loop.  k == 0 stores +0.
//
// A lane owns one 16-byte piece of rows (vec16: 2 doubles / 4 floats) and NC <= 8 accumulator pieces, one per column of the group.  A's columns
// are read with 16-byte loads when every A + j lda is 16-byte aligned (A aligned, and lda even / a multiple of 4, or k <= 1), element by
// element otherwise and in the ragged last piece; kUnroll = 4 columns of A are loaded before the first is used.  The loads carry the nt hint
// when one group covers n (A is then read once); with n > 8 the next group reads A again, and the loads are plain.  The NC columns of B the group
// needs are wave-uniform: the workgroup stages them in LDS kChunk = 64 rows of B at a time (any k: the chunks follow one another), laid out
// [row of B][column] so that one step reads NC consecutive values every lane shares.  C is written once with plain stores (16 bytes where
// C's columns are aligned).  Every element of C has one owner: no atomics, no reduction across lanes.  All offsets are 64-bit.
// Grid: one workgroup per 256 pieces up to kFusedMaxGrid workgroups, tile-strided past that; one launch per group of columns.
#include "blas1_shared.h"

namespace cmi {
namespace {

constexpr int kCols = 8;     // columns of C per pass over A
constexpr int kChunk = 64;   // rows of B staged at a time
constexpr int kUnroll = 4;   // loads of A in flight per lane

template <typename T, int NC>
__global__ void __launch_bounds__(kBlasBlock)
dense_gemm_kernel(int64_t m, int64_t k, const T *__restrict__ A, int64_t lda, const T *__restrict__ B, int64_t ldb, T *__restrict__ C, int64_t ldc, int wide_a,
                  int wide_c, int nt_a)
{
    typedef typename vec16<T>::type V;
    constexpr int W = vec16<T>::n;
    __shared__ T sB[kChunk * NC];
    const int64_t npieces = (m + W - 1) / W;
    const int64_t ntiles = (npieces + kBlasBlock - 1) / kBlasBlock;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (uniform in the workgroup: the barriers below are reached by all)
        const int64_t piece = tile * kBlasBlock + threadIdx.x;
        const bool active = piece < npieces;
        const int64_t e0 = piece * W;
        const int cnt = !active ? 0 : (m - e0 < W ? (int)(m - e0) : W);
        const bool full = cnt == W;
        V acc[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) acc[c] = V{};
        for (int64_t j0 = 0; j0 < k; j0 += kChunk) {
            const int kc = k - j0 < kChunk ? (int)(k - j0) : kChunk;
            __syncthreads(); // the chunk before this one has been read
            for (int idx = threadIdx.x; idx < kc * NC; idx += kBlasBlock) {
                const int c = idx / kc, jj = idx - c * kc; // consecutive lanes read down a column of B
                sB[jj * NC + c] = B[(int64_t)c * ldb + j0 + jj];
            }
            __syncthreads();
            if (active) {
                const T *a = A + j0 * lda + e0;
                int jj = 0;
                for (; jj + kUnroll <= kc; jj += kUnroll) {
                    V av[kUnroll];
#pragma unroll
                    for (int u = 0; u < kUnroll; u++) av[u] = ld_piece(a + (int64_t)(jj + u) * lda, cnt, full && wide_a, nt_a != 0);
#pragma unroll
                    for (int u = 0; u < kUnroll; u++)
#pragma unroll
                        for (int c = 0; c < NC; c++) {
                            const T b = sB[(jj + u) * NC + c];
#pragma unroll
                            for (int w = 0; w < W; w++) acc[c][w] = acc[c][w] + av[u][w] * b;
                        }
                }
                for (; jj < kc; jj++) {
                    const V av = ld_piece(a + (int64_t)jj * lda, cnt, full && wide_a, nt_a != 0);
#pragma unroll
                    for (int c = 0; c < NC; c++) {
                        const T b = sB[jj * NC + c];
#pragma unroll
                        for (int w = 0; w < W; w++) acc[c][w] = acc[c][w] + av[w] * b;
                    }
                }
            }
        }
        if (active) {
#pragma unroll
            for (int c = 0; c < NC; c++) st_piece(C + (int64_t)c * ldc + e0, acc[c], cnt, full && wide_c, false);
        }
    }
}

// every column start base + j ld (j < count) is 16-byte aligned
template <typename T> bool columns_aligned16(const T *base, int64_t ld, int64_t count)
{
    return reinterpret_cast<uintptr_t>(base) % 16 == 0 && (count <= 1 || (ld * (int64_t)sizeof(T)) % 16 == 0);
}

template <typename T, int NC>
void launch_group(int grid, int64_t m, int64_t k, const T *A, int64_t lda, const T *B, int64_t ldb, T *C, int64_t ldc, bool single_group, hipStream_t s)
{
    hipLaunchKernelGGL((dense_gemm_kernel<T, NC>), dim3(grid), dim3(kBlasBlock), 0, s, m, k, A, lda, B, ldb, C, ldc, (int)columns_aligned16(A, lda, k),
                       (int)columns_aligned16(C, ldc, (int64_t)NC), (int)single_group);
}

// bytes spanned by a column-major rows x cols operand with leading dimension ld (0 when empty)
template <typename T> size_t span_bytes(int64_t rows, int64_t cols, int64_t ld)
{
    return rows > 0 && cols > 0 ? ((size_t)(cols - 1) * (size_t)ld + (size_t)rows) * sizeof(T) : 0;
}

template <typename T>
int gemm_impl(int64_t m, int64_t n, int64_t k, const T *A, int64_t lda, const T *B, int64_t ldb, T *C, int64_t ldc, void *stream)
{
    if (m < 0 || n < 0 || k < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_dense_gemm: negative size");
    const bool has_a = m > 0 && k > 0, has_b = k > 0 && n > 0, has_c = m > 0 && n > 0;
    if ((has_a && lda < m) || (has_b && ldb < k) || (has_c && ldc < m))
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_dense_gemm: a leading dimension is smaller than the operand's rows");
    if ((has_a && !A) || (has_b && !B) || (has_c && !C)) return fail(CMI_ERROR_INVALID_VALUE, "cmi_dense_gemm: null array");
    if (any_overlap({{C, span_bytes<T>(m, n, ldc)}}, {{A, span_bytes<T>(m, k, lda)}, {B, span_bytes<T>(k, n, ldb)}}))
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_dense_gemm: C overlaps A or B");
    if (!has_c) return CMI_SUCCESS;
    const int grid = fused_grid(m, vec16<T>::n);
    const hipStream_t s = as_stream(stream);
    for (int64_t c0 = 0; c0 < n; c0 += kCols) {
        const T *b = B + c0 * ldb;
        T *c = C + c0 * ldc;
        switch (n - c0 < kCols ? (int)(n - c0) : kCols) {
        case 1: launch_group<T, 1>(grid, m, k, A, lda, b, ldb, c, ldc, n <= kCols, s); break;
        case 2: launch_group<T, 2>(grid, m, k, A, lda, b, ldb, c, ldc, n <= kCols, s); break;
        case 3: launch_group<T, 3>(grid, m, k, A, lda, b, ldb, c, ldc, n <= kCols, s); break;
        case 4: launch_group<T, 4>(grid, m, k, A, lda, b, ldb, c, ldc, n <= kCols, s); break;
        case 5: launch_group<T, 5>(grid, m, k, A, lda, b, ldb, c, ldc, n <= kCols, s); break;
        case 6: launch_group<T, 6>(grid, m, k, A, lda, b, ldb, c, ldc, n <= kCols, s); break;
        case 7: launch_group<T, 7>(grid, m, k, A, lda, b, ldb, c, ldc, n <= kCols, s); break;
        default: launch_group<T, 8>(grid, m, k, A, lda, b, ldb, c, ldc, n <= kCols, s); break;
        }
    }
    CMI_LAUNCH_CHECK("dense_gemm");
    return CMI_SUCCESS;
}

} // namespace
} // namespace cmi

using namespace cmi;

CMI_API int cmi_dense_gemm_f64(int64_t m, int64_t n, int64_t k, const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc, void *stream)
{ return gemm_impl<double>(m, n, k, A, lda, B, ldb, C, ldc, stream); }
CMI_API int cmi_dense_gemm_f32(int64_t m, int64_t n, int64_t k, const float *A, int64_t lda, const float *B, int64_t ldb, float *C, int64_t ldc, void *stream)
{ return gemm_impl<float>(m, n, k, A, lda, B, ldb, C, ldc, stream); }

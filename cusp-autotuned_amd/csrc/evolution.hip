// evolution.hip -- evolution strength of connection for smoothed aggregation: the transpose map of a symmetric
// pattern, the sparse product sampled on the pattern, and the measure built from them.
//
// Replaces (reference): cusp/precond/aggregation/system/detail/generic/evolution_strength.h -- its sort of the column indices
// (here: a binary search of the partner row, which also finds the patterns the sort silently assumes away), its
// incomplete_inner_functor (here: masked_product_kernel, the row staged in LDS once per wave) and its chain of some twenty
// Thrust transforms, scatters and a reduce_by_key (here: three per-entry kernels and one per-row kernel).
//
// Contract, as for amg.hip: every value is produced by ONE lane in the order include/cusp_mi355x.h states; multiply, add and
// divide are rounded separately (-ffp-contract=off); no atomics (the flag is a plain store of the same word).  Row offsets are
// clamped to [0, num_entries] before they address anything and a column outside the matrix addresses no row.
#include "amg_shared.h"

#include <cmath>
#include <limits>

namespace cmi {

constexpr int kEvoStage = 192; // entries of A that a wave stages: 64 entries lie in rows of at most 64 entries => a span below 64 + 2 * 63

// the largest i in [0, num_rows) with Ap[i] <= e (empty rows share their successor's offset and lose), as scale_rows_kernel
__device__ __forceinline__ int evo_row_of(int64_t num_rows, const int *__restrict__ Ap, int64_t e)
{
    int64_t lo = 0, hi = num_rows - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if ((int64_t)Ap[mid] <= e) lo = mid;
        else hi = mid - 1;
    }
    return (int)lo;
}

// ---- (a) t(e) = the position of (col(e), row(e)) ---------------------------------------------------------------------------
// One lane per index: index i <= num_rows checks the offsets (from 0 to num_entries without a decrease), index e < num_entries
// checks its entry (column inside the matrix and above its left neighbour's) and searches row col(e) for row(e).
// *bad = 1 on any miss.  rows (may be null): row(e), for the kernels that follow.
__global__ void __launch_bounds__(kAmgBlock)
transpose_positions_kernel(int64_t num_rows, int64_t num_entries, const int *__restrict__ Ap, const int *__restrict__ Aj, int *__restrict__ tpos, int *__restrict__ rows,
                           int *__restrict__ bad)
{
    const int64_t e = (int64_t)blockIdx.x * kAmgBlock + threadIdx.x;
    bool ok = true;
    if (e < num_rows) ok = Ap[e] >= 0 && Ap[e] <= Ap[e + 1] && (int64_t)Ap[e + 1] <= num_entries && (e > 0 || Ap[0] == 0);
    if (e == num_rows) ok = (int64_t)Ap[e] == num_entries;
    if (e < num_entries) {
        const int row = evo_row_of(num_rows, Ap, e);
        const int lo = amg_clamp(Ap[row], num_entries);
        const int col = Aj[e];
        int at = -1;
        if (col < 0 || (int64_t)col >= num_rows || (e > lo && Aj[e - 1] >= col)) ok = false;
        else {
            int a = amg_clamp(Ap[col], num_entries), b = amg_clamp(Ap[col + 1], num_entries); // the first position in [a, b) whose column is >= row
            const int end = b;
            while (a < b) {
                const int mid = a + ((b - a) >> 1);
                if (Aj[mid] < row) a = mid + 1;
                else b = mid;
            }
            if (a < end && Aj[a] == row) at = a;
            else ok = false;
        }
        tpos[e] = at;
        if (rows) rows[e] = row;
    }
    if (!ok) *bad = 1;
}

// ---- (b) out[e] = sum of Vx[p] * Wx[q] over the common columns of rows row(e) and col(e) ------------------------------------
// One wave (= one block) owns 64 consecutive ENTRIES, one per lane, so no lane idles whatever the row lengths.  The rows those
// entries lie in are contiguous: the lanes whose row has at most 64 entries stage the span of their rows (columns and values,
// at most 190 entries) in LDS once, and every lane then merges its partner row (read from global memory) against its own row's
// piece of the span.  A row of more than 64 entries is staged by the whole wave in chunks of kEvoStage; each of its lanes keeps
// its own place in its partner row and its own sum across the chunks, so the chain is the one merge in ascending column order.
// (Offsets that decrease or overlap can make the short rows' span exceed the stage: then every lane takes the chunked path.)
template <typename T>
__global__ void __launch_bounds__(kWave)
masked_product_kernel(int64_t num_rows, int64_t num_entries, const int *__restrict__ Ap, const int *__restrict__ Aj, const T *__restrict__ Vx, const T *__restrict__ Wx,
                      const int *__restrict__ rows, T *__restrict__ out)
{
    __shared__ int sc[kEvoStage];
    __shared__ T sv[kEvoStage];
    const int lane = threadIdx.x;
    const int64_t e = (int64_t)blockIdx.x * kWave + lane;
    const bool live = e < num_entries;
    int row = 0, rlo = 0, rhi = 0, q = 0, qe = 0;
    if (live) {
        row = rows ? rows[e] : evo_row_of(num_rows, Ap, e);
        rlo = amg_clamp(Ap[row], num_entries);
        rhi = amg_clamp(Ap[row + 1], num_entries);
        if (rhi < rlo) rhi = rlo;
        const int col = Aj[e];
        if (col >= 0 && (int64_t)col < num_rows) {
            q = amg_clamp(Ap[col], num_entries);
            qe = amg_clamp(Ap[col + 1], num_entries);
        }
    }
    bool is_long = live && rhi - rlo > kWave;
    // the span of the short rows: wave-wide minimum and maximum by a butterfly of shuffles
    int slo = (live && !is_long) ? rlo : INT32_MAX, shi = (live && !is_long) ? rhi : 0;
    for (int d = kWave / 2; d > 0; d >>= 1) {
        const int l2 = __shfl_xor(slo, d), h2 = __shfl_xor(shi, d);
        slo = l2 < slo ? l2 : slo;
        shi = h2 > shi ? h2 : shi;
    }
    const bool staged = shi > slo && shi - slo <= kEvoStage; // (wave-uniform)
    if (!staged) is_long = live;
    T sum = T(0);
    if (staged) {
        for (int k = lane; k < shi - slo; k += kWave) {
            sc[k] = Aj[slo + k];
            sv[k] = Vx[slo + k];
        }
    }
    __syncthreads();
    if (staged && live && !is_long) {
        int p = rlo - slo;
        const int pe = rhi - slo;
        while (p < pe && q < qe) {
            const int a = sc[p], b = Aj[q];
            if (a == b) {
                const T prod = sv[p] * Wx[q];
                sum = sum + prod;
                p++;
                q++;
            } else if (a < b) p++;
            else q++;
        }
    }
    unsigned long long todo = __ballot(is_long); // every lane of the wave is here: no lane has left
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        const int r = __shfl(row, src), lo = __shfl(rlo, src), hi = __shfl(rhi, src);
        const bool mine = is_long && row == r;
        todo &= ~__ballot(mine);
        for (int base = lo; base < hi; base += kEvoStage) {
            const int cnt = hi - base < kEvoStage ? hi - base : kEvoStage;
            __syncthreads(); // the stage is free: every lane has finished with what it held
            for (int k = lane; k < cnt; k += kWave) {
                sc[k] = Aj[base + k];
                sv[k] = Vx[base + k];
            }
            __syncthreads();
            if (mine) {
                int p = 0;
                while (p < cnt && q < qe) {
                    const int a = sc[p], b = Aj[q];
                    if (a == b) {
                        const T prod = sv[p] * Wx[q];
                        sum = sum + prod;
                        p++;
                        q++;
                    } else if (a < b) p++;
                    else q++;
                }
            }
        }
    }
    if (live) out[e] = sum;
}

template <typename T>
static hipError_t launch_masked_product(int64_t num_rows, int64_t num_entries, const int *Ap, const int *Aj, const T *Vx, const T *Wx, const int *rows, T *out, hipStream_t s)
{
    return launch(masked_product_kernel<T>, (unsigned)ceil_div(num_entries, kWave), kWave, 0, s, num_rows, num_entries, Ap, Aj, Vx, Wx, rows, out);
}

static int evo_sizes(const char *who, int64_t num_rows, int64_t num_entries)
{
    if (num_rows < 0 || num_entries < 0) {
        set_error("%s: negative size", who);
        return CMI_ERROR_INVALID_VALUE;
    }
    if (num_rows > INT32_MAX - 1 || num_entries > kAmgCeiling) {
        set_error("%s: sizes exceed the int32 index type", who);
        return CMI_ERROR_INVALID_VALUE;
    }
    if (num_entries > 0 && num_rows == 0) {
        set_error("%s: entries without rows", who);
        return CMI_ERROR_INVALID_VALUE;
    }
    return CMI_SUCCESS;
}

static int transpose_positions(int64_t num_rows, const int *Ap, const int *Aj, int *tpos, int *conforming_host, void *stream)
{
    if (num_rows < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_transpose_positions: negative size");
    if (num_rows > INT32_MAX - 1) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_transpose_positions: sizes exceed the int32 index type");
    if (!conforming_host || !Ap) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_transpose_positions: null array");
    hipStream_t s = as_stream(stream);
    // the entry count is the last offset (the one number this call reads before it checks anything)
    int last = 0;
    CMI_HIP(hipMemcpyAsync(&last, Ap + num_rows, sizeof(int), hipMemcpyDeviceToHost, s));
    CMI_HIP(hipStreamSynchronize(s));
    const int64_t num_entries = last;
    if (num_entries < 0 || num_entries > kAmgCeiling || (num_entries > 0 && num_rows == 0)) {
        *conforming_host = 0;
        return CMI_SUCCESS;
    }
    if (num_entries > 0 && (!Aj || !tpos)) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_transpose_positions: null array");
    device_counters<int> bad;
    hipError_t e = bad.open(s);
    const int64_t lanes = (num_entries > num_rows + 1 ? num_entries : num_rows + 1);
    if (e == hipSuccess) e = launch(transpose_positions_kernel, amg_blocks(lanes), kAmgBlock, 0, s, num_rows, num_entries, Ap, Aj, tpos, nullptr, bad.dev());
    if (e == hipSuccess) e = bad.fetch(s);
    else (void)hipStreamSynchronize(s); // (the flag goes when this returns)
    if (e != hipSuccess) return hip_fail(e, "cmi_csr_transpose_positions");
    *conforming_host = bad.host[0] ? 0 : 1;
    return CMI_SUCCESS;
}

template <typename T> static int masked_product(int64_t num_rows, const int *Ap, const int *Aj, const T *Vx, const T *Wx, T *out, void *stream)
{
    if (num_rows < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_masked_product: negative size");
    if (num_rows > INT32_MAX - 1) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_masked_product: sizes exceed the int32 index type");
    if (!Ap) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_masked_product: null array");
    hipStream_t s = as_stream(stream);
    int last = 0; // the entry count is the last offset
    CMI_HIP(hipMemcpyAsync(&last, Ap + num_rows, sizeof(int), hipMemcpyDeviceToHost, s));
    CMI_HIP(hipStreamSynchronize(s));
    const int64_t num_entries = last;
    if (num_entries < 0 || num_entries > kAmgCeiling || (num_entries > 0 && num_rows == 0))
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_masked_product: the last row offset is not an entry count");
    if (num_entries > 0 && (!Aj || !Vx || !Wx || !out)) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_masked_product: null array");
    if (num_entries == 0) return CMI_SUCCESS;
    const hipError_t e = launch_masked_product<T>(num_rows, num_entries, Ap, Aj, Vx, Wx, nullptr, out, s);
    return e == hipSuccess ? CMI_SUCCESS : hip_fail(e, "launch csr_masked_product");
}

// ---- (c) the measure ----------------------------------------------------------------------------------------------------------
// steps 1 and 6: cusp::extract_diagonal's kernel (0 where none is stored, else +0 plus the entry); the offsets have been checked by then
static int diagonal_of(int64_t n, const int *Ap, const int *Aj, const double *Ax, double *d, void *stream) { return cmi_csr_diagonal_f64(n, Ap, Aj, Ax, d, 0, stream); }
static int diagonal_of(int64_t n, const int *Ap, const int *Aj, const float *Ax, float *d, void *stream) { return cmi_csr_diagonal_f32(n, Ap, Aj, Ax, d, 0, stream); }


// steps 2 and 4: v[e] = T((row == col) - (1.0 / rho) * double(Ax[e] / D[row])), rho already rounded to T (inv = 1.0 / double(T(rho)))
template <typename T>
__global__ void __launch_bounds__(kAmgBlock)
evo_scale_kernel(int64_t num_entries, const int *__restrict__ rows, const int *__restrict__ Aj, const T *__restrict__ Ax, const T *__restrict__ D, double inv, T *__restrict__ v)
{
    const int64_t e = (int64_t)blockIdx.x * kAmgBlock + threadIdx.x;
    if (e >= num_entries) return;
    const int row = rows[e];
    const T scaled = Ax[e] / D[row];
    const double prod = inv * (double)scaled;
    v[e] = (T)((row == Aj[e] ? 1.0 : 0.0) - prod);
}

template <typename T>
__global__ void __launch_bounds__(kAmgBlock) evo_gather_kernel(int64_t num_entries, const int *__restrict__ tpos, const T *__restrict__ v, T *__restrict__ w)
{
    const int64_t e = (int64_t)blockIdx.x * kAmgBlock + threadIdx.x;
    if (e < num_entries) w[e] = v[tpos[e]];
}

// steps 7 to 14: from data to a
template <typename T>
__global__ void __launch_bounds__(kAmgBlock)
evo_ratio_kernel(int64_t num_entries, const int *__restrict__ rows, const int *__restrict__ Aj, const T *__restrict__ data, const T *__restrict__ DAt, const T *__restrict__ B,
                 T perfect, T *__restrict__ a_out)
{
    const int64_t e = (int64_t)blockIdx.x * kAmgBlock + threadIdx.x;
    if (e >= num_entries) return;
    const T d = data[e];
    T b = B[Aj[e]];
    if (b == T(0)) b = T(1);
    const T scaled_row = T(1) * DAt[rows[e]];
    T a = scaled_row * b;
    const T angle = d * a;
    const bool neg = angle < T(0);
    a = a / d;
    const bool weak = a < (T)1e-4;
    a = (T)fabs(1.0 - (double)a);
    if (neg || weak) a = T(0);
    if (a < perfect && a != T(0)) a = (T)1e-4;
    a_out[e] = a;
}

// step 15 for one entry: s = T(0.5 * double(T(a[e] + a[t(e)])))
template <typename T> __device__ __forceinline__ T evo_half_sum(const T *__restrict__ a, const int *__restrict__ tpos, int64_t e)
{
    const T both = a[e] + a[tpos[e]];
    return (T)(0.5 * (double)both);
}
template <typename T> __device__ __forceinline__ T evo_non_zero_minimum(T lhs, T rhs)
{
    if (lhs == T(0)) return rhs;
    if (rhs == T(0)) return lhs;
    return lhs < rhs ? lhs : rhs;
}

// step 16's minimum: small[i] = the left-to-right non_zero_minimum chain over row i's s, started from the row's first entry.
// One wave per 64 consecutive rows, as strength_kernel: a row of at most 64 entries is walked by its own lane; a longer row by
// the whole wave, 64 entries loaded at a time and then chained in storage order through shuffles (the operator is not
// associative once a NaN is among the values, so the order is kept).
template <typename T>
__global__ void __launch_bounds__(kAmgBlock)
evo_row_minimum_kernel(int64_t num_rows, int64_t num_entries, const int *__restrict__ Ap, const int *__restrict__ tpos, const T *__restrict__ a, T *__restrict__ small)
{
    const int64_t row = (int64_t)blockIdx.x * kAmgBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    int lo = 0, hi = 0;
    if (row < num_rows) {
        lo = amg_clamp(Ap[row], num_entries);
        hi = amg_clamp(Ap[row + 1], num_entries);
        if (hi < lo) hi = lo;
    }
    const bool is_long = hi - lo > kWave;
    T acc = std::numeric_limits<T>::max(); // (an empty row: never read)
    if (!is_long && hi > lo) {
        acc = evo_half_sum(a, tpos, lo);
        for (int jj = lo + 1; jj < hi; jj++) acc = evo_non_zero_minimum(acc, evo_half_sum(a, tpos, jj));
    }
    unsigned long long todo = __ballot(is_long);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int rlo = __shfl(lo, src), rhi = __shfl(hi, src);
        T chain = T(0);
        for (int base = rlo; base < rhi; base += kWave) {
            const int jj = base + lane;
            const T mine = jj < rhi ? evo_half_sum(a, tpos, jj) : T(0);
            const int cnt = rhi - base < kWave ? rhi - base : kWave;
            for (int k = 0; k < cnt; k++) {
                const T next = __shfl(mine, k);
                chain = (base == rlo && k == 0) ? next : evo_non_zero_minimum(chain, next);
            }
        }
        if (lane == src) acc = chain;
    }
    if (row < num_rows) small[row] = acc;
}

// steps 15 to 17 for one entry x: the symmetrised value, filtered against its row's minimum, 1 on the diagonal
template <typename T>
__device__ __forceinline__ T evo_filtered(const T *__restrict__ a, const int *__restrict__ tpos, const int *__restrict__ rows, const int *__restrict__ Aj,
                                          const T *__restrict__ small, bool filter, T epsilon, int64_t x)
{
    const int row = rows[x];
    if (row == Aj[x]) return T(1);
    T s = evo_half_sum(a, tpos, x);
    if (filter) {
        const T limit = epsilon * small[row];
        if (s >= limit) s = T(0);
    }
    return s;
}

// steps 15 to 18 and the flags of step 19: s[e] = s'(e) + s'(t(e)); keep[e] = s[e] != 0 (keep[num_entries] = 0)
template <typename T>
__global__ void __launch_bounds__(kAmgBlock)
evo_measure_kernel(int64_t num_entries, const int *__restrict__ rows, const int *__restrict__ Aj, const int *__restrict__ tpos, const T *__restrict__ a,
                   const T *__restrict__ small, int filter, T epsilon, T *__restrict__ s_out, int *__restrict__ keep)
{
    const int64_t e = (int64_t)blockIdx.x * kAmgBlock + threadIdx.x;
    if (e > num_entries) return;
    if (e == num_entries) {
        keep[e] = 0;
        return;
    }
    const T here = evo_filtered(a, tpos, rows, Aj, small, filter != 0, epsilon, e);
    const T there = evo_filtered(a, tpos, rows, Aj, small, filter != 0, epsilon, (int64_t)tpos[e]);
    const T s = here + there;
    s_out[e] = s;
    keep[e] = s != T(0) ? 1 : 0;
}

// the compaction: entry e goes to pos[e] when kept; Sp[i] = pos[Ap[i]] (index num_entries + i serves row i, 0 <= i <= num_rows)
template <typename T>
__global__ void __launch_bounds__(kAmgBlock)
evo_compact_kernel(int64_t num_rows, int64_t num_entries, const int *__restrict__ Ap, const int *__restrict__ Aj, const T *__restrict__ s, const int *__restrict__ keep,
                   const int *__restrict__ pos, int *__restrict__ Sp, int *__restrict__ Sj, T *__restrict__ Sx, int64_t capacity)
{
    const int64_t e = (int64_t)blockIdx.x * kAmgBlock + threadIdx.x;
    if (e < num_entries) {
        const int64_t at = pos[e];
        if (keep[e] && at < capacity) {
            Sj[at] = Aj[e];
            Sx[at] = s[e];
        }
    } else if (e - num_entries <= num_rows) {
        const int64_t i = e - num_entries;
        Sp[i] = pos[amg_clamp(Ap[i], num_entries)];
    }
}

template <typename T>
static int evolution_strength(int64_t num_rows, int64_t num_entries, const int *Ap, const int *Aj, const T *Ax, const T *B, double rho_DinvA, double epsilon, int *Sp,
                              int *Sj, T *Sx, int64_t capacity, int *conforming_host, void *stream)
{
    if (capacity < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_evolution_strength: negative size");
    if (int st = evo_sizes("cmi_csr_evolution_strength", num_rows, num_entries)) return st;
    if (capacity < num_entries) {
        set_error("cmi_csr_evolution_strength: capacity %lld is below the %lld entries of A", (long long)capacity, (long long)num_entries);
        return CMI_ERROR_INVALID_VALUE;
    }
    if (!(rho_DinvA != 0.0) || !std::isfinite(rho_DinvA)) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_evolution_strength: rho_DinvA must be finite and not zero");
    if (!conforming_host || !Sp || (num_rows > 0 && (!Ap || !B)) || (num_entries > 0 && (!Aj || !Ax || !Sj || !Sx)))
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_evolution_strength: null array");
    *conforming_host = 0;
    hipStream_t s = as_stream(stream);
    if (num_rows == 0 || num_entries == 0) { // nothing to keep: an all-zero Sp
        CMI_HIP(hipMemsetAsync(Sp, 0, (size_t)(num_rows + 1) * sizeof(int), s));
        CMI_HIP(hipStreamSynchronize(s));
        *conforming_host = 1;
        return CMI_SUCCESS;
    }
    const size_t M = (size_t)num_entries, N = (size_t)num_rows;
    device_arena arena;
    device_counters<int> bad;
    device_array<unsigned char> scan_temp;
    hipError_t e = arena.open(4 * device_arena::padded((M + 1) * sizeof(int)) + 3 * device_arena::padded(M * sizeof(T)) + 3 * device_arena::padded(N * sizeof(T)));
    if (e == hipSuccess) e = bad.open(s);
    if (e != hipSuccess) return hip_fail(e, "cmi_csr_evolution_strength: scratch");
    int *const tpos = arena.take<int>(M + 1), *const rows = arena.take<int>(M + 1), *const keep = arena.take<int>(M + 1), *const pos = arena.take<int>(M + 1);
    T *const v = arena.take<T>(M), *const w = arena.take<T>(M), *const data = arena.take<T>(M);
    T *const D = arena.take<T>(N), *const DAt = arena.take<T>(N), *const small = arena.take<T>(N);
    if (!small) return fail(CMI_ERROR_ALLOC,"cmi_csr_evolution_strength: the scratch reservation is too small");
    const unsigned entry_blocks = amg_blocks(num_entries);
    const int64_t check_lanes = num_entries > num_rows + 1 ? num_entries : num_rows + 1;
    e = launch(transpose_positions_kernel, amg_blocks(check_lanes), kAmgBlock, 0, s, num_rows, num_entries, Ap, Aj, tpos, rows, bad.dev());
    if (e == hipSuccess) e = bad.fetch(s); // the flag is read once, before anything of the caller's is written
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s); // (the arena goes when this returns)
        return hip_fail(e, "cmi_csr_evolution_strength: checking the pattern");
    }
    if (bad.host[0]) return CMI_SUCCESS; // *conforming_host == 0: the caller refuses
    const T rho_t = (T)rho_DinvA; // the reference's functor holds rho in the value type
    const double inv = 1.0 / (double)rho_t;
    const T perfect = std::sqrt(std::numeric_limits<T>::epsilon());
    const int filter = epsilon != (double)std::numeric_limits<T>::infinity();
    T *const a = v, *const s_all = w; // v and w are done with once `data` stands
    int st = diagonal_of(num_rows, Ap, Aj, Ax, D, stream);
    if (st == CMI_SUCCESS) {
        e = launch(evo_scale_kernel<T>, entry_blocks, kAmgBlock, 0, s, num_entries, rows, Aj, Ax, D, inv, v);
        if (e == hipSuccess) e = launch(evo_gather_kernel<T>, entry_blocks, kAmgBlock, 0, s, num_entries, tpos, v, w);
        if (e == hipSuccess) e = launch_masked_product<T>(num_rows, num_entries, Ap, Aj, v, w, rows, data, s);
        if (e != hipSuccess) st = hip_fail(e, "cmi_csr_evolution_strength: the masked product");
    }
    if (st == CMI_SUCCESS) st = diagonal_of(num_rows, Ap, Aj, data, DAt, stream);
    if (st == CMI_SUCCESS) {
        e = launch(evo_ratio_kernel<T>, entry_blocks, kAmgBlock, 0, s, num_entries, rows, Aj, data, DAt, B, perfect, a);
        if (e == hipSuccess && filter) e = launch(evo_row_minimum_kernel<T>, amg_blocks(num_rows), kAmgBlock, 0, s, num_rows, num_entries, Ap, tpos, a, small);
        if (e == hipSuccess) e = launch(evo_measure_kernel<T>, amg_blocks(num_entries + 1), kAmgBlock, 0, s, num_entries, rows, Aj, tpos, a, small, filter, (T)epsilon, s_all, keep);
        if (e == hipSuccess) e = exclusive_offsets(scan_temp, keep, pos, num_entries, s);
        if (e == hipSuccess)
            e = launch(evo_compact_kernel<T>, amg_blocks(num_entries + num_rows + 1), kAmgBlock, 0, s, num_rows, num_entries, Ap, Aj, s_all, keep, pos, Sp, Sj, Sx, capacity);
        if (e != hipSuccess) st = hip_fail(e, "cmi_csr_evolution_strength");
    }
    // the scratch is released when this returns: everything enqueued above must have finished with it
    e = hipStreamSynchronize(s);
    if (st == CMI_SUCCESS && e != hipSuccess) st = hip_fail(e, "cmi_csr_evolution_strength");
    if (st == CMI_SUCCESS) *conforming_host = 1;
    return st;
}

} // namespace cmi

CMI_API int cmi_csr_transpose_positions(int64_t num_rows, const int32_t *Ap, const int32_t *Aj, int32_t *tpos, int *conforming_host, void *stream)
{ return cmi::transpose_positions(num_rows, Ap, Aj, tpos, conforming_host, stream); }

CMI_API int cmi_csr_masked_product_f64(int64_t num_rows, const int32_t *Ap, const int32_t *Aj, const double *Vx, const double *Wx, double *out, void *stream)
{ return cmi::masked_product<double>(num_rows, Ap, Aj, Vx, Wx, out, stream); }
CMI_API int cmi_csr_masked_product_f32(int64_t num_rows, const int32_t *Ap, const int32_t *Aj, const float *Vx, const float *Wx, float *out, void *stream)
{ return cmi::masked_product<float>(num_rows, Ap, Aj, Vx, Wx, out, stream); }

CMI_API int cmi_csr_evolution_strength_f64(int64_t num_rows, int64_t num_entries, const int32_t *Ap, const int32_t *Aj, const double *Ax, const double *B,
                                           double rho_DinvA, double epsilon, int32_t *Sp, int32_t *Sj, double *Sx, int64_t capacity, int *conforming_host,
                                           void *stream)
{ return cmi::evolution_strength<double>(num_rows, num_entries, Ap, Aj, Ax, B, rho_DinvA, epsilon, Sp, Sj, Sx, capacity, conforming_host, stream); }
CMI_API int cmi_csr_evolution_strength_f32(int64_t num_rows, int64_t num_entries, const int32_t *Ap, const int32_t *Aj, const float *Ax, const float *B,
                                           double rho_DinvA, double epsilon, int32_t *Sp, int32_t *Sj, float *Sx, int64_t capacity, int *conforming_host,
                                           void *stream)
{ return cmi::evolution_strength<float>(num_rows, num_entries, Ap, Aj, Ax, B, rho_DinvA, epsilon, Sp, Sj, Sx, capacity, conforming_host, stream); }

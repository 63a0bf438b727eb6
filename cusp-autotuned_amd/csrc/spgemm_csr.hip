// spgemm_csr.hip -- CSR times CSR (SpGEMM): C = A B, A m x k, B k x n, C returned through a handle.
//
// Replaces (reference): cusp/multiply.h generalized_spgemm; device path cusp/system/cuda/detail/multiply/spgemm.h (expand the
// products in slabs, sort by (row, column), reduce_by_key, concatenate); host-order oracle
// cusp/system/detail/sequential/multiply/csr_spgemm.h:102-131.
//
// Contract.  Structure: one entry per distinct (i, c) with at least one structural product A(i,j) B(j,c), columns
// strictly ascending in every row, exact-zero sums KEPT (as the reference's device path keeps them); it depends on the two
// patterns only.  Values: s = T(0); for jj over row i of A in storage order, for kk over row Aj[jj] of B in storage order with
// Bj[kk] == c: s = s + (Ax[jj] * Bx[kk]) -- multiply and add rounded separately (-ffp-contract=off), one lane per output entry,
// no atomics on values and no re-association: the bits of the host loop.  (The reference's device path leaves the order of a
// segment's sum to reduce_by_key; here it is fixed.)
//
// Method: expand, sort, compress, in row slabs.
//   1. per entry e of A the length of B's row Aj[e] (int64), exclusive scan -> entry_start[e]: the position of e's first product
//      in EXPANSION ORDER (rows of A in order, a row's entries in storage order, B's row in storage order).  The products of row i
//      start at entry_start[Ap[i]]: the host reads those m + 1 numbers and cuts the rows into slabs of at most W products.
//   2. per slab: one lane per PRODUCT (two bounded binary searches: its entry of A, its row) writes the key
//      (local row << column bits) | column and the value Ax[e] * Bx[kk]; rocprim::radix_sort_pairs (stable LSD radix sort, a ROCm
//      library primitive as in sort.hip) sorts the keys carrying the product's position, on the key bits the slab needs only;
//      equal keys therefore stay in expansion order.  Segment heads are marked and scanned; one lane per output entry adds
//      its segment's products in sorted order from +0 and writes column and value; one lane per row finds its first entry by a
//      lower bound on the sorted keys (no atomics anywhere, not even on counts).
//   3. the slab results stay in the handle as pieces and are concatenated into the caller's arrays by cmi_spgemm_take_*.
// A row with more than W products is refused (CMI_ERROR_NOT_SUPPORTED): a chain is never split across slabs.
//
// Bad indices are the caller's error, but none reaches scratch unclamped: an entry of A whose column lies outside [0, k), or
// whose row of B has offsets outside [0, b_entries] or decreasing, contributes no product; Ap is clamped to [0, a_entries] where
// it addresses entry_start; a column of B is masked to the key's column bits.
//
// Workgroup- or wave-private LDS tiles for short rows (the AMG case) are NOT implemented: cmi_spgemm_info reports 0 rows in
// tiles and cmi_spgemm_limits a tile size of 0.
#include "setup_scan.h"

#include <algorithm>
#include <new>
#include <vector>

namespace cmi {

constexpr int64_t kSpgemmCeiling = (int64_t)INT32_MAX - 65536; // entries of A, B and C (the CSR ceiling)
constexpr int64_t kSpgemmWorkspaceCap = (int64_t)1 << 26;     // default W at most (~3 GB of scratch in f64)
constexpr int64_t kSpgemmWorkspaceMax = kSpgemmCeiling;        // positions inside a slab are 32-bit
constexpr int kSpgemmTempPerProduct = 16;                      // bytes per product allowed for the sort's own ping-pong storage when W is derived from free memory

static int64_t g_spgemm_workspace = 0; // cmi_spgemm_set_workspace; 0: the default rule

static int64_t scratch_bytes_per_product(size_t value_bytes)
{
    // keys in / out 8 + 8, position 4, segment index 4, value, the sort's temporary storage
    return 8 + 8 + 4 + 4 + (int64_t)value_bytes + kSpgemmTempPerProduct;
}

__device__ __forceinline__ int clamp_offset(int p, int64_t entries) { return p < 0 ? 0 : ((int64_t)p > entries ? (int)entries : p); }

// len[e] = products entry e of A expands to = the length of B's row Aj[e]; len[a_entries] = 0 (the scan's total lands there)
__global__ void __launch_bounds__(256) spgemm_entry_products_kernel(int64_t a_entries, int64_t k, int64_t b_entries, const int *__restrict__ Aj,
                                                                    const int *__restrict__ Bp, int64_t *__restrict__ len)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e <= a_entries; e += stride) {
        int64_t l = 0;
        if (e < a_entries) {
            const int j = Aj[e];
            if (j >= 0 && (int64_t)j < k) {
                const int lo = Bp[j], hi = Bp[j + 1];
                if (lo >= 0 && hi > lo && (int64_t)hi <= b_entries) l = (int64_t)hi - lo;
            }
        }
        len[e] = l;
    }
}

// row_start[i] = entry_start[Ap[i]] for i in [0, m]: the position of row i's first product
__global__ void __launch_bounds__(256) spgemm_row_products_kernel(int64_t m, int64_t a_entries, const int *__restrict__ Ap,
                                                                  const int64_t *__restrict__ entry_start, int64_t *__restrict__ row_start)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= m; i += stride) row_start[i] = entry_start[clamp_offset(Ap[i], a_entries)];
}

// One lane per product p of the slab (rows [r0, r1), products [base, base + P) of the expansion order).
template <typename T>
__global__ void __launch_bounds__(256)
spgemm_expand_kernel(int64_t P, int64_t base, int r0, int r1, int64_t a_entries, const int *__restrict__ Ap, const int *__restrict__ Aj,
                     const T *__restrict__ Ax, const int *__restrict__ Bp, const int *__restrict__ Bj, const T *__restrict__ Bx,
                     const int64_t *__restrict__ entry_start, int col_bits, uint32_t col_mask, uint64_t *__restrict__ keys, T *__restrict__ vals)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int64_t g = base + p;
    const int e_lo = clamp_offset(Ap[r0], a_entries), e_hi = clamp_offset(Ap[r1], a_entries);
    // the entry of A: the largest e in [e_lo, e_hi) with entry_start[e] <= g (entries without products share their successor's start and lose)
    int64_t lo = e_lo, hi = (int64_t)e_hi - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (entry_start[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    const int e = (int)lo;
    // its row: the largest i in [r0, r1) with Ap[i] <= e (empty rows share their successor's offset and lose)
    int64_t rl = r0, rh = (int64_t)r1 - 1;
    while (rl < rh) {
        const int64_t mid = (rl + rh + 1) >> 1;
        if (clamp_offset(Ap[mid], a_entries) <= e) rl = mid;
        else rh = mid - 1;
    }
    const int j = Aj[e]; // (e has products: spgemm_entry_products_kernel found j and B's offsets in range)
    const int64_t kk = (int64_t)Bp[j] + (g - entry_start[e]);
    keys[p] = ((uint64_t)(uint32_t)(rl - r0) << col_bits) | (uint64_t)((uint32_t)Bj[kk] & col_mask);
    vals[p] = Ax[e] * Bx[kk];
}

// head[q] = 1 where a new (row, column) starts in the sorted keys
__global__ void __launch_bounds__(256) spgemm_heads_kernel(int64_t P, const uint64_t *__restrict__ keys, uint32_t *__restrict__ head)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= P) return;
    head[q] = (q == 0 || keys[q] != keys[q - 1]) ? 1u : 0u;
}

// seg = inclusive scan of the heads: the head of output entry u (seg == u + 1) records where its segment starts
__global__ void __launch_bounds__(256)
spgemm_starts_kernel(int64_t P, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ seg, uint32_t *__restrict__ starts)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= P) return;
    if (q == 0 || keys[q] != keys[q - 1]) starts[seg[q] - 1] = (uint32_t)q;
}

// ONE lane per output entry: the segment's products in sorted order = expansion order, from +0
template <typename T>
__global__ void __launch_bounds__(256)
spgemm_sum_kernel(int64_t U, int64_t P, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ starts,
                  const T *__restrict__ vals, uint32_t col_mask, int *__restrict__ Cj, T *__restrict__ Cx)
{
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= U) return;
    const int64_t q0 = starts[u], q1 = u + 1 < U ? (int64_t)starts[u + 1] : P;
    T s = T(0);
    for (int64_t q = q0; q < q1; q++) s = s + vals[perm[q]];
    Cj[u] = (int)((uint32_t)keys[q0] & col_mask);
    Cx[u] = s;
}

// Cp[r0 + i] = entries before this slab + segment heads before the first key of local row i
__global__ void __launch_bounds__(256) spgemm_row_offsets_kernel(int64_t rows, int64_t P, int r0, int64_t entries_before, int col_bits,
                                                                 const uint64_t *__restrict__ keys, const uint32_t *__restrict__ seg, int *__restrict__ Cp)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const uint64_t target = (uint64_t)i << col_bits;
    int64_t lo = 0, hi = P; // the first q with keys[q] >= target
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < target) lo = mid + 1;
        else hi = mid;
    }
    Cp[r0 + i] = (int)(entries_before + (lo > 0 ? (int64_t)seg[lo - 1] : 0));
}

static int spgemm_bits_for(int64_t count) // how many low bits hold every value in [0, count)
{
    int b = 1;
    while (b < 32 && ((int64_t)1 << b) < count) b++;
    return b;
}

static unsigned blocks_for(int64_t n) { return (unsigned)(n < 1 ? 1 : ceil_div(n, 256)); }
static int capped_grid(int64_t n)
{
    int64_t b = ceil_div(n, 256);
    if (b > kCus * 16) b = kCus * 16;
    return b < 1 ? 1 : (int)b;
}

} // namespace cmi

// What cmi_spgemm_csr_* returns: C's row offsets and its entries as one piece per slab, all on the device.
struct cmi_spgemm {
    int dtype = CMI_F64;
    int64_t m = 0, num_entries = 0;
    cmi::device_array<int32_t> Cp; // m + 1; empty: every offset is 0
    struct piece { cmi::device_array<int32_t> Cj; cmi::device_array<unsigned char> Cx; int64_t count = 0; }; // Cx: `count` values of dtype
    std::vector<piece> pieces;
    int64_t products = 0, slabs = 0, rows_in_tiles = 0, rows_in_slabs = 0;
};

namespace cmi {

template <typename T>
static int spgemm_csr(int64_t m, int64_t k, int64_t n, int64_t a_entries, const int *Ap, const int *Aj, const T *Ax, int64_t b_entries, const int *Bp,
                      const int *Bj, const T *Bx, cmi_spgemm **result, void *stream)
{
    if (!result) return fail(CMI_ERROR_INVALID_VALUE, "cmi_spgemm_csr: result is NULL");
    *result = nullptr;
    if (m < 0 || k < 0 || n < 0 || a_entries < 0 || b_entries < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_spgemm_csr: negative size");
    if (m > INT32_MAX || k > INT32_MAX || n > INT32_MAX || a_entries > kSpgemmCeiling || b_entries > kSpgemmCeiling)
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_spgemm_csr: sizes exceed the int32 index type");
    if ((m > 0 && !Ap) || (a_entries > 0 && (!Aj || !Ax)) || (k > 0 && a_entries > 0 && !Bp) || (b_entries > 0 && (!Bj || !Bx)))
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_spgemm_csr: null array");

    cmi_spgemm *r = new (std::nothrow) cmi_spgemm;
    if (!r) return fail(CMI_ERROR_ALLOC, "cmi_spgemm_csr: out of host memory");
    struct guard { // the handle is the caller's only on success
        cmi_spgemm *r;
        ~guard() { delete r; }
    } own{r};
    r->dtype = sizeof(T) == 8 ? CMI_F64 : CMI_F32;
    r->m = m;
    if (m == 0 || a_entries == 0 || b_entries == 0 || k == 0) { // no products: an all-zero Cp, nothing on the device
        *result = r;
        own.r = nullptr;
        return CMI_SUCCESS;
    }

    hipStream_t s = as_stream(stream);
    // the scratch of this call: released on every path out
    device_array<int64_t> entry_block, row_block;
    device_array<uint64_t> keys_block, keys_sorted_block;
    device_array<uint32_t> perm_block, seg_block;
    device_array<T> vals_block;
    device_array<unsigned char> temp, sort_temp;
    hipError_t e = entry_block.alloc((size_t)a_entries + 1);
    if (e == hipSuccess) e = row_block.alloc((size_t)m + 1);
    if (e != hipSuccess) return hip_fail(e, "cmi_spgemm_csr: scratch");
    int64_t *const entry_start = entry_block.get(), *const row_start = row_block.get();
    hipLaunchKernelGGL(spgemm_entry_products_kernel, dim3(capped_grid(a_entries + 1)), dim3(256), 0, s, a_entries, k, b_entries, Aj, Bp, entry_start);
    CMI_LAUNCH_CHECK("spgemm entry products");
    e = with_temp(temp, [&](void *t, size_t &b) {
        return rocprim::exclusive_scan(t, b, entry_start, entry_start, (int64_t)0, (size_t)(a_entries + 1), rocprim::plus<int64_t>(), s);
    });
    if (e != hipSuccess) return hip_fail(e, "cmi_spgemm_csr: scan of the product counts");
    hipLaunchKernelGGL(spgemm_row_products_kernel, dim3(capped_grid(m + 1)), dim3(256), 0, s, m, a_entries, Ap, entry_start, row_start);
    CMI_LAUNCH_CHECK("spgemm row products");
    std::vector<int64_t> start;
    try {
        start.resize((size_t)m + 1);
    } catch (const std::bad_alloc &) {
        (void)hipStreamSynchronize(s);
        return fail(CMI_ERROR_ALLOC, "cmi_spgemm_csr: out of host memory");
    }
    e = hipMemcpyAsync(start.data(), row_start, (size_t)(m + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s);
        return hip_fail(e, "cmi_spgemm_csr: reading the product counts");
    }
    for (int64_t i = 0; i < m; i++)
        if (start[i + 1] < start[i]) return fail(CMI_ERROR_INVALID_VALUE, "cmi_spgemm_csr: the row offsets of A are not non-decreasing");
    const int64_t total = start[m] - start[0];
    r->products = total;

    e = r->Cp.alloc((size_t)m + 1);
    if (e != hipSuccess) return hip_fail(e, "cmi_spgemm_csr: row offsets of C");
    if (total == 0) {
        e = hipMemsetAsync(r->Cp.get(), 0, (size_t)(m + 1) * sizeof(int32_t), s);
        hipError_t e2 = hipStreamSynchronize(s);
        if (e == hipSuccess) e = e2;
        if (e != hipSuccess) return hip_fail(e, "cmi_spgemm_csr");
        *result = r;
        own.r = nullptr;
        return CMI_SUCCESS;
    }

    // W: the caller's, or the lesser of the product count, the cap and what a third of the free memory holds
    int64_t W = g_spgemm_workspace;
    if (W == 0) {
        size_t free_bytes = 0, total_bytes = 0;
        e = hipMemGetInfo(&free_bytes, &total_bytes);
        if (e != hipSuccess) return hip_fail(e, "cmi_spgemm_csr: hipMemGetInfo");
        W = (int64_t)(free_bytes / 3) / scratch_bytes_per_product(sizeof(T));
        if (W > kSpgemmWorkspaceCap) W = kSpgemmWorkspaceCap;
        if (W < 1) W = 1;
    }
    if (W > total) W = total;

    // slabs of consecutive rows with at most W products each
    std::vector<int64_t> cut(1, 0);
    int64_t largest = 0;
    for (int64_t r0 = 0; r0 < m;) {
        const int64_t r1 = (std::upper_bound(start.begin() + r0 + 1, start.end(), start[r0] + W) - start.begin()) - 1;
        if (r1 == r0) {
            set_error("cmi_spgemm_csr: row %lld expands to %lld products, more than the workspace of %lld products holds (cmi_spgemm_set_workspace)",
                      (long long)r0, (long long)(start[r0 + 1] - start[r0]), (long long)W);
            return CMI_ERROR_NOT_SUPPORTED;
        }
        largest = std::max(largest, start[r1] - start[r0]);
        cut.push_back(r1);
        r0 = r1;
    }

    size_t sort_bytes = 0, scan_bytes = 0;
    rocprim::counting_iterator<uint32_t> position(0);
    const size_t cap = (size_t)largest;
    e = keys_block.alloc(cap);
    if (e == hipSuccess) e = keys_sorted_block.alloc(cap);
    if (e == hipSuccess) e = perm_block.alloc(cap);
    if (e == hipSuccess) e = seg_block.alloc(cap);
    if (e == hipSuccess) e = vals_block.alloc(cap);
    uint64_t *const keys = keys_block.get(), *const keys_sorted = keys_sorted_block.get();
    uint32_t *const perm = perm_block.get(), *const seg = seg_block.get();
    T *const vals = vals_block.get();
    // the two rocPRIM calls of a slab, sized once for the largest slab and every key bit into ONE block (they run one after the other)
    size_t count = cap;
    unsigned end_bit = 64u;
    auto sort = [&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, (const uint64_t *)keys, keys_sorted, position, perm, (unsigned)count, 0u, end_bit, s); };
    auto number_heads = [&](void *t, size_t &b) { return rocprim::inclusive_scan(t, b, seg, seg, count, rocprim::plus<uint32_t>(), s); };
    if (e == hipSuccess) e = temp_size(sort, &sort_bytes);
    if (e == hipSuccess) e = temp_size(number_heads, &scan_bytes);
    if (e == hipSuccess) e = sort_temp.alloc(std::max(sort_bytes, scan_bytes));
    if (e != hipSuccess) return hip_fail(e, "cmi_spgemm_csr: slab scratch");
    uint32_t *starts = reinterpret_cast<uint32_t *>(keys); // (the unsorted keys are dead once the sort has run)

    const int col_bits = spgemm_bits_for(n);
    const uint32_t col_mask = (uint32_t)(((uint64_t)1 << col_bits) - 1);
    int64_t entries = 0;
    int st = CMI_SUCCESS;
    for (size_t b = 0; b + 1 < cut.size() && st == CMI_SUCCESS; b++) {
        const int64_t r0 = cut[b], r1 = cut[b + 1], P = start[r1] - start[r0];
        count = (size_t)P;
        end_bit = (unsigned)(col_bits + spgemm_bits_for(r1 - r0)); // (P >= 1: W >= 1 and a slab ends at the last row it can hold)
        size_t sb = sort_bytes, cb = scan_bytes;
        e = launch(spgemm_expand_kernel<T>, blocks_for(P), 256, 0, s, P, start[r0], (int)r0, (int)r1, a_entries, Ap, Aj, Ax, Bp, Bj, Bx, entry_start, col_bits, col_mask, keys, vals);
        if (e == hipSuccess) e = sort(sort_temp.get(), sb);
        if (e == hipSuccess) e = launch(spgemm_heads_kernel, blocks_for(P), 256, 0, s, P, keys_sorted, seg);
        if (e == hipSuccess) e = number_heads(sort_temp.get(), cb);
        uint32_t unique = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&unique, seg + (P - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { st = hip_fail(e, "cmi_spgemm_csr: sort and compress"); break; }
        const int64_t U = unique;
        if (entries + U > kSpgemmCeiling) {
            st = fail(CMI_ERROR_INVALID_VALUE, "cmi_spgemm_csr: C has more entries than the int32 index type holds");
            break;
        }
        cmi_spgemm::piece pc;
        pc.count = U;
        e = pc.Cj.alloc((size_t)U);
        if (e == hipSuccess) e = pc.Cx.alloc((size_t)U * sizeof(T));
        if (e != hipSuccess) { st = hip_fail(e, "cmi_spgemm_csr: entries of C"); break; }
        int32_t *const Cj = pc.Cj.get();
        T *const Cx = reinterpret_cast<T *>(pc.Cx.get());
        try {
            r->pieces.push_back(std::move(pc)); // (the handle's from here)
        } catch (const std::bad_alloc &) {
            st = fail(CMI_ERROR_ALLOC, "cmi_spgemm_csr: out of host memory");
            break;
        }
        e = launch(spgemm_starts_kernel, blocks_for(P), 256, 0, s, P, keys_sorted, seg, starts);
        if (e == hipSuccess) e = launch(spgemm_sum_kernel<T>, blocks_for(U), 256, 0, s, U, P, keys_sorted, perm, starts, vals, col_mask, Cj, Cx);
        if (e == hipSuccess) e = launch(spgemm_row_offsets_kernel, blocks_for(r1 - r0), 256, 0, s, r1 - r0, P, (int)r0, entries, col_bits, keys_sorted, seg, r->Cp.get());
        if (e != hipSuccess) { st = hip_fail(e, "launch spgemm compress"); break; }
        entries += U;
        r->slabs++;
    }
    if (st == CMI_SUCCESS) {
        e = hipMemsetD32Async((hipDeviceptr_t)(r->Cp.get() + m), (int)entries, 1, s);
        if (e != hipSuccess) st = hip_fail(e, "cmi_spgemm_csr: last row offset");
    }
    // the scratch is released when this returns: everything enqueued above must have finished with it
    e = hipStreamSynchronize(s);
    if (st == CMI_SUCCESS && e != hipSuccess) st = hip_fail(e, "cmi_spgemm_csr");
    if (st != CMI_SUCCESS) return st;
    r->num_entries = entries;
    r->rows_in_slabs = m;
    *result = r;
    own.r = nullptr;
    return CMI_SUCCESS;
}

template <typename T> static int spgemm_take(cmi_spgemm *r, int32_t *Cp, int32_t *Cj, T *Cx, int64_t capacity, void *stream)
{
    if (!r) return fail(CMI_ERROR_INVALID_VALUE, "cmi_spgemm_take: result is NULL");
    if (r->dtype != (sizeof(T) == 8 ? CMI_F64 : CMI_F32)) return fail(CMI_ERROR_INVALID_VALUE, "cmi_spgemm_take: the result holds the other value type");
    if (capacity < r->num_entries) {
        set_error("cmi_spgemm_take: capacity %lld is below the %lld entries of C", (long long)capacity, (long long)r->num_entries);
        return CMI_ERROR_INVALID_VALUE;
    }
    if (!Cp || (r->num_entries > 0 && (!Cj || !Cx))) return fail(CMI_ERROR_INVALID_VALUE, "cmi_spgemm_take: null array");
    hipStream_t s = as_stream(stream);
    if (r->Cp) CMI_HIP(hipMemcpyAsync(Cp, r->Cp.get(), (size_t)(r->m + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    else CMI_HIP(zero_store(Cp, r->m + 1, s)); // an empty product; a kernel, not a memset node: the call records into a capture (common.h)
    int64_t at = 0;
    for (const cmi_spgemm::piece &q : r->pieces) {
        if (q.count == 0) continue;
        CMI_HIP(hipMemcpyAsync(Cj + at, q.Cj.get(), (size_t)q.count * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        CMI_HIP(hipMemcpyAsync(Cx + at, q.Cx.get(), (size_t)q.count * sizeof(T), hipMemcpyDeviceToDevice, s));
        at += q.count;
    }
    return CMI_SUCCESS;
}

} // namespace cmi

CMI_API int cmi_spgemm_csr_f64(int64_t m, int64_t k, int64_t n, int64_t a_entries, const int32_t *Ap, const int32_t *Aj, const double *Ax,
                               int64_t b_entries, const int32_t *Bp, const int32_t *Bj, const double *Bx, cmi_spgemm **result, void *stream)
{ return cmi::spgemm_csr<double>(m, k, n, a_entries, Ap, Aj, Ax, b_entries, Bp, Bj, Bx, result, stream); }
CMI_API int cmi_spgemm_csr_f32(int64_t m, int64_t k, int64_t n, int64_t a_entries, const int32_t *Ap, const int32_t *Aj, const float *Ax,
                               int64_t b_entries, const int32_t *Bp, const int32_t *Bj, const float *Bx, cmi_spgemm **result, void *stream)
{ return cmi::spgemm_csr<float>(m, k, n, a_entries, Ap, Aj, Ax, b_entries, Bp, Bj, Bx, result, stream); }

CMI_API int cmi_spgemm_num_entries(const cmi_spgemm *r, int64_t *num_entries)
{
    if (!r || !num_entries) return cmi::fail(CMI_ERROR_INVALID_VALUE, "cmi_spgemm_num_entries: null argument");
    *num_entries = r->num_entries;
    return CMI_SUCCESS;
}

CMI_API int cmi_spgemm_take_f64(cmi_spgemm *r, int32_t *Cp, int32_t *Cj, double *Cx, int64_t capacity, void *stream)
{ return cmi::spgemm_take<double>(r, Cp, Cj, Cx, capacity, stream); }
CMI_API int cmi_spgemm_take_f32(cmi_spgemm *r, int32_t *Cp, int32_t *Cj, float *Cx, int64_t capacity, void *stream)
{ return cmi::spgemm_take<float>(r, Cp, Cj, Cx, capacity, stream); }

CMI_API int cmi_spgemm_info(const cmi_spgemm *r, int64_t *products, int64_t *slabs, int64_t *rows_in_tiles, int64_t *rows_in_slabs)
{
    if (!r) return cmi::fail(CMI_ERROR_INVALID_VALUE, "cmi_spgemm_info: result is NULL");
    if (products) *products = r->products;
    if (slabs) *slabs = r->slabs;
    if (rows_in_tiles) *rows_in_tiles = r->rows_in_tiles;
    if (rows_in_slabs) *rows_in_slabs = r->rows_in_slabs;
    return CMI_SUCCESS;
}

CMI_API int cmi_spgemm_destroy(cmi_spgemm *r)
{
    delete r;
    return CMI_SUCCESS;
}

CMI_API int cmi_spgemm_limits(int64_t *tile_products, int64_t *workspace_products)
{
    if (tile_products) *tile_products = 0; // no LDS tile path in this build
    if (workspace_products) *workspace_products = cmi::g_spgemm_workspace ? cmi::g_spgemm_workspace : cmi::kSpgemmWorkspaceCap;
    return CMI_SUCCESS;
}

CMI_API int cmi_spgemm_set_workspace(int64_t products)
{
    if (products < 0 || products > cmi::kSpgemmWorkspaceMax)
        return cmi::fail(CMI_ERROR_INVALID_VALUE, "cmi_spgemm_set_workspace: the workspace is 0 (default) or 1 .. INT32_MAX - 65536 products");
    cmi::g_spgemm_workspace = products;
    return CMI_SUCCESS;
}

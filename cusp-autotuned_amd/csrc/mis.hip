// mis.hip -- cusp::graph::maximal_independent_set and cusp::precond::aggregation::mis_aggregate on the device (DESIGN 3.10,
// 3.11): a chain of CSR row sweeps that take the maximum of a 64-bit key over the entries of a row -- a multiply without values.
//
// Replaces (reference): cusp/system/detail/generic/graph/maximal_independent_set.h (generalized_spmv on zipped
// (state, random, index) tuples, two for_each passes and a count per round) and
// cusp/precond/aggregation/system/detail/generic/mis_aggregate.h (two more generalized_spmv, a scan, a gather, a sort and a
// reduce_by_key for the singletons).  The tuple is ONE uint64 here -- state << 62 | random << 31 | index -- so that the
// lexicographic maximum is an integer maximum; the random values are cusp::detail::random_hash(i, seed) >> 33, not the
// reference's.
//
// Contract: the sequential loops as include/cusp_mi355x.h states them.  All integer work: a maximum is exact in any order, so
// the storage-order rule of the floating-point kernels does not bind here -- a lane keeps four gathers in flight and a long row
// is folded across the wave.  The graph is the stored pattern: every entry is an edge, columns may repeat, rows may be
// unsorted, a node always sees itself.  Row offsets are clamped to [0, num_entries] before they address anything, a decreasing
// pair is an empty row, a column outside [0, num_rows) contributes nothing and is never used as an address.
//
// Bytes of one sweep (the hot kernel; every sweep of both algorithms is this kernel):
//   reads  4 (num_rows + 1) row offsets + 4 num_entries columns + 8 num_rows own keys, gathers 8 num_entries keys
//   writes 8 num_rows keys
// The gathered keys are the array the own-key read streams once, so what must come from HBM is 4 num_entries + 20 num_rows
// bytes (poisson5pt: 40 bytes per row against 100 for the f64 multiply); the gathers are L2 / Infinity-Cache traffic as x is in
// the multiply.  The last sweep of a MIS round touches undecided rows only.
#include "amg_shared.h"

#include "../include/cusp/detail/random_hash.h"

namespace cmi {

typedef unsigned long long key_t; // uint64_t's device-side spelling (the shuffles are overloaded on it)
constexpr key_t kIndexMask = 0x7FFFFFFFull;
constexpr int kStateOut = 0, kStateUndecided = 1, kStateIn = 2;

__device__ __forceinline__ key_t key_max(key_t a, key_t b) { return a > b ? a : b; }
__device__ __forceinline__ key_t mis_key(int state, int64_t i, uint64_t seed)
{
    return ((key_t)state << 62) | ((key_t)(cusp::detail::random_hash((uint64_t)i, seed) >> 33) << 31) | (key_t)i;
}

// x[j] for a column inside the matrix, 0 (the identity of max over keys) and the flag otherwise
__device__ __forceinline__ key_t ring_gather(const key_t *__restrict__ x, int j, int64_t num_rows, bool &outside)
{
    const bool in = j >= 0 && (int64_t)j < num_rows;
    outside |= !in;
    return in ? x[j] : 0ull;
}

enum { kRingPlain = 0, kRingLastOfRound = 1, kRingBoost = 2 };
// z[i] = max(x[i], max over row i of x[Aj[jj]]).  One wave per 64 consecutive rows (block = 4 waves).  A row of at most 64
// entries is walked by its own lane, four gathers in flight; a longer row by the whole wave, 64 entries at a time, folded by
// a butterfly of six shuffles.
//   kRingLastOfRound: only undecided rows (state[i] == 1; after a first sweep x[i] no longer tells) are computed and written; a
//                     row whose maximum carries its own index joins the set (state[i] = 2: step 3 of the round).  A lane
//                     touches its own row's state only.
//   kRingBoost:       z[i] = the maximum + (state[i] == 2) << 31 (mis_aggregate's first sweep).
// *bad = 1 when a computed row holds a column outside the matrix (a plain store: every offender stores the same word).
template <int MODE>
__global__ void __launch_bounds__(kAmgBlock)
ring_max_kernel(int64_t num_rows, int64_t num_entries, const int *__restrict__ Ap, const int *__restrict__ Aj, const key_t *__restrict__ x, key_t *__restrict__ z,
                int *state, int *__restrict__ bad)
{
    const int64_t row = (int64_t)blockIdx.x * kAmgBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    bool active = row < num_rows;
    key_t best = 0;
    if (active) {
        best = x[row];
        if (MODE == kRingLastOfRound) active = state[row] == kStateUndecided;
    }
    int lo = 0, hi = 0;
    if (active) {
        lo = amg_clamp(Ap[row], num_entries);
        hi = amg_clamp(Ap[row + 1], num_entries);
        if (hi < lo) hi = lo;
    }
    bool outside = false;
    const bool is_long = hi - lo > kWave;
    if (!is_long) {
        int jj = lo;
        for (; jj + 4 <= hi; jj += 4) {
            const int j0 = Aj[jj], j1 = Aj[jj + 1], j2 = Aj[jj + 2], j3 = Aj[jj + 3];
            const key_t v0 = ring_gather(x, j0, num_rows, outside), v1 = ring_gather(x, j1, num_rows, outside);
            const key_t v2 = ring_gather(x, j2, num_rows, outside), v3 = ring_gather(x, j3, num_rows, outside);
            best = key_max(best, key_max(key_max(v0, v1), key_max(v2, v3)));
        }
        for (; jj < hi; jj++) best = key_max(best, ring_gather(x, Aj[jj], num_rows, outside));
    }
    unsigned long long todo = __ballot(is_long); // every lane of the wave is here: no lane has left
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int rlo = __shfl(lo, src), rhi = __shfl(hi, src);
        key_t m = 0;
        for (int base = rlo; base < rhi; base += kWave) {
            const int jj = base + lane; // (rhi <= INT32_MAX - 65536: no overflow)
            if (jj < rhi) m = key_max(m, ring_gather(x, Aj[jj], num_rows, outside));
        }
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) m = key_max(m, __shfl_xor(m, d));
        if (lane == src) best = key_max(best, m);
    }
    if (active) {
        if (MODE == kRingBoost) best += (key_t)(state[row] == kStateIn) << 31;
        z[row] = best;
        if (MODE == kRingLastOfRound && (int64_t)(best & kIndexMask) == row) state[row] = kStateIn;
    }
    if (outside && bad) *bad = 1;
}

static hipError_t ring_launch(int mode, int64_t num_rows, int64_t num_entries, const int *Ap, const int *Aj, const key_t *x, key_t *z, int *state, int *bad,
                              hipStream_t s)
{
    const dim3 grid(amg_blocks(num_rows)), block(kAmgBlock);
    const auto kernel = mode == kRingPlain ? ring_max_kernel<kRingPlain> : (mode == kRingLastOfRound ? ring_max_kernel<kRingLastOfRound> : ring_max_kernel<kRingBoost>);
    return launch(kernel, grid, block, 0, s, num_rows, num_entries, Ap, Aj, x, z, state, bad);
}

// ---- MIS(k): the round loop ---------------------------------------------------------------------------------------------------
// counters of one round, read by the host once: undecided nodes, a column out of range, nodes in the set
enum { kCountUndecided = 0, kCountBad = 1, kCountInSet = 2, kCounters = 3 };

__global__ void __launch_bounds__(kAmgBlock) mis_start_kernel(int64_t n, uint64_t seed, int *__restrict__ state, key_t *__restrict__ x)
{
    const int64_t i = (int64_t)blockIdx.x * kAmgBlock + threadIdx.x;
    if (i >= n) return;
    state[i] = kStateUndecided;
    x[i] = mis_key(kStateUndecided, i, seed);
}

// Step 4 of a round, the next round's keys and the counts, one launch.  An undecided node whose final key's index names a node
// that is in the set leaves.  state[idx] is read while other lanes store 0 over a 1: neither value is 2, and no lane stores a 2
// here, so the test does not depend on the order.  One integer atomic per wave and counter.
__global__ void __launch_bounds__(kAmgBlock)
mis_finish_kernel(int64_t n, uint64_t seed, const key_t *__restrict__ z, int *state, key_t *__restrict__ x, int *__restrict__ counters)
{
    const int64_t i = (int64_t)blockIdx.x * kAmgBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    int st = kStateOut;
    if (i < n) {
        st = state[i];
        if (st == kStateUndecided && state[z[i] & kIndexMask] == kStateIn) { // (an index field was written from a row number: < n)
            st = kStateOut;
            state[i] = kStateOut;
        }
        x[i] = mis_key(st, i, seed);
    }
    const int undecided = __popcll(__ballot(st == kStateUndecided)), in_set = __popcll(__ballot(st == kStateIn));
    if (lane == 0) {
        if (undecided) atomicAdd(&counters[kCountUndecided], undecided);
        if (in_set) atomicAdd(&counters[kCountInSet], in_set);
    }
}

// flag[i] = 1 / 0 for i < n (no states: every node is in the set); i == n (when count says so): 0, the slot in which the
// offsets scan leaves the total
__global__ void __launch_bounds__(kAmgBlock) mis_flags_kernel(int64_t n, int64_t count, const int *__restrict__ state, int *__restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * kAmgBlock + threadIdx.x;
    if (i < count) flag[i] = (i < n && (!state || state[i] == kStateIn)) ? 1 : 0;
}

static size_t mis_states_bytes(int64_t n, int k)
{
    return device_arena::padded((size_t)n * sizeof(int)) + device_arena::padded(kCounters * sizeof(int)) + (k >= 2 ? 3 : 2) * device_arena::padded((size_t)n * sizeof(key_t));
}

// The states of MIS(k), k >= 1, on n >= 1 nodes, left in *state_out (taken from `arena`, which holds mis_states_bytes(n, k) at
// least, as are the key arrays handed back for reuse).  INVALID_VALUE on a column out of range, NOT_SUPPORTED beyond n + 1
// rounds; the stream is idle on return.
static int mis_states(device_arena &arena, int64_t n, int64_t nnz, const int *Ap, const int *Aj, int k, uint64_t seed, int **state_out, key_t *keys_out[3],
                      int64_t *set_size, int *rounds_out, hipStream_t s)
{
    int *state = arena.take<int>((size_t)n), *counters = arena.take<int>(kCounters);
    key_t *keys[3] = {nullptr, nullptr, nullptr};
    for (int a = 0; a < (k >= 2 ? 3 : 2); a++) keys[a] = arena.take<key_t>((size_t)n);
    if (!state || !counters || !keys[0] || !keys[1] || (k >= 2 && !keys[2])) return fail(CMI_ERROR_ALLOC, "maximal independent set: scratch reservation too small");
    hipError_t e = launch(mis_start_kernel, amg_blocks(n), kAmgBlock, 0, s, n, seed, state, keys[0]);
    int rounds = 0, host[kCounters] = {0, 0, 0};
    while (e == hipSuccess) {
        e = hipMemsetAsync(counters, 0, kCounters * sizeof(int), s);
        const key_t *from = keys[0];
        key_t *to = keys[1];
        for (int ring = 1; ring <= k && e == hipSuccess; ring++) { // each sweep reads the one before it: keys[1], keys[2], keys[1], ...
            to = keys[1 + ((ring - 1) & 1)];
            e = ring_launch(ring == k ? kRingLastOfRound : kRingPlain, n, nnz, Ap, Aj, from, to, state, counters + kCountBad, s);
            from = to;
        }
        if (e == hipSuccess) e = launch(mis_finish_kernel, amg_blocks(n), kAmgBlock, 0, s, n, seed, to, state, keys[0], counters);
        if (e == hipSuccess) e = hipMemcpyAsync(host, counters, sizeof(host), hipMemcpyDeviceToHost, s);
        const hipError_t e2 = hipStreamSynchronize(s); // the one host read of the round
        if (e == hipSuccess) e = e2;
        if (e != hipSuccess) break;
        rounds++;
        if (host[kCountBad]) return fail(CMI_ERROR_INVALID_VALUE, "maximal independent set: a column index lies outside [0, num_rows)");
        if (host[kCountUndecided] == 0) break;
        if ((int64_t)rounds > n) return fail(CMI_ERROR_NOT_SUPPORTED, "maximal independent set: nodes still undecided after num_rows + 1 rounds");
    }
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s); // the scratch goes with the caller's allocation
        return hip_fail(e, "maximal independent set");
    }
    *state_out = state;
    if (keys_out)
        for (int a = 0; a < 3; a++) keys_out[a] = keys[a];
    *set_size = host[kCountInSet];
    *rounds_out = rounds;
    return CMI_SUCCESS;
}

static int mis_check_sizes(const char *who, int64_t num_rows, int64_t num_entries, const int *Ap, const int *Aj)
{
    if (num_rows < 0 || num_entries < 0) {
        set_error("%s: negative size", who);
        return CMI_ERROR_INVALID_VALUE;
    }
    if (num_rows > INT32_MAX - 1 || num_entries > kAmgCeiling) {
        set_error("%s: sizes exceed the int32 index type", who);
        return CMI_ERROR_INVALID_VALUE;
    }
    if ((num_rows > 0 && !Ap) || (num_entries > 0 && !Aj)) {
        set_error("%s: null array", who);
        return CMI_ERROR_INVALID_VALUE;
    }
    return CMI_SUCCESS;
}

static int maximal_independent_set(int64_t num_rows, int64_t num_entries, const int *Ap, const int *Aj, int k, uint64_t seed, int *stencil, int64_t *set_size,
                                   int *rounds, void *stream)
{
    const char *who = "cmi_csr_maximal_independent_set";
    const int st = mis_check_sizes(who, num_rows, num_entries, Ap, Aj);
    if (st != CMI_SUCCESS) return st;
    if (k < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_maximal_independent_set: k is negative");
    if (!set_size || !rounds || (num_rows > 0 && !stencil)) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_maximal_independent_set: null array");
    hipStream_t s = as_stream(stream);
    *set_size = 0;
    *rounds = 0;
    if (num_rows == 0) return CMI_SUCCESS;
    device_arena arena;
    int *state = nullptr;
    if (k > 0) {
        const hipError_t ea = arena.open(mis_states_bytes(num_rows, k));
        if (ea != hipSuccess) return hip_fail(ea, "cmi_csr_maximal_independent_set: scratch");
        const int r = mis_states(arena, num_rows, num_entries, Ap, Aj, k, seed, &state, nullptr, set_size, rounds, s);
        if (r != CMI_SUCCESS) {
            *set_size = 0;
            *rounds = 0;
            return r;
        }
    } else *set_size = num_rows; // every node, no sweep (state stays null)
    hipError_t e = launch(mis_flags_kernel, amg_blocks(num_rows), kAmgBlock, 0, s, num_rows, num_rows, state, stencil);
    const hipError_t e2 = hipStreamSynchronize(s); // the scratch is released when this returns
    if (e == hipSuccess) e = e2;
    return e == hipSuccess ? CMI_SUCCESS : hip_fail(e, who);
}

// ---- mis_aggregate ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kAmgBlock) aggregate_keys_kernel(int64_t n, const int *__restrict__ state, key_t *__restrict__ x)
{
    const int64_t i = (int64_t)blockIdx.x * kAmgBlock + threadIdx.x;
    if (i < n) x[i] = ((key_t)(state[i] == kStateIn) << 31) | (key_t)i;
}

// first[i] = the set node's number that node i's final key names, -1 when the key's top part is 0 (no set node within two
// steps); members[a] counts the nodes of a by integer atomics (exact in any order)
__global__ void __launch_bounds__(kAmgBlock)
aggregate_first_kernel(int64_t n, const key_t *__restrict__ z, const int *__restrict__ number, int *__restrict__ first, int *__restrict__ members)
{
    const int64_t i = (int64_t)blockIdx.x * kAmgBlock + threadIdx.x;
    if (i >= n) return;
    const key_t v = z[i];
    const int a = (v >> 31) == 0 ? -1 : number[v & kIndexMask];
    first[i] = a;
    if (a >= 0) atomicAdd(&members[a], 1);
}

__global__ void __launch_bounds__(kAmgBlock) aggregate_keep_kernel(int64_t n, const int *__restrict__ members, int *__restrict__ keep)
{
    const int64_t a = (int64_t)blockIdx.x * kAmgBlock + threadIdx.x;
    if (a <= n) keep[a] = (a < n && members[a] >= 2) ? 1 : 0;
}

__global__ void __launch_bounds__(kAmgBlock)
aggregate_final_kernel(int64_t n, const int *__restrict__ first, const int *__restrict__ keep, const int *__restrict__ renumbered, const int *__restrict__ flag,
                       int *__restrict__ aggregates, int *__restrict__ mis)
{
    const int64_t i = (int64_t)blockIdx.x * kAmgBlock + threadIdx.x;
    if (i >= n) return;
    const int a = first[i];
    aggregates[i] = (a >= 0 && keep[a]) ? renumbered[a] : -1;
    mis[i] = flag[i];
}

static int mis_aggregate(int64_t num_rows, int64_t num_entries, const int *Ap, const int *Aj, uint64_t seed, int *aggregates, int *mis, int64_t *num_aggregates,
                         void *stream)
{
    const char *who = "cmi_csr_mis_aggregate";
    const int st = mis_check_sizes(who, num_rows, num_entries, Ap, Aj);
    if (st != CMI_SUCCESS) return st;
    if (!num_aggregates || (num_rows > 0 && (!aggregates || !mis))) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_mis_aggregate: null array");
    *num_aggregates = 0;
    if (num_rows == 0) return CMI_SUCCESS;
    hipStream_t s = as_stream(stream);
    const int64_t n = num_rows;
    device_arena arena;
    size_t scan_bytes = 0; // of one exclusive scan of n + 1 ints (both scans have this shape)
    hipError_t e = temp_size(offsets_scan<int>(nullptr, nullptr, n, s), &scan_bytes);
    if (e == hipSuccess)
        e = arena.open(mis_states_bytes(n, 2) + 5 * device_arena::padded((size_t)(n + 1) * sizeof(int)) + device_arena::padded((size_t)n * sizeof(int)) +
                                device_arena::padded(scan_bytes));
    if (e != hipSuccess) return hip_fail(e, "cmi_csr_mis_aggregate: scratch");
    int *state = nullptr, rounds = 0;
    key_t *keys[3];
    int64_t set_size = 0;
    const int r = mis_states(arena, n, num_entries, Ap, Aj, 2, seed, &state, keys, &set_size, &rounds, s);
    if (r != CMI_SUCCESS) return r;
    int *flag = arena.take<int>((size_t)n + 1), *number = arena.take<int>((size_t)n + 1), *members = arena.take<int>((size_t)n + 1);
    int *keep = arena.take<int>((size_t)n + 1), *renumbered = arena.take<int>((size_t)n + 1), *first = arena.take<int>((size_t)n);
    void *scan_temp = arena.take<char>(scan_bytes ? scan_bytes : 1);
    if (!flag || !number || !members || !keep || !renumbered || !first || !scan_temp) return fail(CMI_ERROR_ALLOC, "cmi_csr_mis_aggregate: scratch reservation too small");
    // exclusive_offsets() in the arena's block, sized above
    auto offsets = [&](const int *in, int *out) { return offsets_scan(in, out, n, s)(scan_temp, scan_bytes); };
    const dim3 grid(amg_blocks(n)), grid1(amg_blocks(n + 1)), block(kAmgBlock);
    e = launch(aggregate_keys_kernel, grid, block, 0, s, n, state, keys[0]);
    if (e == hipSuccess) e = ring_launch(kRingBoost, n, num_entries, Ap, Aj, keys[0], keys[1], state, nullptr, s);
    if (e == hipSuccess) e = ring_launch(kRingPlain, n, num_entries, Ap, Aj, keys[1], keys[2], state, nullptr, s);
    if (e == hipSuccess) e = launch(mis_flags_kernel, grid1, block, 0, s, n, n + 1, state, flag);
    if (e == hipSuccess) e = offsets(flag, number);
    if (e == hipSuccess) e = hipMemsetAsync(members, 0, (size_t)(n + 1) * sizeof(int), s);
    if (e == hipSuccess) e = launch(aggregate_first_kernel, grid, block, 0, s, n, keys[2], number, first, members);
    if (e == hipSuccess) e = launch(aggregate_keep_kernel, grid1, block, 0, s, n, members, keep);
    if (e == hipSuccess) e = offsets(keep, renumbered);
    if (e == hipSuccess) e = launch(aggregate_final_kernel, grid, block, 0, s, n, first, keep, renumbered, flag, aggregates, mis);
    int count = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&count, renumbered + n, sizeof(int), hipMemcpyDeviceToHost, s);
    const hipError_t e2 = hipStreamSynchronize(s); // the scratch is released when this returns
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return hip_fail(e, who);
    *num_aggregates = count;
    return CMI_SUCCESS;
}

} // namespace cmi

CMI_API int cmi_csr_ring_max_u64(int64_t num_rows, int64_t num_entries, const int32_t *Ap, const int32_t *Aj, const uint64_t *x, uint64_t *z, void *stream)
{
    const int st = cmi::mis_check_sizes("cmi_csr_ring_max_u64", num_rows, num_entries, Ap, Aj);
    if (st != CMI_SUCCESS) return st;
    if (num_rows > 0 && (!x || !z)) return cmi::fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_ring_max_u64: null array");
    if (num_rows > 0 && x == z) return cmi::fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_ring_max_u64: z must not be x (other rows gather x)");
    if (num_rows == 0) return CMI_SUCCESS;
    const hipError_t e = cmi::ring_launch(cmi::kRingPlain, num_rows, num_entries, Ap, Aj, (const cmi::key_t *)x, (cmi::key_t *)z, nullptr, nullptr, cmi::as_stream(stream));
    return e == hipSuccess ? CMI_SUCCESS : cmi::hip_fail(e, "launch csr_ring_max");
}

CMI_API int cmi_csr_maximal_independent_set(int64_t num_rows, int64_t num_entries, const int32_t *Ap, const int32_t *Aj, int k, uint64_t seed, int32_t *stencil,
                                            int64_t *set_size, int *rounds, void *stream)
{ return cmi::maximal_independent_set(num_rows, num_entries, Ap, Aj, k, seed, stencil, set_size, rounds, stream); }

CMI_API int cmi_csr_mis_aggregate(int64_t num_rows, int64_t num_entries, const int32_t *Ap, const int32_t *Aj, uint64_t seed, int32_t *aggregates, int32_t *mis,
                                  int64_t *num_aggregates, void *stream)
{ return cmi::mis_aggregate(num_rows, num_entries, Ap, Aj, seed, aggregates, mis, num_aggregates, stream); }

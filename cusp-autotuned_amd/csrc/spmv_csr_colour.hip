// spmv_csr_colour.hip -- one colour of a multicolour Gauss-Seidel sweep: a CSR row sweep over an INDEXED subset of rows that
// skips the diagonal and writes x in place (reference sequential/relaxation/gauss_seidel.h gauss_seidel_indexed).
//
// For every slot s of [slot_begin, slot_end), i = ordering[s]:
//   rsum = T(0); over row i in storage order: an entry in column i sets diag (the last one wins) and adds nothing -- its
//   product is never formed --, any other entry does rsum = rsum + Ax * x[Aj] (multiply, then add: -ffp-contract=off);
//   if (diag != 0) x[i] = (b[i] - rsum) / diag, else x[i] keeps its bits.
// The sum is ONE ordered chain per row, so the bits are the host loop's.
//
// Shape: the rows of a colour are scattered over the matrix, each row's entries are contiguous.  A wave owns 64 consecutive
// slots (a wave-private tile: no LDS, no workgroup barrier).  A group of G lanes (a power of two, 1..64, chosen on the host
// from num_entries / num_rows) serves one row at a time, the wave's 64 / G groups serve 64 / G consecutive slots per step
// and the tile takes G steps.  A round fetches G consecutive entries of the row, one per lane, on consecutive addresses;
// every lane forms its one product (none for a diagonal hit or past the row's end); then every lane of the group receives
// the G products lane by lane (a lane shuffle each) and adds those that count, in entry order -- the group's lanes all hold
// the same chain, and its first lane stores.  A row longer than G takes more rounds.
//
// Two forms.  In place (scratch == NULL): the caller promises that no row of the range holds an off-diagonal column that
// is also in the range, so no lane reads an x another writes.  Parked (scratch != NULL): the first launch leaves slot s's
// value in scratch[s - slot_begin] and does not touch x -- the new value, or, where the row has no usable diagonal, the
// bits x[i] already has --; the second, stream-ordered behind it, stores scratch[s - slot_begin] to x[ordering[s]].  Every
// row then read the x from before the call, whatever the range holds.
#include "common.h"

namespace cmi {

constexpr int kGsBlock = 256;                 // 4 waves
constexpr int kGsSlots = kGsBlock;            // slots per workgroup: 64 per wave

template <typename T, int G, bool PARK>
__global__ void __launch_bounds__(kGsBlock)
gs_colour_kernel(const int *__restrict__ Ap, const int *__restrict__ Aj, const T *__restrict__ Ax, const T *__restrict__ b, T *x,
                 const int *__restrict__ ordering, int64_t slot_begin, int64_t slot_end, T *__restrict__ park)
{
    constexpr int kGroups = kWave / G;
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane & (G - 1), first = lane & ~(G - 1); // position in the group, the group's first lane
    const int64_t tile = slot_begin + ((int64_t)blockIdx.x * (kGsBlock / kWave) + threadIdx.x / kWave) * kWave;
    for (int step = 0; step < G; step++) {
        const int64_t s = tile + (int64_t)step * kGroups + lane / G;
        if (s >= slot_end) continue; // a whole group at a time: the shuffles below stay inside the group
        const int i = ordering[s];
        const int row_begin = Ap[i], row_end = Ap[i + 1];
        const T bi = b[i];
        T rsum = T(0), diag = T(0);
        for (int base = row_begin; base < row_end; base += G) { // (base + G stays inside int: the CSR ceiling)
            const int j = base + sub;
            const bool in = j < row_end;
            int c = i;
            T v = T(0);
            if (in) { c = Aj[j]; v = Ax[j]; }
            const bool hit = in && c == i, off = in && c != i;
            T p = T(0);
            if (off) p = v * x[c];
            if constexpr (G == 1) {
                if (off) rsum = rsum + p;
                if (hit) diag = v;
            } else {
                constexpr unsigned long long kMask = G == 64 ? ~0ull : (1ull << (G & 63)) - 1;
                const unsigned long long offs = (__ballot(off) >> first) & kMask, hits = (__ballot(hit) >> first) & kMask;
#pragma unroll
                for (int k = 0; k < G; k++) {
                    const T pk = __shfl(p, first + k);
                    if ((offs >> k) & 1) rsum = rsum + pk;
                }
                const int last = hits ? 63 - __clzll(hits) : 0; // the last diagonal entry of the round wins
                const T dv = __shfl(v, first + last);
                if (hits) diag = dv;
            }
        }
        if (sub != 0) continue;
        if constexpr (PARK) {
            park[s - slot_begin] = diag != T(0) ? (bi - rsum) / diag : x[i];
        } else {
            if (diag != T(0)) x[i] = (bi - rsum) / diag;
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(kGsBlock)
gs_scatter_kernel(const int *__restrict__ ordering, int64_t slot_begin, int64_t slot_end, const T *__restrict__ park, T *__restrict__ x)
{
    const int64_t s = slot_begin + (int64_t)blockIdx.x * kGsBlock + threadIdx.x;
    if (s < slot_end) x[ordering[s]] = park[s - slot_begin];
}

static bool gs_overlap(const void *p, int64_t np, const void *q, int64_t nq, size_t s)
{
    const uintptr_t pl = reinterpret_cast<uintptr_t>(p), ph = pl + (uintptr_t)np * s;
    const uintptr_t ql = reinterpret_cast<uintptr_t>(q), qh = ql + (uintptr_t)nq * s;
    return np > 0 && nq > 0 && pl < qh && ql < ph;
}

// lanes per row from the mean row length, as the reference's launcher picks its vector width (cuda/detail/relaxation/
// gauss_seidel.h: mean <= 2 -> 2, <= 4 -> 4, ... ), continued to 1 below and to 64 above
static int gs_group(int64_t rows, int64_t nnz)
{
    const int64_t mean = nnz / rows;
    int g = 1;
    while (g < 64 && mean > g) g *= 2;
    return g;
}

template <typename T>
static int csr_gauss_seidel_colour(int64_t rows, int64_t nnz, const int *Ap, const int *Aj, const T *Ax, const T *b, T *x, const int *ordering,
                                   int64_t slot_begin, int64_t slot_end, T *scratch, void *stream)
{
    const char *who = "cmi_csr_gauss_seidel_colour";
    if (rows < 0 || nnz < 0) { set_error("%s: negative size", who); return CMI_ERROR_INVALID_VALUE; }
    if (rows > INT32_MAX || nnz > INT32_MAX - 65536) { set_error("%s: sizes exceed the int32 index type", who); return CMI_ERROR_INVALID_VALUE; }
    if (slot_begin < 0 || slot_end < slot_begin || slot_end > rows) {
        set_error("%s: the slot range [%lld, %lld) is reversed or outside [0, num_rows]", who, (long long)slot_begin, (long long)slot_end);
        return CMI_ERROR_INVALID_VALUE;
    }
    const int64_t slots = slot_end - slot_begin;
    if (slots == 0) return CMI_SUCCESS;
    if (!Ap || !b || !x || !ordering || (nnz > 0 && (!Aj || !Ax))) { set_error("%s: null array", who); return CMI_ERROR_INVALID_VALUE; }
    if (gs_overlap(x, rows, b, rows, sizeof(T))) { set_error("%s: b overlaps x", who); return CMI_ERROR_INVALID_VALUE; }
    if (scratch && gs_overlap(x, rows, scratch, slots, sizeof(T))) { set_error("%s: scratch overlaps x", who); return CMI_ERROR_INVALID_VALUE; }

    const dim3 grid((unsigned)ceil_div(slots, kGsSlots)); // slots <= INT32_MAX
    const bool known = with_int<1, 2, 4, 8, 16, 32, 64>(gs_group(rows, nnz), [&](auto GV) {
        with_bool(scratch != nullptr, [&](auto PARK) {
            hipLaunchKernelGGL((gs_colour_kernel<T, decltype(GV)::value, decltype(PARK)::value>), grid, dim3(kGsBlock), 0, as_stream(stream), Ap, Aj,
                               Ax, b, x, ordering, slot_begin, slot_end, scratch);
        });
    });
    if (!known) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_gauss_seidel_colour: no kernel instance for the group size");
    CMI_LAUNCH_CHECK("gauss-seidel colour sweep");
    if (scratch) {
        hipLaunchKernelGGL((gs_scatter_kernel<T>), grid, dim3(kGsBlock), 0, as_stream(stream), ordering, slot_begin, slot_end, scratch, x);
        CMI_LAUNCH_CHECK("gauss-seidel colour scatter");
    }
    return CMI_SUCCESS;
}

} // namespace cmi

CMI_API int cmi_csr_gauss_seidel_colour_f64(int64_t num_rows, int64_t num_entries, const int32_t *Ap, const int32_t *Aj, const double *Ax,
                                            const double *b, double *x, const int32_t *ordering, int64_t slot_begin, int64_t slot_end,
                                            double *scratch, void *stream)
{
    return cmi::csr_gauss_seidel_colour<double>(num_rows, num_entries, Ap, Aj, Ax, b, x, ordering, slot_begin, slot_end, scratch, stream);
}
CMI_API int cmi_csr_gauss_seidel_colour_f32(int64_t num_rows, int64_t num_entries, const int32_t *Ap, const int32_t *Aj, const float *Ax,
                                            const float *b, float *x, const int32_t *ordering, int64_t slot_begin, int64_t slot_end,
                                            float *scratch, void *stream)
{
    return cmi::csr_gauss_seidel_colour<float>(num_rows, num_entries, Ap, Aj, Ax, b, x, ordering, slot_begin, slot_end, scratch, stream);
}

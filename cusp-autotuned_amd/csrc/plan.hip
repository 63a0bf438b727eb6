// plan.hip -- cmi_plan: what a multiply needs to know about ONE matrix beyond its arrays, found once.
//
// SURVEY.md section 8(b) asked for `cmi_plan_create/destroy/select` owning "autotune table lookup, optional
// preprocessing"; round 1 instead measured a CSR matrix's row lengths inside its first multiply (device allocation + copy +
// stream synchronise, cached by pointer).  Here the measurement happens at plan creation, explicitly, and the
// multiply entry points (cmi_spmv_*_plan_*) neither allocate nor wait.  The reference keeps comparable state in
// function-local statics of its KTT path (cusp/system/cuda/ktt/csr_multiply.h:22-29,239-247: `row_starts`,
// `row_counter`, recomputed on the host for every call) -- there is no object to port.
//
//   CSR : launch shape from the table (or the caller's config), completed; the row-length profile (longest row, entries
//         in rows of 512+) decides between the row-tile kernel, its long-row instance and the merge-path kernel.
//   COO : "are the entries sorted by row?" -- sorted input gets the row offsets its row indices imply and runs the CSR
//         kernels on them (12 instead of 16 bytes per entry); anything else the order-agnostic atomics kernels.  An explicit
//         CMI_COO_TILE config keeps the COO tile kernel.
//   ELL / DIA : the resolved launch shape only (nothing to measure).
//   HYB (cmi_plan_create_hyb) : is the COO part sorted by row?  Then one int per 256 rows -- where that tile's COO entries
//         begin -- lets ONE kernel finish a row (ELL slots, then its COO entries) instead of two launches over y.
#include "common.h"
#include <cstdlib>
#include <new>
#include <utility>

using namespace cmi;

// opt-in default for cmi_plan_create_csr with an AUTO kernel: try the 16-bit column copy ($CMI_COMPRESS_INDICES=1 at load,
// cmi_set_index_compression afterwards)
static int g_compress = -1;
static int compress_default()
{
    if (g_compress < 0) {
        const char *e = std::getenv("CMI_COMPRESS_INDICES");
        g_compress = (e && e[0] && e[0] != '0') ? 1 : 0;
    }
    return g_compress;
}
CMI_API int cmi_set_index_compression(int on) { g_compress = on ? 1 : 0; return CMI_SUCCESS; }
CMI_API int cmi_get_index_compression(void) { return compress_default(); }

static int plan_create(int format, int dtype, int64_t num_rows, int64_t num_cols, int64_t num_entries,
                       const int32_t *index_array, const int32_t *csr_columns, const cmi_config *cfg, void *stream, cmi_plan **plan_out, const void *csr_values = nullptr);

// ---- checksum of an index array (cmi_plan_validate) -------------------------------------------------------------------------
// sum over i of mix(i, a[i]) mod 2^64: position-dependent terms, combined by integer addition -- the same value whatever the
// launch shape or the order the workgroups finish in.  One pass over the array at streaming speed (10^7 row offsets: ~10 us).
namespace cmi {
__device__ __forceinline__ unsigned long long fp_mix(unsigned long long i, int v)
{
    unsigned long long h = ((unsigned long long)(unsigned int)v + 0x9E3779B97F4A7C15ull) * ((i << 1) | 1ull);
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    return h;
}
__global__ void __launch_bounds__(256) fingerprint_kernel(int64_t n, const int *__restrict__ a, unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long slots[256 / kWave];
    unsigned long long h = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) h += fp_mix((unsigned long long)i, a[i]);
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) h += __shfl_down(h, o);
    if ((threadIdx.x & (kWave - 1)) == 0) slots[threadIdx.x / kWave] = h;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 256 / kWave; w++) h += slots[w];
        atomicAdd(out, h);
    }
}
// *fp <- checksum of a[0, n); synchronises the stream (set-up / validation call)
static int fingerprint(int64_t n, const int *a, hipStream_t s, uint64_t *fp)
{
    *fp = 0;
    if (n <= 0 || !a) return CMI_SUCCESS;
    device_counters<unsigned long long> sum;
    hipError_t e = sum.open(s);
    if (e == hipSuccess) {
        int64_t blocks = ceil_div(n, 256 * 8);
        if (blocks > kCus * 8) blocks = kCus * 8;
        hipLaunchKernelGGL(fingerprint_kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks)), dim3(256), 0, s, n, a, sum.dev());
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = sum.fetch(s);
    if (e != hipSuccess) return hip_fail(e, "plan fingerprint");
    *fp = (uint64_t)sum.host[0];
    return CMI_SUCCESS;
}
// how many entries of the index array a plan of this format was made from
static int64_t index_length(const cmi_plan *p)
{
    switch (p->format) {
    case CMI_FORMAT_CSR: return p->rows > 0 ? p->rows + 1 : 0;
    case CMI_FORMAT_COO: return p->nnz;
    case CMI_FORMAT_HYB: return p->hyb_coo;
    default: return 0;
    }
}
} // namespace cmi

// Have the arrays this plan was made from changed?  Recomputes their checksum on the device (one streaming pass; synchronises
// `stream`) and compares it with the one taken at plan creation.  *valid_host = 1: same contents (up to a 2^-64 collision), 0: the
// structure was edited in place -- destroy the plan and make a new one.  column_indices: only compared when the plan owns data
// derived from them (CMI_CSR_STREAM_C16); may be NULL otherwise.  ELL / DIA plans hold nothing derived from the arrays: always valid.
CMI_API int cmi_plan_validate(const cmi_plan *plan, const int32_t *index_array, const int32_t *column_indices, void *stream, int *valid_host)
{
    if (!plan || !valid_host) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_validate: null plan or result");
    *valid_host = 1;
    hipStream_t s = as_stream(stream);
    if (plan->has_fp_index) {
        if (!index_array) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_validate: the plan was made from an index array; pass it");
        uint64_t fp = 0;
        if (int st = fingerprint(index_length(plan), index_array, s, &fp)) return st;
        if (fp != plan->fp_index) *valid_host = 0;
    }
    if (plan->has_fp_columns && *valid_host) {
        if (!column_indices) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_validate: the plan owns a copy of the column indices; pass them");
        uint64_t fp = 0;
        if (int st = fingerprint(plan->nnz, column_indices, s, &fp)) return st;
        if (fp != plan->fp_columns) *valid_host = 0;
    }
    return CMI_SUCCESS;
}

// csr_wave (CMI_CSR_STREAM_WAVE) instead of csr_stream: the longest row has 2..10 entries and the mean is within 7 % of it
// ($CMI_CSR_WAVE=0: never -- measurements of csr_stream on stencil matrices)
static int wave_env()
{
    static const int env = [] { const char *e = std::getenv("CMI_CSR_WAVE"); return e ? std::atoi(e) : 1; }();
    return env;
}
static bool wave_tiles_fit(int64_t rows, int64_t nnz, int64_t max_len)
{
    if (!wave_env() || rows <= 0 || max_len < 2 || max_len > kWaveTileMaxK) return false;
    return (double)nnz >= 0.93 * (double)max_len * (double)rows;
}
// Round 4 (the regret run, profiles/r04_auto_regret.txt, then the A/B of tools/stencil_tiles_probe.py, r04_stencil_tiles_ab.txt: one
// process, plans interleaved, five rounds that agree to 0.3 %): on f64 stencil rows of 5-7 entries csr_wavev with V = 1 -- wave tiles of
// 256 entries on a plan-built partition, the entry streams fetched as 16-byte vectors instead of csr_wave's lane-strided 4 + 8 bytes --
// takes 0.954 of csr_wave's time replayed (headline matrix 113.8 against 119.4 us = 0.878 against 0.837 of peak; 7-point 215^3 163.4
// against 171.2), 0.95-0.96 cold (125.9 against 130.9; 170.9 against 180.2) and 0.954 with the fused <y, w> of CG (123.1 against 129.0).
// Not so: 3 per row (replay 0.99, cold 1.05, fused dot 1.09), f32 (1.01), a cache-resident matrix (1000^2: 13.7 against 13.3 us), and
// rows of 9 (0.98 replayed, without the columns).  So: f64, the longest row 5..8, the streams beyond 1.25 x the Infinity Cache, and few
// enough tiles for the fused dot's partial list (one per 1024 entries) -- otherwise csr_wave as before.  $CMI_CSR_WAVE_VEC=0: never.
// f32 (sessions 22 / 24 / 25, three boxes): V = 1 gains nothing (0.99-1.01, fused dot 1.06), V = 2 -- tiles of 512 entries -- takes
// 0.971-0.981 of csr_wave's time replayed on the 5- and 7-point matrices, 0.96-1.00 cold, 0.98-1.00 with the fused dot: small, never a
// loss, taken.  Returns the index vectors per lane (0: csr_wave stays).
static int stencil_vector_tiles(int64_t nnz, const row_profile &prof, int dtype, size_t vbytes)
{
    static const int env = [] { const char *e = std::getenv("CMI_CSR_WAVE_VEC"); return e ? std::atoi(e) : 1; }();
    if (!env || prof.max_len < 5 || prof.max_len > 8 || prof.in_long > 0) return 0;
    if (nnz * (int64_t)(sizeof(int) + vbytes) <= kInfinityCacheBytes + kInfinityCacheBytes / 4) return 0;
    const int v = dtype == CMI_F64 ? 1 : 2;
    return nnz <= (int64_t)1024 * v * kPartialCapacity ? v : 0;
}
// Round 9: an AUTO plan of that rule made WITH the columns reads them from a plan-owned 16-bit copy (csr_wavev's C16 variant, spmv_csr.hip
// wavev_cols16_build; cfg.nontemporal bit 8) -- f64 only.  Measured on the headline matrix against the parent build, the driver's full line,
// one process per run, alternated (profiles/r09_cols16_ab.txt): counted traffic 810.5 -> 711.8 MB per launch, replayed 111.7 -> 103.2 us,
// cold 122.9 -> 112.0 us, each more than twice the session's parent-to-parent spread; in one process, explicit configs 3 against 11: 114.1 ->
// 101.5 us replayed, 119.3 -> 105.6 cold, 123.9 -> 115.4 with the fused dot.  The copy costs 2 bytes per entry of plan memory and two more
// passes over the columns at plan creation; a plan from the row offsets alone, or an explicit config without the bit, does without.
// A matrix with a tile that spans more than 65535 columns (the 7-point 215^3 stencil: +-46225 around the diagonal) is refused by the builder
// and runs the 32-bit kernel as before.  f32 (V = 2) was not measured and does not take the copy by itself; bit 8 asks for it explicitly.
static bool stencil_cols16(int dtype)
{
    return dtype == CMI_F64;
}
// ... and csr_wave on a plan-built partition (spmv_csr.hip wave_partition_build) for IRREGULAR short rows: K entries per lane with
// K = floor(mean + longest / 64), so that a wave tile of Q = 64 K - longest entries holds about Q / mean <= 64 rows; the longest row
// small enough for the tiles to fill 90 % of the wave's request slots.  OPT-IN: asked for per plan (cfg.kernel = CMI_CSR_STREAM_WAVE
// with rows_per_block < 0) -- measured against csr_stream it wins on FEM-like rows (thermal2-like 0.94 / 0.90 of its time, f64 / f32)
// and loses on large matrices with scattered columns (1.02-1.30x; archive/profiles/r02_wavep_ab.txt), so no plan selects it by itself
// ($CMI_CSR_WAVE=2: every AUTO plan whose rows qualify does -- measurements).
static int wave_partition_k(int64_t rows, int64_t nnz, const row_profile &prof, bool asked, int asked_k)
{
    if (!asked && (wave_env() < 2 || rows < 4096)) return 0;
    if (rows <= 0 || nnz <= 0 || prof.max_len < 1 || prof.in_long > 0) return 0;
    const double mean = (double)nnz / (double)rows;
    if (!asked && mean < 2.5) return 0;
    int k = asked_k > 0 ? asked_k : (int)std::floor(mean + (double)prof.max_len / 64.0);
    if (k < 2 && asked_k <= 0) k = 2;
    if (k < 2 || k > kWaveTileMaxK || (double)prof.max_len > 6.4 * k) return 0;
    return k;
}

// csr_wavev (CMI_CSR_STREAM_WAVEV): index vectors per lane V (a wave tile = 256 V slots), or 0 = not for this matrix.  Asked for (a plan
// made with that kernel): the caller's V or the rule's, refused when the longest row takes more than half of the tile.  AUTO plans:
// the rule below ($CMI_CSR_WAVEV=0: never; =1: whenever the rows qualify).
// AUTO plans take csr_wavev when ALL of (tools/wavev_ab.py, profiles/r03_wavev_ab.txt and r03_wavev_wavex_ab.txt: 24 matrices, f64 and f32,
// every variant bit-checked, interleaved rounds on one box):
//   * the index + value streams are beyond 0.75 x the Infinity Cache -- smaller matrices lose or tie (305 000 rows of 20: 1.13x; thermal2-like
//     at 104 MB even) because the partition's extra scalar hop is not hidden by anything there; at 240 MB (f32, 2..8 per row) it wins 0.79;
//   * fewer than 44 entries per row on average: 2-60 per row with columns anywhere in a +-2000..5000 band take 0.64-0.84 of csr_stream's
//     time (the wave keeps 16 gathers per lane in flight where csr_stream keeps 4-8: these matrices are gather-bound, 0.31-0.44 of peak),
//     27-point-like and nlpkkt120-like rows 0.95-0.97, columns scattered over the whole vector 0.98-1.00 (nothing helps those);
//     ldoor-like (45.6 per row) is 1.05x against the table's re-tuned csr_stream shape -- hence the bound;
//   * at least 4096 rows, no row of 512+ entries, the longest row at most half a wave tile (wavev_vectors below).
// Tile size: V = 4 (1024 request slots per wave) -- except f64 rows of fewer than 8 entries whose columns share x lines (see
// column_profile below: thermal2-like x6 110.0 us with V = 1 against 119.6), known only to plans made WITH the column indices.
// Stencil rows never get here (csr_wave is chosen first).  $CMI_CSR_WAVEV=0: never, =1: whenever the rows qualify.
static bool wavev_auto(int64_t rows, int64_t nnz, const row_profile &prof, int v, size_t vbytes)
{
    (void)prof;
    if (v != 4 || rows < 4096) return false;
    const double mean = (double)nnz / (double)rows;
    if (mean < 2.0 || mean >= 44.0) return false; // (2.0: until session 35 of round 4 2.5 -- rows of 1..4, mean 2.4999: 84.5 against 102.7 us, r04_auto_regret_set2_before.txt)
    return nnz * (int64_t)(sizeof(int) + vbytes) > kInfinityCacheBytes / 4 * 3;
}
// What a plan made with the column indices (cmi_plan_create_csr) adds: where the columns of a row lie.  `jumps` = share of entries 16+
// columns away from their predecessor in the row (each its own L1 lookup), `inside` = share within 1536 columns of the row's diagonal
// position (what an LDS x window around a workgroup's rows would serve).  Measured (r03_wavev_wavex_ab.txt):
//   jumps >= 0.6 and inside >= 0.25 (columns anywhere in a band): csr_wavex, the x window in LDS -- f32 0.71-0.92 of csr_wavev's time
//       (window 4096 from 15 entries per row, else 2048), f64 0.93-1.00 (window 2048); with jumps <= 0.31 (FEM blocks, stencils, sorted
//       meshes) the window only adds traffic: 1.3-1.8x SLOWER -- never selected there; inside = 0 (scattered): nothing helps.
//   f64, fewer than 8 entries per row, jumps < 0.5: V = 1.
//   inside < 0.05 with jumps >= 0.6 (scattered): csr_stream stays (wave tiles 0.97-1.06x: a wash).
//   f32 rows of 16+ entries with jumps < 0.5 -- or columns unknown -- : csr_stream stays (27-point-like / nlpkkt120-like f32: wave tiles 1.05-1.06x).
struct column_profile { double jumps = -1.0, inside = -1.0; int64_t jump_count = 0; bool measured = false; }; // < 0: not measured (jump_count: jumps as counted)
static int wavev_env()
{
    static const int env = [] { const char *e = std::getenv("CMI_CSR_WAVEV"); return e ? std::atoi(e) : -1; }();
    return env;
}
// Round 4: f64 rows of fewer than 8 entries whose columns share x lines take wave tiles with V = 1 BELOW the size gate
// too -- thermal2-like at 0.3 x / 1 x its size: 9.7 against 10.4 us, 20.8 against 21.8 (3 x: 63.6 against 70.6, already admitted),
// profiles/r04_size_gates_scale_sweep.txt, r04_thermal2_wave_tiles_v1.txt; V = 2 / 4 lose there.  From 200 000 rows; the column profile
// (jumps < 0.5) is checked by the caller, so only plans made WITH the columns qualify.
static bool short_f64_rows(int64_t rows, int64_t nnz, const row_profile &prof, int dtype, bool have_columns)
{
    if (!have_columns || dtype != CMI_F64 || rows < 200000 || nnz <= 0 || prof.max_len < 1 || prof.in_long > 0) return false;
    static const int env = [] { const char *e = std::getenv("CMI_CSR_WAVEV"); return e ? std::atoi(e) : -1; }();
    if (env == 0) return false;
    const double mean = (double)nnz / (double)rows;
    return mean >= 2.5 && mean < 8.0 && 2 * (prof.max_len + 3) <= 256;
}
// Round 4, session 35 (the regret table's sets 2 and 3, profiles/r04_auto_regret_set2_before.txt, r04_auto_regret_set3_size_gate.txt): on
// GATHER-BOUND band matrices (columns anywhere inside +-2000: every entry its own L1 lookup) the wave tiles win INSIDE the cache too --
// poisson(16) row lengths, 16 M entries: 47.0 against 53.5-56.3 us (f64), 29.0 against 33.7-40.5 (f32); 8 M: 26.5-28.1 against 29.0-30.6
// and 16.6-18.2 against 19.3-23.3; f32 at 4 M: 9.3-10.6 against 10.7-14.0; f64 at 4 M a tie -- where the size gate above (streams beyond
// 0.75 x the cache: made for rows whose columns share x lines, which lose or tie below it) keeps them out.  Such a matrix is admitted
// from 8 M entries (f64) / 4 M (f32) when its column profile says so (the caller measures it: plans made with the columns only); there
// the plain tiles do best, f64 with V = 2, f32 with V = 4 -- the x window pays only beyond the cache.
static bool band_candidate(int64_t rows, int64_t nnz, const row_profile &prof, int dtype, bool have_columns)
{
    if (!have_columns || rows < 4096 || nnz <= 0 || prof.max_len < 1 || prof.in_long > 0 || wavev_env() == 0) return false;
    const double mean = (double)nnz / (double)rows;
    const int v = dtype == CMI_F64 ? 2 : 4;
    return mean >= 2.0 && mean < 44.0 && nnz >= (dtype == CMI_F64 ? 8000000 : 4000000) && 2 * (prof.max_len + 3) <= 256 * v;
}
static int wavev_vectors(int64_t rows, int64_t nnz, const row_profile &prof, bool asked, int asked_v, size_t vbytes)
{
    if (rows <= 0 || nnz <= 0 || prof.max_len < 1 || prof.in_long > 0) return 0;
    const double mean = (double)nnz / (double)rows;
    int v = asked_v;
    if (v == 0) v = asked ? (mean >= 20.0 ? 4 : mean >= 8.0 ? 2 : 1) : 4; // (asked for: tile size by row length; AUTO plans: the measured V = 4)
    if (v != 1 && v != 2 && v != 4) return 0;
    while (v < 4 && !asked_v && 2 * (prof.max_len + 3) > 256 * v) v *= 2; // (the rule may widen the tile for a long row)
    if (2 * (prof.max_len + 3) > 256 * v) return 0;
    if (asked) return v;
    if (wavev_env() == 0) return 0;
    if (wavev_env() == 1) return rows >= 4096 ? v : 0;
    return wavev_auto(rows, nnz, prof, v, vbytes) ? v : 0;
}

// Adopts a wave-tile launch shape (declared in common.h: the plan-less stencil rule of spmv_csr.hip uses it too): 256 lanes, no lane groups,
// the kernel's own request shape and -- unless a caller's policy bits are kept as given -- the cache policy of streams read once.
// bytes_per_entry: what one entry adds to the streams this kernel reads (index + value, or the plan-owned copy that replaces the index).
void cmi::adopt_wave_shape(cmi_config *c, int64_t nnz, int kernel, int rows_per_block, int items_per_thread, int64_t bytes_per_entry, bool keep_policy)
{
    c->kernel = kernel;
    c->block_size = 256;
    c->rows_per_block = rows_per_block;
    c->items_per_thread = items_per_thread;
    c->threads_per_row = 0;
    c->nontemporal &= ~kPolStrided; // (the request shape is the kernel's own)
    if (keep_policy) return;
    // every line of its streams is requested exactly once: beyond the Infinity Cache the streaming hint is right whatever
    // the table's csr_stream entry of this bucket says (its 16-byte-vector shapes measured the other way) -- the top twelve of
    // 96 swept shapes on the headline matrix all carry it, a tridiagonal matrix of 10^7 rows 91.8 -> 83 us
    // (archive/profiles/r02_wave_shape_sweep.txt, r02_wave_ab.txt); below it, plain loads keep the matrix resident (tuning.hip)
    if (nnz * bytes_per_entry > kInfinityCacheBytes + kInfinityCacheBytes / 4) c->nontemporal |= kPolLoadNT;
    c->nontemporal |= kPolStoreNT;
}

// csr_waver (CMI_CSR_STREAM_WAVER): wave tiles on the run-compressed column copy.  Asked for: built whenever the tile can hold the longest
// row.  AUTO plans made with the columns ($CMI_CSR_WAVER=0: never, =1: whenever the rows qualify): at least 4096 rows of 8+ entries on
// average, no row of 512+, and the tuning table's "waver_rule" (tools/autotune_waver.py; tuning.hip has the built-in copy): at least
// min_entries entries (below: the partition's scalar hop is not hidden) and pieces of min_piece+ entries on average -- measured by
// building the copy, which is dropped again when they are shorter.  The rule also holds the launch shape (slots per lane, cap, XCD dealing).
static int waver_env()
{
    static const int env = [] { const char *e = std::getenv("CMI_CSR_WAVER"); return e ? std::atoi(e) : -1; }();
    return env;
}
static bool waver_try(cmi_plan *p, const int *Ap, const int *Aj, bool asked, int asked_v, int asked_cap, bool keep_policy, const void *values, hipStream_t s, int *st)
{
    const int64_t rows = p->rows, nnz = p->nnz;
    if (rows <= 0 || nnz <= 0 || p->prof.max_len < 1 || p->prof.in_long > 0 || p->cols < (p->dtype == CMI_F64 ? 2 : 4) || p->cols >= ((int64_t)1 << 30)) return false;
    // (f32, session 10 of round 4: ldoor-like 49.8 us against csr_stream's 70.9, nlpkkt120-like 101.3 against 156.8 -- the index stream is half of
    //  an f32 matrix's bytes, so compressing it pays more than for f64; same rule, profiles/r04_waver_f32_time.txt)
    cmi_waver_rule rule; // the persisted shape / gates (tuning table "waver_rule": tools/autotune_waver.py), else the built-in ones
    waver_rule(p->dtype, &rule);
    int v = asked_v ? asked_v : rule.items_per_thread;
    // (f64 rows of fewer than 12 entries: tiles of 512 slots, as for the plain wave tiles -- 5-point x 2 dof, 10 per row: 190.6 against
    //  211.3 us with V = 4; 9-point 143.7 against 144.4; in f32 V = 4 is ahead there, 125.1 against 133.1: r04_auto_regret_set4_before.txt)
    if (!asked && !asked_v && p->dtype == CMI_F64 && p->rows > 0 && (double)p->nnz < 12.0 * (double)p->rows && v == 4) v = 2; // (AUTO plans: an asked-for plan keeps the table's V)
    if (v != 1 && v != 2 && v != 4) return false;
    while (v < 4 && !asked_v && 2 * (p->prof.max_len + 3) > 256 * v) v *= 2;
    if (2 * (p->prof.max_len + 3) > 256 * v) return false;
    if (!asked) {
        if (waver_env() == 0) return false;
        const double mean = (double)nnz / (double)rows;
        if (rows < 4096) return false;
        // (size gate, profiles/r04_size_gates_scale_sweep.txt: at 10.8-10.9 M entries -- 130 MB of streams -- it takes 0.85-0.95 of the table
        //  kernel's time, at 5 M entries 1.13-1.22: smaller matrices keep csr_stream)
        //  f32 (r04_waver_f32_time.txt, f32 scale sweep): still 0.92 of the table kernel's time at 5.2 M entries -- gate at 5 M
        if (waver_env() != 1 && (mean < 8.0 || nnz < rule.min_entries)) return false;
    }
    double mean_piece = 0.0;
    *st = csr_runs_build(p, Ap, Aj, v, asked ? 0.0 : rule.min_piece, values, s, &mean_piece, asked && asked_cap ? asked_cap : rule.cap);
    if (*st != CMI_SUCCESS || !p->runs_start) return false;
    // (the residency rule counts the 12 / 8 bytes per entry of the caller's streams; a caller's policy bits are kept as given)
    adopt_wave_shape(&p->cfg, nnz, values ? CMI_CSR_STREAM_PACKED : CMI_CSR_STREAM_WAVER, 0, v, p->dtype == CMI_F64 ? 12 : 8, keep_policy);
    p->cfg.xcd_swizzle = rule.xcd_swizzle; // (16: chunks of 16 workgroups = 64 wave tiles per XCD: 0.99 of launch order's time on both configs[3] matrices, twice, profiles/r04_waver_xcd_dealing.txt)
    return true;
}

// CMI_CSR_STREAM_PACKED on stencil-like rows: the wave-tiled 16-bit copy, then everything a wave needs packed into one span per tile
static bool packed16_try(cmi_plan *p, const int *Ap, const int *Aj, const void *values, bool keep_policy, hipStream_t s, int *st)
{
    const cmi_config before = p->cfg;
    *st = csr16_build(p, Ap, Aj, s, (int)p->prof.max_len); // granted only if every tile of 64 rows spans fewer than 65536 columns
    if (*st == CMI_SUCCESS && p->cfg.kernel == CMI_CSR_STREAM_C16 && p->csr16_wave_k > 0) *st = csr16_pack(p, Ap, values, s);
    if (*st != CMI_SUCCESS || !p->csr16_packed) { if (*st == CMI_SUCCESS) p->cfg = before; return false; }
    // (the shape csr16_build / csr16_pack gave the tiles: 64 rows per wave, the longest row per lane; 2 bytes of column + the value per entry)
    adopt_wave_shape(&p->cfg, p->nnz, CMI_CSR_STREAM_PACKED, kWave, p->csr16_wave_k, 2 + (p->dtype == CMI_F64 ? 8 : 4), keep_policy);
    return true;
}

CMI_API int cmi_plan_create(int format, int dtype, int64_t num_rows, int64_t num_cols, int64_t num_entries,
                            const int32_t *index_array, const cmi_config *cfg, void *stream, cmi_plan **plan_out)
{
    if (format == CMI_FORMAT_CSR && cfg && cfg->kernel == CMI_CSR_STREAM_C16)
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_create: CMI_CSR_STREAM_C16 needs the column indices -- use cmi_plan_create_csr");
    return plan_create(format, dtype, num_rows, num_cols, num_entries, index_array, nullptr, cfg, stream, plan_out);
}

// CSR with both structure arrays: what cmi_plan_create(CMI_FORMAT_CSR, ...) does, plus -- asked for by
// cfg->kernel == CMI_CSR_STREAM_C16, or by the process-wide default with an AUTO kernel -- the 16-bit column copy.
CMI_API int cmi_plan_create_csr(int dtype, int64_t num_rows, int64_t num_cols, int64_t num_entries, const int32_t *row_offsets,
                                const int32_t *column_indices, const cmi_config *cfg, void *stream, cmi_plan **plan_out)
{
    if (num_entries > 0 && !column_indices) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_create_csr: null column indices");
    if (cfg && cfg->kernel == CMI_CSR_STREAM_PACKED) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_create_csr: CMI_CSR_STREAM_PACKED copies the values -- use cmi_plan_create_csr_values");
    return plan_create(CMI_FORMAT_CSR, dtype, num_rows, num_cols, num_entries, row_offsets, column_indices, cfg, stream, plan_out);
}

// COO with both index arrays: cmi_plan_create(CMI_FORMAT_COO, ...) plus, for ROW-SORTED entries, a CSR sub-plan made WITH the columns -- an FEM /
// KKT matrix held in COO then multiplies from the run-compressed column copy too (the reference's benchmark converts one matrix into every
// format, performance/spmv/spmv.cu:41-66: its COO line of such a matrix is this path).
CMI_API int cmi_plan_create_coo(int dtype, int64_t num_rows, int64_t num_cols, int64_t num_entries, const int32_t *row_indices,
                                const int32_t *column_indices, const cmi_config *cfg, void *stream, cmi_plan **plan_out)
{
    if (num_entries > 0 && !column_indices) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_create_coo: null column indices");
    return plan_create(CMI_FORMAT_COO, dtype, num_rows, num_cols, num_entries, row_indices, column_indices, cfg, stream, plan_out);
}

// CSR with the structure arrays AND the values: cmi_plan_create_csr plus -- asked for by cfg->kernel == CMI_CSR_STREAM_PACKED -- the packed
// per-tile copy of pieces and values (spmv_csr_runs.hip).  The values of any other plan stay the caller's.  With non-NULL values, a plan that
// ends up with csr_wavev's shift table (an AUTO or NULL config on the stencil route, or CMI_CSR_STREAM_WAVEV asked for with nontemporal bit 8)
// also gets the CONSTANT tiles' marks (spmv_csr.hip wavev_const_build): marks only, the multiply reads the values live.  Every other explicit
// config ignores the values as before.
CMI_API int cmi_plan_create_csr_values(int dtype, int64_t num_rows, int64_t num_cols, int64_t num_entries, const int32_t *row_offsets,
                                       const int32_t *column_indices, const void *values, const cmi_config *cfg, void *stream, cmi_plan **plan_out)
{
    if (num_entries > 0 && !column_indices) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_create_csr_values: null column indices");
    const bool packed = cfg && cfg->kernel == CMI_CSR_STREAM_PACKED;
    if (packed && num_entries > 0 && !values) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_create_csr_values: CMI_CSR_STREAM_PACKED needs the values");
    int st = plan_create(CMI_FORMAT_CSR, dtype, num_rows, num_cols, num_entries, row_offsets, column_indices, cfg, stream, plan_out, packed ? values : nullptr);
    // (the shift table exists on two routes only: the AUTO stencil route, and CMI_CSR_STREAM_WAVEV asked for with nontemporal bit 8)
    if (st == CMI_SUCCESS && values && (*plan_out)->cfg.kernel == CMI_CSR_STREAM_WAVEV && (*plan_out)->wavev_shift) {
        st = wavev_const_build(*plan_out, values, as_stream(stream));
        if (st != CMI_SUCCESS) { (void)cmi_plan_destroy(*plan_out); *plan_out = nullptr; }
    }
    return st;
}

CMI_API int cmi_plan_validate_values(const cmi_plan *plan, const void *values, void *stream, int *valid_host)
{
    if (!plan || !valid_host) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_validate_values: null plan or result");
    *valid_host = 1;
    if (plan->wavev_const) return wavev_const_check(plan, values, as_stream(stream), valid_host); // (never on a PACKED plan: marks come with an AUTO config only)
    if (!plan->has_fp_values) return CMI_SUCCESS;
    if (!values) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_validate_values: the plan owns a copy of the values; pass them");
    uint64_t fp = 0;
    if (int st = fingerprint(plan->nnz * (plan->dtype == CMI_F64 ? 2 : 1), reinterpret_cast<const int *>(values), as_stream(stream), &fp)) return st;
    if (fp != plan->fp_values) *valid_host = 0;
    return CMI_SUCCESS;
}

CMI_API int cmi_plan_device_bytes(const cmi_plan *plan, int64_t *bytes)
{
    if (!plan || !bytes) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_device_bytes: null argument");
    int64_t b = (int64_t)(plan->hyb_tile_start.bytes() + plan->coo_offsets.bytes() + plan->wave_row_start.bytes() + plan->wavev_base.bytes() +
                          plan->wavev_cols16.bytes() + plan->wavev_shift.bytes() + plan->wavev_const.bytes() + plan->csr16_base.bytes() + plan->csr16_cols.bytes() +
                          plan->runs_start.bytes() + plan->runs_pieces.bytes() + plan->runs_packed.bytes() + plan->csr16_packed.bytes());
    int64_t sub = 0;
    if (plan->hyb_coo_plan && cmi_plan_device_bytes(plan->hyb_coo_plan, &sub) == CMI_SUCCESS) b += sub;
    if (plan->coo_csr_plan && cmi_plan_device_bytes(plan->coo_csr_plan, &sub) == CMI_SUCCESS) b += sub;
    *bytes = b;
    return CMI_SUCCESS;
}

// the config is the table's csr_stream entry (or a caller's AUTO-kernel shape of it) with one lane per row: what the plan-built kernels replace
static bool table_stream(const cmi_config &c) { return c.kernel == CMI_CSR_STREAM && c.threads_per_row <= 1; }

// a plan with its header filled in and nothing measured yet (null: out of host memory)
static cmi_plan *plan_new(int format, int dtype, int64_t rows, int64_t cols, int64_t nnz)
{
    cmi_plan *p = new (std::nothrow) cmi_plan;
    if (!p) return nullptr;
    p->format = format;
    p->dtype = dtype;
    p->rows = rows;
    p->cols = cols;
    p->nnz = nnz;
    p->coo_sorted = -1; // (prof: "not measured" by its own initialisers)
    return p;
}

// What the caller asked a CSR plan for by naming a plan-only kernel: the kernel, its own use of the launch-shape fields, and the rest of
// the caller's config stripped to a table look-up (`lookup`: cache policy and XCD dealing if set, everything else the table's).
struct csr_ask {
    int kernel = CMI_KERNEL_AUTO; // CMI_CSR_STREAM_WAVE (rows_per_block < 0), _WAVEV, _WAVEX, _WAVER, _PACKED; AUTO: none of them
    int v = 0;           // WAVE: entries per lane; the others: index vectors per lane (0 = the rule's)
    int cap = 0;         // WAVER / PACKED: entries per piece at most (0 = the rule, 3 or 4)
    int window = 0;      // WAVEX: length of the x window (0 = the default)
    bool cols16 = false; // WAVEV with nontemporal bit 8 and the columns at hand: the plan-owned 16-bit column copy
    cmi_config lookup = {}; // ... whose nontemporal is the caller's cache policy (kept as given when any bit is set) and whose xcd_swizzle the
                         // caller's XCD dealing (kept as given when not 0; < 0: launch order)
    bool partition() const { return kernel == CMI_CSR_STREAM_WAVE; }
    bool wavev() const { return kernel == CMI_CSR_STREAM_WAVEV || kernel == CMI_CSR_STREAM_WAVEX; }
    bool waver() const { return kernel == CMI_CSR_STREAM_WAVER || kernel == CMI_CSR_STREAM_PACKED; }
    bool packed() const { return kernel == CMI_CSR_STREAM_PACKED; }
};
// the caller's config stripped to a table look-up: select_config takes the block size (none here) and the policy bits from an AUTO-kernel config
static cmi_config table_lookup_of(const cmi_config &cfg)
{
    cmi_config c = cfg;
    c.kernel = CMI_KERNEL_AUTO;
    c.block_size = c.threads_per_row = c.rows_per_block = c.items_per_thread = 0;
    return c;
}
// fills `a` from a config that names a plan-only kernel and returns the config to look the table up with (cfg itself otherwise):
//   CMI_CSR_STREAM_WAVE with rows_per_block < 0: wave tiles on a partition the plan builds (irregular short rows); launch policy from
//       the table, entries per lane from the caller (items_per_thread) or the rule
//   CMI_CSR_STREAM_WAVEV: wave-private tiles with the 16-byte-vector body on a partition the plan builds (rows of ~16-250 entries);
//       cache policy / XCD dealing from the caller's fields if set, else the table's; index vectors per lane from the caller or the rule.
//       nontemporal bit 8 (kPolCols16) asks for the plan-owned 16-bit column copy (spmv_csr.hip wavev_cols16_build); it needs the columns
//       (cmi_plan_create_csr).  The bit is not a cache policy: it is taken off here and put back into the plan's config only when the
//       copy was granted.
//   CMI_CSR_STREAM_WAVEX: the same partition; the multiply adds an x window in LDS (rows_per_block = its length)
//   CMI_CSR_STREAM_WAVER / _PACKED: wave tiles on the run-compressed column copy (spmv_csr_runs.hip); policy / dealing as for WAVEV
static const cmi_config *csr_ask_from(const cmi_config *cfg, bool have_columns, csr_ask *a)
{
    csr_ask named;
    named.kernel = cfg ? cfg->kernel : CMI_KERNEL_AUTO;
    if (!(named.partition() && cfg->rows_per_block < 0) && !named.wavev() && !named.waver()) return cfg;
    a->kernel = cfg->kernel;
    a->v = cfg->items_per_thread;
    if (a->kernel == CMI_CSR_STREAM_WAVEX) {
        a->window = cfg->rows_per_block > 0 ? cfg->rows_per_block : 0;
        if (a->v == 0) a->v = 4;
        if (a->v == 1) a->v = 2;
    }
    if (a->waver()) a->cap = cfg->threads_per_row; // (this kernel's use of the field: entries per piece at most, 0 = the rule, 3 or 4)
    a->cols16 = a->kernel == CMI_CSR_STREAM_WAVEV && (cfg->nontemporal & kPolCols16) && have_columns;
    a->lookup = table_lookup_of(*cfg);
    if (a->wavev()) a->lookup.nontemporal &= ~kPolCols16;
    return &a->lookup;
}

// the column profile of a plan made with the columns, measured when the first rule asks for it and at most once per plan (a full device
// pass over the columns)
static int column_profile_of(const cmi_plan *p, const int *Ap, const int *Aj, hipStream_t s, column_profile *cp)
{
    if (cp->measured || !Aj) return CMI_SUCCESS;
    int64_t inside = 0;
    if (int st = measure_column_locality(p->rows, p->cols, Ap, Aj, 1536, s, &inside, &cp->jump_count)) return st;
    cp->inside = (double)inside / (double)p->nnz;
    cp->jumps = (double)cp->jump_count / (double)p->nnz;
    cp->measured = true;
    return CMI_SUCCESS;
}

// stencil rows of 5..8 entries beyond the Infinity Cache: wave tiles of 256 (f64) / 512 (f32) entries on a plan-built partition
// (8 bytes per tile), entries fetched as 16-byte vectors (csr_wavev, V = 1 / 2) -- see stencil_vector_tiles above
static int route_stencil_vector_tiles(cmi_plan *p, const int *Ap, const int *Aj, int sv, hipStream_t s)
{
    int st = wave_partition_build(p, Ap, sv, s, 256 * sv - (int)p->prof.max_len - 3);
    if (st != CMI_SUCCESS || !p->wave_row_start) return st;
    // (beyond the cache by the rule: every line of the streams is requested once -- stencil_vector_tiles' gate is the helper's residency
    //  bound, so nt loads and nt stores are set whatever the table's entry says)
    adopt_wave_shape(&p->cfg, p->nnz, CMI_CSR_STREAM_WAVEV, 0, sv, sizeof(int) + (p->dtype == CMI_F64 ? 8 : 4), false);
    // ... and a plan made with the columns reads them from its own 16-bit copy (2 of the 12 / 8 bytes per entry leave the stream; see
    // stencil_cols16 above for what was measured).  Only this branch: the other AUTO routes into csr_wavev below keep the 32-bit
    // columns until a regret run over their matrices says otherwise.
    if (Aj && stencil_cols16(p->dtype)) st = wavev_cols16_build(p, Aj, s);
    return st;
}

// what an AUTO plan's csr_wavev route runs: index vectors per lane, with the x window (and its length) or without, or csr_stream after all
struct wavev_choice { int v; bool wavex = false, keep_stream = false; int window = 0; };
// an AUTO plan: refine by the value type and -- made with the columns -- by where the columns lie
static void wavev_refine(const cmi_plan *p, const column_profile &cp, bool small_only, bool short_rule, bool band_rule, wavev_choice *c)
{
    const double mean = (double)p->nnz / (double)p->rows;
    const char *wx = std::getenv("CMI_CSR_WAVEX");
    if (small_only) {
        if (band_rule && cp.jumps >= 0.6 && cp.inside >= 0.25) c->v = p->dtype == CMI_F64 ? 2 : 4; // (plain tiles: no window inside the cache)
        else if (!(short_rule && cp.jumps >= 0.0 && cp.jumps < 0.5)) c->keep_stream = true;
    } else if (cp.jumps >= 0.6 && cp.inside >= 0.25 && !(wx && wx[0] == '0')) {
        c->wavex = true;
        c->window = (p->dtype == CMI_F32 && mean >= 15.0) ? 4096 : 2048;
    } else if (cp.inside >= 0.0 && cp.inside < 0.05 && cp.jumps >= 0.6) {
        c->keep_stream = true; // columns scattered over the whole vector: 0.08-0.11 of peak whatever runs; wave tiles 0.97-1.06x
    } else if (p->dtype == CMI_F32 && mean >= 16.0 && cp.jumps < 0.5) {
        c->keep_stream = true; // f32 stencil / FEM-block rows of 16+ entries (or unknown columns): the table's csr_stream is 5-6 % faster
    } else if (mean < 12.0 && cp.jumps >= 0.0 && cp.jumps < (p->dtype == CMI_F64 ? 0.6 : 0.5)) {
        // (f64 up to 0.6 since session 38: a 7-point stencil with 12 % of its entries removed -- rows of 1..7, 57 % jumps -- 118.3 us
        //  with V = 1 against 127.0 with V = 4; in f32 V = 4 stays ahead there, 88.5 against 90.2 / 92.5)
        // short rows whose columns share x lines: smaller tiles.  f64 rows of fewer than 8 entries, none longer than 16: V = 1
        // (thermal2-like 20.4 / 63.4 us against 21.5 / 67.3 with V = 2); otherwise V = 2 -- against V = 4 (what every AUTO plan
        // ran until the regret run of round 4, profiles/r04_auto_regret.txt): uniform 1..16 per row 74.9 against 78.3 us (f64) and
        // 54.2 against 55.5 (f32), 4 / 40 per row 71.5 against 77.5 (V = 1: 78.6) and 44.9 against 46.3, thermal2-like x3 in f32
        // 38.5 against 40.0.  Columns anywhere in a band (jumps >= 0.6) without the x window keep V = 4 (217.5 against 234.0).
        // Either way only while the longest row still takes at most half of the smaller tile: with Q = 256 v - longest - 3
        // entries per tile a few rows of 126-252 entries would leave Q = 127..1, i.e. up to one wave tile (8 bytes of plan
        // memory, one wave) per handful of entries.  Widen back until the bound wavev_vectors() checked holds.
        c->v = (p->dtype == CMI_F64 && mean < 8.0 && p->prof.max_len <= 16) ? 1 : 2;
        while (c->v < 4 && 2 * (p->prof.max_len + 3) > 256 * c->v) c->v *= 2;
    }
}
// csr_wavev / csr_wavex on a plan-built partition, asked for or by the AUTO rules (wavev_vectors, short_f64_rows, band_candidate);
// `v` = wavev_vectors' answer, `cols_known` = an AUTO plan made with the columns
static int route_wavev(cmi_plan *p, const int *Ap, const int *Aj, const csr_ask &ask, int v, bool cols_known, column_profile *cp, hipStream_t s)
{
    // v == 0 here: only the rules of round 4 for CACHE-RESIDENT matrices admitted this one -- f64 rows of fewer than 8 entries whose
    // columns share x lines run wave tiles with V = 1, gather-bound band matrices V = 2 (f64) / 4 (f32); else nothing changes
    const bool small_only = v == 0;
    const bool short_rule = small_only && short_f64_rows(p->rows, p->nnz, p->prof, p->dtype, cols_known);
    const bool band_rule = small_only && band_candidate(p->rows, p->nnz, p->prof, p->dtype, cols_known);
    wavev_choice c{small_only ? 1 : v};
    if (ask.wavev()) {
        c.wavex = ask.kernel == CMI_CSR_STREAM_WAVEX;
        c.window = ask.window;
    } else {
        if (int st = column_profile_of(p, Ap, Aj, s, cp)) return st;
        wavev_refine(p, *cp, small_only, short_rule, band_rule, &c);
    }
    if (c.keep_stream) return CMI_SUCCESS; // (the table's csr_stream entry stays: nothing is built)
    int st = wave_partition_build(p, Ap, c.v, s, 256 * c.v - (int)p->prof.max_len - 3);
    if (st != CMI_SUCCESS || !p->wave_row_start) return st;
    // (rows_per_block: the partition's; WAVEX: the window length, 0 = the default.  A caller's policy bits are kept as given)
    adopt_wave_shape(&p->cfg, p->nnz, c.wavex ? CMI_CSR_STREAM_WAVEX : CMI_CSR_STREAM_WAVEV, c.wavex ? c.window : 0, c.v, sizeof(int) + (p->dtype == CMI_F64 ? 8 : 4),
                     ask.wavev() && ask.lookup.nontemporal);
    // ... and so is a caller's XCD dealing (< 0: launch order) -- select_config takes only block size and policy from an AUTO-kernel
    // config, so until session 29 of round 4 an asked-for dealing was silently the table's (the "sweeps" of it measured nothing)
    if (ask.wavev() && ask.lookup.xcd_swizzle != 0) p->cfg.xcd_swizzle = ask.lookup.xcd_swizzle < 0 ? 0 : ask.lookup.xcd_swizzle;
    if (ask.cols16 && p->cfg.kernel == CMI_CSR_STREAM_WAVEV) st = wavev_cols16_build(p, Aj, s); // (asked for; not granted: the bit stays clear)
    return st;
}

// csr_wave on a plan-built partition: asked for, or ($CMI_CSR_WAVE=2) for every AUTO plan whose rows qualify -- see wave_partition_k
static int route_wave_partition(cmi_plan *p, const int *Ap, const csr_ask &ask, hipStream_t s)
{
    const int k = wave_partition_k(p->rows, p->nnz, p->prof, ask.partition(), ask.v);
    if (ask.partition() && k == 0)
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_create: wave tiles on a row partition need 2..10 entries per lane and the longest row <= 6.4 x that");
    if (k == 0) return CMI_SUCCESS;
    const int st = wave_partition_build(p, Ap, k, s);
    if (st != CMI_SUCCESS || !p->wave_row_start) return st;
    // (rows_per_block: the partition's, about Q / mean rows per wave.  A caller's policy bits are kept as given)
    adopt_wave_shape(&p->cfg, p->nnz, CMI_CSR_STREAM_WAVE, 0, k, sizeof(int) + (p->dtype == CMI_F64 ? 8 : 4), ask.partition() && ask.lookup.nontemporal);
    return CMI_SUCCESS;
}

// Which kernel a CSR plan runs instead of the table's csr_stream entry: the routes below are tried in this order and the first whose guard
// passes claims the matrix -- even when it then builds nothing (csr_stream kept, a partition not built).  A builder's error ends plan creation.
// DESIGN.md 3.1 has the order as a table.
static int plan_csr_routes(cmi_plan *p, const int *Ap, const int *Aj, const void *values, const csr_ask &ask, bool auto_kernel, hipStream_t s)
{
    const size_t vbytes = p->dtype == CMI_F64 ? 8 : 4;
    // open: no kernel named by the caller (or one of csr_ask's, stripped), and the table -- after the balanced override and the default
    // 16-bit copy -- says csr_stream with one lane per row
    const bool open = auto_kernel && table_stream(p->cfg);
    const bool fits = wave_tiles_fit(p->rows, p->nnz, p->prof.max_len);
    const bool asked_nothing = ask.kernel == CMI_KERNEL_AUTO;
    column_profile cp;
    int st = CMI_SUCCESS;
    // Rows that all have (nearly) the same short length -- stencils -- take csr_stream's lane-strided body with wave-private
    // tiles (spmv_csr.hip csr_wave_kernel): 64 rows per wave, as many entries per lane as the longest row has, so every
    // tile fits and (mean within 7 % of the longest row) at least 93 % of the request lanes carry an entry.  Cache policy and
    // XCD dealing are the table's csr_stream entry's.  Not for a caller's explicit kernel, not over a granted 16-bit copy.
    // Equal short rows are a stencil's signature -- but only its columns make it one.  A plan made WITH the columns looks: where 75 %+ of
    // the entries sit 16+ columns from their predecessor in the row (a 5-point stencil: 40 %, 7-point: 57 %, 9-point: 33 %; columns drawn
    // anywhere inside a band: 97 %) the matrix is gather-bound and none of the stencil kernels below is right for it -- 6 / 9 entries per
    // row exactly, columns anywhere in +-2000: csr_wave / V = 1 tiles 161-167 us (f64), 94-95 (f32), where the general rule further down
    // (wave tiles V = 4, with the x window) gets 120-138 and 70-85 (profiles/r04_auto_regret_equal_lengths.txt).  Without the columns
    // the lengths decide, as before.
    bool gather_bound = false;
    if (open && fits && asked_nothing && Aj) {
        if ((st = column_profile_of(p, Ap, Aj, s, &cp))) return st;
        gather_bound = (double)cp.jump_count >= 0.75 * (double)p->nnz;
    }
    if (open && fits && asked_nothing && !gather_bound) {
        // stencil rows of 8+ entries whose columns come in runs (9-point: three runs of 3) and a plan made with the columns: the
        // run-compressed copy, tried BEFORE csr_wave (waver_try's own gates: the table's rule; pieces shorter than it asks -> nothing
        // is kept and csr_wave below runs).  9-point 3000^2: 143.9 us against csr_wave's 187.1 (f64), 89.8 against 134.0 (f32),
        // profiles/r04_auto_regret.txt -- until then every stencil-like matrix took csr_wave unseen.
        if (Aj && waver_try(p, Ap, Aj, false, 0, 0, false, nullptr, s, &st)) return CMI_SUCCESS;
        if (st != CMI_SUCCESS) return st;
        if (const int sv = stencil_vector_tiles(p->nnz, p->prof, p->dtype, vbytes)) return route_stencil_vector_tiles(p, Ap, Aj, sv, s);
    }
    if (open && fits && !gather_bound && !ask.wavev() && !ask.waver()) { // (csr_wave's fixed tiles; a caller who asked for a partition lands here too)
        adopt_wave_shape(&p->cfg, p->nnz, CMI_CSR_STREAM_WAVE, 256, (int)p->prof.max_len, sizeof(int) + vbytes, false);
        return CMI_SUCCESS;
    }
    if (open && fits && ask.packed() && values && Aj) {
        // (stencil-like rows: packed wave tiles of the 16-bit copy, spmv_csr16.hip; p->cfg is set)
        if (packed16_try(p, Ap, Aj, values, ask.lookup.nontemporal != 0, s, &st)) return CMI_SUCCESS;
        if (st != CMI_SUCCESS) return st;
    }
    if (open && !ask.partition() && !ask.wavev() && Aj) {
        if (waver_try(p, Ap, Aj, ask.waver(), ask.v, ask.cap, ask.waver() && ask.lookup.nontemporal != 0, ask.packed() ? values : nullptr, s, &st)) {
            // (the run-compressed copy was built and pays: p->cfg is set; a caller's XCD dealing is kept as given)
            if (ask.waver() && ask.lookup.xcd_swizzle != 0) p->cfg.xcd_swizzle = ask.lookup.xcd_swizzle < 0 ? 0 : ask.lookup.xcd_swizzle;
            return CMI_SUCCESS;
        }
        if (st != CMI_SUCCESS) return st;
    }
    if (ask.waver())
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_create: CMI_CSR_STREAM_WAVER / _PACKED need f64 values, 2 <= columns < 2^30, items_per_thread 0, 1, 2 or 4, no row of 512+ entries and the longest row at most half of the 256 x items_per_thread slots of a wave tile");
    if (open && !ask.partition()) { // (a caller who asked for csr_wave on a partition gets that)
        const bool cols_known = Aj != nullptr && !ask.wavev();
        const int v = wavev_vectors(p->rows, p->nnz, p->prof, ask.wavev(), ask.v, vbytes);
        if (v > 0 || short_f64_rows(p->rows, p->nnz, p->prof, p->dtype, cols_known) || band_candidate(p->rows, p->nnz, p->prof, p->dtype, cols_known))
            return route_wavev(p, Ap, Aj, ask, v, cols_known, &cp, s);
    }
    if (ask.wavev())
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_create: CMI_CSR_STREAM_WAVEV needs items_per_thread 0, 1, 2 or 4, no row of 512+ entries and the longest row at most half of the 256 x items_per_thread slots of a wave tile");
    return open ? route_wave_partition(p, Ap, ask, s) : CMI_SUCCESS;
}

// A CSR plan's measurements and choices: the row-length profile, the balanced override, the default 16-bit copy, then the routes
static int plan_csr(cmi_plan *p, const int *Ap, const int *Aj, const void *values, const csr_ask &ask, bool auto_kernel, bool want16, bool table_shape, hipStream_t s)
{
    const int64_t num_rows = p->rows, num_entries = p->nnz;
    int64_t ends[2] = {0, num_entries};
    if (int st = measure_row_lengths(num_rows, Ap, s, &p->prof.max_len, &p->prof.in_long, ends)) return st;
    // the kernels and the plan-owned arrays (wave partition, 16-bit copy) are sized from num_entries: row offsets that do not span
    // exactly [0, num_entries] are refused here, once, instead of being trusted by every multiply
    if (ends[0] != 0 || ends[1] != num_entries) {
        set_error("cmi_plan_create: row offsets run from %lld to %lld, expected 0 to num_entries = %lld", (long long)ends[0], (long long)ends[1], (long long)num_entries);
        return CMI_ERROR_INVALID_VALUE;
    }
    if (auto_kernel && prefers_balanced(num_rows, num_entries, p->prof, p->dtype == CMI_F64 ? 8 : 4, p->cfg.threads_per_row == 1)) {
        p->cfg.kernel = CMI_CSR_BALANCED;
        p->cfg.items_per_thread = 0; // the table's row-tile launch shape does not apply: balanced defaults
        p->cfg.blocks_per_cu = 0;
        p->cfg.xcd_swizzle = 0;      // (chunks in launch order: a skewed matrix has no x window worth dealing for)
    }
    if (want16 && table_stream(p->cfg)) {
        // the tiling is frozen into the copy, so the fused-dot instance cannot re-tile as spmv_csr.hip does for it: a
        // table-chosen shape takes whole waves of rows per tile here, for every multiply, when one LDS pass holds them
        const int tuned_rpb = p->cfg.rows_per_block;
        if (table_shape) {
            const int rpb = p->cfg.rows_per_block, up = (rpb + kWave - 1) / kWave * kWave;
            const double mean = (double)num_entries / (double)num_rows;
            if (up != rpb && up <= p->cfg.block_size && (double)up * mean + 3.0 <= (double)p->cfg.block_size * p->cfg.items_per_thread * 4) p->cfg.rows_per_block = up;
        }
        // (stencil-like rows and the table's shape: the copy is tiled for the wave-tile kernel instead -- 64 rows per tile)
        const int wave_k = table_shape && wave_tiles_fit(num_rows, num_entries, p->prof.max_len) ? (int)p->prof.max_len : 0;
        const int st = csr16_build(p, Ap, Aj, s, wave_k); // all tiles qualify -> cfg.kernel = CMI_CSR_STREAM_C16, else unchanged
        if (p->cfg.kernel != CMI_CSR_STREAM_C16) p->cfg.rows_per_block = tuned_rpb; // not granted: csr_stream as tuned
        if (st != CMI_SUCCESS) return st;
    }
    return plan_csr_routes(p, Ap, Aj, values, ask, auto_kernel, s);
}

// A COO plan: are the entries sorted by row?  Then the tile kernel's table entry and -- no kernel asked for -- row offsets and a CSR sub-plan
static int plan_coo(cmi_plan *p, const int *Ai, const int *Aj, const cmi_config *cfg, void *stream)
{
    const int64_t num_rows = p->rows, num_cols = p->cols, num_entries = p->nnz;
    int sorted = 1, long_runs = 0;
    if (num_entries > 0)
        if (int st = coo_rows_sorted(num_rows, num_entries, Ai, as_stream(stream), &sorted, &long_runs)) return st;
    p->coo_sorted = sorted;
    const bool auto_kernel = !cfg || cfg->kernel == CMI_KERNEL_AUTO;
    // sorted entries: the table's CMI_TABLE_COO_SORTED key (the tile kernel with its tuned cache policy / XCD dealing)
    // (fewer than four entries: the tile kernel's vector loads have nothing to read -- the order-agnostic kernel stays)
    // (a row of more than 1024 entries: the tile kernel would walk its tail serially -- the order-agnostic kernel stays)
    if (sorted && !long_runs && auto_kernel && num_entries >= 4) select_config(CMI_TABLE_COO_SORTED, p->dtype, num_rows, num_cols, num_entries, cfg, &p->cfg);
    // Sorted entries and no kernel asked for: the row indices carry no more than row offsets do.  The plan builds the
    // offsets once (4 bytes per row of HBM it owns) and a CSR plan for them; every multiply then streams 12 bytes per
    // entry instead of 16 through the CSR kernels -- same products, storage-order sums, rows of any length.
    // ($CMI_COO_PLAN_OFFSETS=0: keep the COO kernels -- measurements of the tile kernel.)
    const char *off = std::getenv("CMI_COO_PLAN_OFFSETS");
    int st = CMI_SUCCESS;
    if (sorted && auto_kernel && num_entries >= 4 && num_rows > 0 && num_entries <= INT32_MAX - 65536 && !(off && off[0] == '0')) {
        hipError_t e = p->coo_offsets.alloc((size_t)num_rows + 1);
        if (e != hipSuccess) st = hip_fail(e, "cmi_plan_create: COO row offsets");
        int sorted2 = 0;
        if (st == CMI_SUCCESS) st = cmi_coo_row_offsets(num_rows, num_entries, Ai, p->coo_offsets.get(), &sorted2, stream);
        if (st == CMI_SUCCESS && sorted2)
            st = plan_create(CMI_FORMAT_CSR, p->dtype, num_rows, num_cols, num_entries, p->coo_offsets.get(), Aj /* cmi_plan_create_coo: the CSR plan may then hold the run-compressed copy */, nullptr, stream, &p->coo_csr_plan);
        if (st == CMI_SUCCESS && p->coo_csr_plan) p->cfg = p->coo_csr_plan->cfg; // what cmi_plan_config reports: the kernel that runs
    }
    // an explicit CMI_COO_TILE on unsorted entries would add rows up wrongly: refuse it here, where it is known
    if (st == CMI_SUCCESS && !sorted && p->cfg.kernel == CMI_COO_TILE) st = fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_create: CMI_COO_TILE needs row-sorted entries");
    return st;
}

static int plan_create(int format, int dtype, int64_t num_rows, int64_t num_cols, int64_t num_entries,
                       const int32_t *index_array, const int32_t *csr_columns, const cmi_config *cfg, void *stream, cmi_plan **plan_out, const void *csr_values)
{
    if (!plan_out) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_create: null result pointer");
    *plan_out = nullptr;
    if (format < 0 || format >= CMI_FORMAT_COUNT || dtype < 0 || dtype > 1)
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_create: bad format or value type");
    if (num_rows < 0 || num_cols < 0 || num_entries < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_create: negative size");
    if (num_rows > INT32_MAX || num_cols > INT32_MAX) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_create: sizes exceed the int32 index type");
    // a CSR plan is for cmi_spmv_csr_* / cmi_spmm_csr_*, which take at most INT32_MAX - 65536 entries ("int32 index
    // ceiling"): refused here rather than by the first multiply
    if (format == CMI_FORMAT_CSR && num_entries > INT32_MAX - 65536)
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_create: more than INT32_MAX - 65536 CSR entries (the CSR kernels' ceiling)");
    const bool indexed = format == CMI_FORMAT_CSR || format == CMI_FORMAT_COO;
    if (indexed && !index_array && (format == CMI_FORMAT_CSR ? num_rows > 0 : num_entries > 0))
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_create: CSR / COO plans need the row offsets / row indices");
    cmi_plan *p = plan_new(format, dtype, num_rows, num_cols, num_entries);
    if (!p) return fail(CMI_ERROR_ALLOC, "cmi_plan_create: out of host memory");
    p->cfg_explicit = cfg && cfg->kernel != CMI_KERNEL_AUTO && !(cfg->kernel == CMI_CSR_STREAM_C16 && !(cfg->block_size || cfg->rows_per_block || cfg->items_per_thread));
    // CMI_CSR_STREAM_C16 is csr_stream's shape (the caller's launch-shape fields if any, else the table's) + the 16-bit copy
    cmi_config shape;
    bool want16 = false, table_shape = !cfg || cfg->kernel == CMI_KERNEL_AUTO;
    if (format == CMI_FORMAT_CSR && csr_columns) {
        if (cfg && cfg->kernel == CMI_CSR_STREAM_C16) {
            want16 = true;
            shape = *cfg;
            table_shape = !(cfg->block_size || cfg->rows_per_block || cfg->items_per_thread);
            shape.kernel = table_shape ? CMI_KERNEL_AUTO : CMI_CSR_STREAM;
            cfg = &shape;
        } else if (table_shape && compress_default())
            want16 = true;
    }
    csr_ask ask;
    if (format == CMI_FORMAT_CSR) cfg = csr_ask_from(cfg, csr_columns != nullptr, &ask);
    if (ask.waver() && !csr_columns && num_entries > 0) { delete p; return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_create: CMI_CSR_STREAM_WAVER needs the column indices -- use cmi_plan_create_csr"); }
    p->kernel_asked = ask.kernel != CMI_KERNEL_AUTO;
    if (p->kernel_asked) p->cfg_explicit = false;
    // HYB's table key is its ELL part's (the COO part looks its own shape up per call)
    select_config(format == CMI_FORMAT_HYB ? CMI_FORMAT_ELL : format, dtype, num_rows, num_cols, num_entries, cfg, &p->cfg);
    if (format == CMI_FORMAT_CSR) p->cfg.nontemporal &= ~kPolCols16; // (only a granted copy sets it, below)
    hipStream_t s = as_stream(stream);
    int st = CMI_SUCCESS;
    if (format == CMI_FORMAT_CSR && num_rows > 0 && num_entries > 0)
        st = plan_csr(p, index_array, csr_columns, csr_values, ask, !cfg || cfg->kernel == CMI_KERNEL_AUTO, want16, table_shape, s);
    else if (format == CMI_FORMAT_COO)
        st = plan_coo(p, index_array, csr_columns, cfg, stream);
    if (st == CMI_SUCCESS && indexed && index_array && index_length(p) > 0) {
        st = fingerprint(index_length(p), index_array, s, &p->fp_index);
        p->has_fp_index = st == CMI_SUCCESS;
    }
    if (st == CMI_SUCCESS && (p->runs_packed || p->csr16_packed) && csr_values) {
        st = fingerprint(num_entries * (dtype == CMI_F64 ? 2 : 1), reinterpret_cast<const int *>(csr_values), s, &p->fp_values);
        p->has_fp_values = st == CMI_SUCCESS;
    }
    if (st == CMI_SUCCESS && p->coo_csr_plan && p->coo_csr_plan->has_fp_columns) { // (a COO plan made with the columns: its CSR sub-plan's copy is what cmi_plan_validate guards)
        p->fp_columns = p->coo_csr_plan->fp_columns;
        p->has_fp_columns = true;
    }
    if (st == CMI_SUCCESS && (p->csr16_cols || p->runs_pieces || p->csr16_packed || p->wavev_cols16) && csr_columns) {
        st = fingerprint(num_entries, csr_columns, s, &p->fp_columns);
        p->has_fp_columns = st == CMI_SUCCESS;
    }
    if (st != CMI_SUCCESS) { (void)cmi_plan_destroy(p); return st; }
    *plan_out = p;
    return CMI_SUCCESS;
}

// HYB: the ELL part's launch shape, the COO part's order and -- when it is sorted by row -- the per-tile entry ranges the
// one-launch kernel (spmv_coo_hyb.hip hyb_tile_kernel) reads (one int per 256 rows, owned by the plan); a heavy or unsorted COO
// part gets a COO plan of its own for the second launch.
CMI_API int cmi_plan_create_hyb(int dtype, int64_t num_rows, int64_t num_cols, int64_t ell_entries_per_row,
                                int64_t coo_entries, const int32_t *coo_row_indices, const cmi_config *cfg_ell,
                                const cmi_config *cfg_coo, void *stream, cmi_plan **plan_out)
{
    if (!plan_out) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_create_hyb: null result pointer");
    *plan_out = nullptr;
    if (dtype < 0 || dtype > 1) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_create_hyb: bad value type");
    if (num_rows < 0 || num_cols < 0 || ell_entries_per_row < 0 || coo_entries < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_create_hyb: negative size");
    if (num_rows > INT32_MAX || num_cols > INT32_MAX || ell_entries_per_row > INT32_MAX)
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_create_hyb: sizes exceed the int32 index type");
    if (coo_entries > 0 && !coo_row_indices) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_create_hyb: the COO part's row indices are needed");
    cmi_plan *p = plan_new(CMI_FORMAT_HYB, dtype, num_rows, num_cols, num_rows * ell_entries_per_row);
    if (!p) return fail(CMI_ERROR_ALLOC, "cmi_plan_create_hyb: out of host memory");
    p->hyb_width = ell_entries_per_row;
    p->hyb_coo = coo_entries;
    select_config(CMI_FORMAT_ELL, dtype, num_rows, num_cols, p->nnz, cfg_ell, &p->cfg);
    select_config(CMI_FORMAT_COO, dtype, num_rows, num_cols, coo_entries, cfg_coo, &p->hyb_coo_cfg);
    hipStream_t s = as_stream(stream);
    int st = CMI_SUCCESS;
    if (coo_entries > 0 && num_rows > 0) {
        int sorted = 0, long_runs = 0;
        st = coo_rows_sorted(num_rows, coo_entries, coo_row_indices, s, &sorted, &long_runs);
        if (st == CMI_SUCCESS) p->coo_sorted = sorted;
        // sorted: the two-launch path's COO half is the tile kernel (storage-order sums on top of the ELL half: still one chain)
        if (st == CMI_SUCCESS && sorted && !long_runs && coo_entries >= 4 && (!cfg_coo || cfg_coo->kernel == CMI_KERNEL_AUTO))
            select_config(CMI_TABLE_COO_SORTED, dtype, num_rows, num_cols, coo_entries, cfg_coo, &p->hyb_coo_cfg);
        const char *force = std::getenv("CMI_HYB_ONE_LAUNCH"); // "0": never, "1": whenever the COO part is sorted, else: by its weight
        const bool never = force && force[0] == '0', always = force && force[0] == '1';
        if (st == CMI_SUCCESS && sorted && !never && coo_entries <= INT32_MAX - 4096 &&
            (always || (double)coo_entries <= kHybFusedMaxPerRow * (double)num_rows)) {
            const int64_t tiles = ceil_div(num_rows, kHybTileRows);
            device_array<int32_t> tile_start;
            device_counters<int> max_in_tile;
            hipError_t e = tile_start.alloc((size_t)tiles + 1);
            if (e == hipSuccess) e = max_in_tile.open(s);
            if (e != hipSuccess) st = hip_fail(e, "cmi_plan_create_hyb: tile ranges");
            if (st == CMI_SUCCESS) st = hyb_tile_starts(num_rows, coo_entries, coo_row_indices, tile_start.get(), max_in_tile.dev(), s);
            if (st == CMI_SUCCESS && (e = max_in_tile.fetch(s)) != hipSuccess) st = hip_fail(e, "cmi_plan_create_hyb: tile ranges");
            // (a few rows hold the COO part: the ranges are dropped here, two launches)
            if (st == CMI_SUCCESS && (always || max_in_tile.host[0] <= kHybFusedMaxInTile)) p->hyb_tile_start = std::move(tile_start);
        }
        // two launches: the COO half multiplies through a COO plan of its own (sorted entries: the CSR kernels on row offsets,
        // accumulating on top of the ELL half -- per row still the host chain)
        if (st == CMI_SUCCESS && !p->hyb_tile_start)
            st = plan_create(CMI_FORMAT_COO, dtype, num_rows, num_cols, coo_entries, coo_row_indices, nullptr, cfg_coo, stream, &p->hyb_coo_plan);
        if (st == CMI_SUCCESS) {
            st = fingerprint(coo_entries, coo_row_indices, s, &p->fp_index);
            p->has_fp_index = st == CMI_SUCCESS;
        }
    }
    if (st != CMI_SUCCESS) { (void)cmi_plan_destroy(p); return st; }
    *plan_out = p;
    return CMI_SUCCESS;
}

CMI_API int cmi_plan_hyb_launches(const cmi_plan *plan, int *launches)
{
    if (!plan || !launches || plan->format != CMI_FORMAT_HYB) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_hyb_launches: not a HYB plan");
    *launches = (plan->hyb_tile_start || plan->hyb_coo == 0) ? 1 : 2;
    return CMI_SUCCESS;
}

// y[i] = (A x)[i] * scale[i] for every later multiply through this plan (NULL: plain again).  Launches nothing and reads nothing on the device;
// only the plans whose multiply is ONE launch of hyb_tile_kernel take it (tile ranges, or an empty COO part).
CMI_API int cmi_plan_set_row_scale(cmi_plan *plan, const void *scale_dev)
{
    if (!plan) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_set_row_scale: null plan");
    if (plan->format != CMI_FORMAT_HYB || !(plan->hyb_tile_start || plan->hyb_coo == 0))
        return fail(CMI_ERROR_NOT_SUPPORTED, "cmi_plan_set_row_scale: only a HYB plan that multiplies in one launch carries a row scale");
    plan->row_scale = scale_dev;
    return CMI_SUCCESS;
}

CMI_API int cmi_plan_wavev_shift_tiles(const cmi_plan *plan, int64_t *marked)
{
    if (!plan || !marked) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_wavev_shift_tiles: null argument");
    *marked = plan->wavev_shift ? plan->wavev_shift_marked : 0;
    return CMI_SUCCESS;
}

CMI_API int cmi_plan_const_tiles(const cmi_plan *plan, int64_t *tiles)
{
    if (!plan || !tiles) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_const_tiles: null argument");
    *tiles = plan->wavev_const ? plan->wavev_const_tiles : 0;
    return CMI_SUCCESS;
}

// Frees the constant tiles' marks (a plan without them: nothing happens).  Launches nothing; the free waits for the multiplies already
// enqueued, as any hipFree does.  From here on the plan multiplies exactly as a plan made without the values.
CMI_API int cmi_plan_drop_const_tiles(cmi_plan *plan)
{
    if (!plan) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_drop_const_tiles: null plan");
    plan->wavev_const.reset();
    plan->wavev_const_tiles = 0;
    return CMI_SUCCESS;
}

CMI_API int cmi_plan_destroy(cmi_plan *plan)
{
    if (!plan) return CMI_SUCCESS;
    if (plan->hyb_coo_plan) (void)cmi_plan_destroy(plan->hyb_coo_plan);
    if (plan->coo_csr_plan) (void)cmi_plan_destroy(plan->coo_csr_plan);
    delete plan; // (its device_array fields free their blocks)
    return CMI_SUCCESS;
}

CMI_API int cmi_plan_config(const cmi_plan *plan, cmi_config *out)
{
    if (!plan || !out) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_config: null argument");
    *out = plan->cfg;
    return CMI_SUCCESS;
}

CMI_API int cmi_plan_info(const cmi_plan *plan, int64_t *max_row_length, int64_t *entries_in_long_rows, int *coo_sorted,
                          int *storage_order_sums)
{
    if (!plan) return fail(CMI_ERROR_INVALID_VALUE, "cmi_plan_info: null plan");
    if (max_row_length) *max_row_length = plan->format == CMI_FORMAT_CSR ? plan->prof.max_len : -1;
    if (entries_in_long_rows) *entries_in_long_rows = plan->format == CMI_FORMAT_CSR ? plan->prof.in_long : -1;
    if (coo_sorted) *coo_sorted = plan->coo_sorted;
    if (storage_order_sums) {
        int exact = 0;
        const cmi_config &c = plan->cfg;
        switch (plan->format) {
        case CMI_FORMAT_CSR:
            // scalar / pipe: always; stream: one lane per row and no row long enough for the cooperative path
            exact = c.kernel == CMI_CSR_SCALAR || c.kernel == CMI_CSR_STREAM_PIPE || c.kernel == CMI_CSR_STREAM_C16 || c.kernel == CMI_CSR_STREAM_WAVE || c.kernel == CMI_CSR_STREAM_WAVEV || c.kernel == CMI_CSR_STREAM_WAVEX || c.kernel == CMI_CSR_STREAM_WAVER || c.kernel == CMI_CSR_STREAM_PACKED ||
                    (c.kernel == CMI_CSR_STREAM && c.threads_per_row <= 1 && (c.threads_per_row == 1 || plan->prof.max_len < 512));
            break;
        case CMI_FORMAT_ELL: exact = ell_lanes_per_row(c, plan->rows, plan->rows > 0 ? plan->nnz / plan->rows : 0) == 1; break;
        case CMI_FORMAT_DIA: exact = 1; break;
        case CMI_FORMAT_COO:
            if (plan->coo_csr_plan) { // through the row offsets: the CSR kernel's class
                int sub = 0;
                (void)cmi_plan_info(plan->coo_csr_plan, nullptr, nullptr, nullptr, &sub);
                exact = sub;
            } else
                exact = c.kernel == CMI_COO_TILE;
            break;
        default: // HYB: one launch = one chain per row; two launches: the same chain when the COO half is the tile kernel, else atomics
            exact = (bool)plan->hyb_tile_start;
            if (!exact && ell_lanes_per_row(c, plan->rows, plan->hyb_width) == 1) {
                int sub = plan->hyb_coo == 0;
                if (plan->hyb_coo_plan) (void)cmi_plan_info(plan->hyb_coo_plan, nullptr, nullptr, nullptr, &sub);
                exact = sub;
            }
            break;
        }
        *storage_order_sums = exact;
    }
    return CMI_SUCCESS;
}

// blas1_shared.h -- what the streaming BLAS-1 kernels of blas1.hip and the multi-shift kernels of krylov_m.hip have in common: the
// workgroup size, the 16-byte lane type, the run-time nt-store policy and the two grid rules.  One definition, two translation units.
#pragma once
#include "common.h"

namespace cmi {

constexpr int kBlasBlock = 256;
constexpr int kFusedMaxGrid = 1 << 16;           // fused update+reduce kernels store too: near one-shot grids (one partial per workgroup; the folds take up to kPartialCapacity)

// element-wise kernels that STORE: one-shot grid, a workgroup per chunk (tools/membench.hip: stores
// from a capped grid-stride grid run at 4.5-5.0 TB/s, one-shot at 6.3-6.9 TB/s)
inline int stream_grid(int64_t n, int per_thread)
{
    int64_t b = ceil_div(n, (int64_t)kBlasBlock * per_thread);
    const int64_t cap = (int64_t)1 << 22;
    if (b > cap) b = cap;
    return b < 1 ? 1 : (int)b;
}

// near one-shot, capped at kFusedMaxGrid workgroups (grid-strided past it)
inline int fused_grid(int64_t n, int per_thread)
{
    int64_t b = ceil_div(n, (int64_t)kBlasBlock * per_thread);
    if (b > kFusedMaxGrid) b = kFusedMaxGrid;
    return b < 1 ? 1 : (int)b;
}

// 16 bytes per lane: 2 doubles or 4 floats
template <typename T> struct vec16;
template <> struct vec16<double> { typedef double2v type; static constexpr int n = 2; };
template <> struct vec16<float> { typedef float4v type; static constexpr int n = 4; };

// store with or without the nt hint by a run-time flag (uniform)
template <typename V> __device__ __forceinline__ void st_policy(V *p, V v, bool nt)
{
    if (nt) __builtin_nontemporal_store(v, p);
    else *p = v;
}

} // namespace cmi

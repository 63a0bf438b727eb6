// blas1_shared.h -- what the streaming BLAS-1 kernels of blas1.hip, the multi-shift kernels of krylov_m.hip and the LOBPCG kernels of
// lobpcg.hip have in common: the workgroup size, the 16-byte lane type and a lane's piece of a vector, the run-time nt-store policy, the
// grid rules and the overlap refusal.  One definition, three translation units.
#pragma once
#include "common.h"

#include <initializer_list>

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

// kernels that leave `sums` partial lists side by side in ONE fold area (list j at [j * cap, (j + 1) * cap) with cap = multi_sum_cap(sums)):
// near one-shot, capped so that every list fits -- 8 lists: 16384 workgroups, grid-strided past 16384 * kBlasBlock pieces
constexpr int multi_sum_cap(int sums) { return kPartialCapacity / sums; }
inline int multi_sum_grid(int64_t n, int per_thread, int sums)
{
    int64_t b = ceil_div(n, (int64_t)kBlasBlock * per_thread);
    if (b > multi_sum_cap(sums)) b = multi_sum_cap(sums);
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

// a lane's piece of one vector: cnt <= W elements from `base`; wide (uniform but for the last piece): one 16-byte access; nt: a stream read once
template <typename T> __device__ __forceinline__ typename vec16<T>::type ld_piece(const T *base, int cnt, bool wide, bool nt = false)
{
    typedef typename vec16<T>::type V;
    constexpr int W = vec16<T>::n;
    V v = {};
    if (wide) v = nt ? __builtin_nontemporal_load(reinterpret_cast<const V *>(base)) : *reinterpret_cast<const V *>(base);
    else {
#pragma unroll
        for (int k = 0; k < W; k++)
            if (k < cnt) v[k] = base[k];
    }
    return v;
}
template <typename T> __device__ __forceinline__ void st_piece(T *base, typename vec16<T>::type v, int cnt, bool wide, bool nt)
{
    typedef typename vec16<T>::type V;
    constexpr int W = vec16<T>::n;
    if (wide) st_policy(reinterpret_cast<V *>(base), v, nt);
    else {
#pragma unroll
        for (int k = 0; k < W; k++)
            if (k < cnt) base[k] = v[k];
    }
}

// ---- refusals, made before any device call ---------------------------------------------------------------------------------------------
struct span { const void *p; size_t bytes; };
inline bool overlap(const span &a, const span &b)
{
    if (!a.p || !b.p || a.bytes == 0 || b.bytes == 0) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a.p), b0 = reinterpret_cast<uintptr_t>(b.p);
    return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}
// every output against every other output and against every input
inline bool any_overlap(std::initializer_list<span> outs, std::initializer_list<span> ins)
{
    for (const span *a = outs.begin(); a != outs.end(); ++a) {
        for (const span *b = a + 1; b != outs.end(); ++b) if (overlap(*a, *b)) return true;
        for (const span &b : ins) if (overlap(*a, b)) return true;
    }
    return false;
}

} // namespace cmi

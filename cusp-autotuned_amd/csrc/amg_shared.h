// amg_shared.h -- what the set-up translation units of smoothed aggregation (amg.hip, mis.hip) share: the size ceiling, the
// launch shape of one lane per row and the clamp of a row offset.
#pragma once
#include "setup_scan.h"

namespace cmi {

constexpr int64_t kAmgCeiling = (int64_t)INT32_MAX - 65536; // entries of a CSR matrix
constexpr int kAmgBlock = 256;

inline unsigned amg_blocks(int64_t n) { return (unsigned)(n < 1 ? 1 : ceil_div(n, kAmgBlock)); }

__device__ __forceinline__ int amg_clamp(int p, int64_t entries) { return p < 0 ? 0 : ((int64_t)p > entries ? (int)entries : p); }

} // namespace cmi

// amg_shared.h -- what the set-up translation units of smoothed aggregation (amg.hip, mis.hip) share: the size ceiling, the
// launch shape of one lane per row, the clamp of a row offset and the scratch of one call.
#pragma once
#include "common.h"

#include <vector>

#include <rocprim/rocprim.hpp>

namespace cmi {

constexpr int64_t kAmgCeiling = (int64_t)INT32_MAX - 65536; // entries of a CSR matrix
constexpr int kAmgBlock = 256;

inline unsigned amg_blocks(int64_t n) { return (unsigned)(n < 1 ? 1 : ceil_div(n, kAmgBlock)); }

__device__ __forceinline__ int amg_clamp(int p, int64_t entries) { return p < 0 ? 0 : ((int64_t)p > entries ? (int)entries : p); }

struct amg_scratch { // device allocations of one call, released on every path out
    std::vector<void *> p;
    hipError_t get(void **out, size_t bytes)
    {
        hipError_t e = hipMalloc(out, bytes ? bytes : 1);
        if (e == hipSuccess) {
            try {
                p.push_back(*out);
            } catch (const std::bad_alloc &) {
                (void)hipFree(*out);
                *out = nullptr;
                return hipErrorOutOfMemory;
            }
        }
        return e;
    }
    ~amg_scratch() { for (void *q : p) (void)hipFree(q); }
};

} // namespace cmi

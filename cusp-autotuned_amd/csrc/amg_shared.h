// amg_shared.h -- what the set-up translation units of smoothed aggregation (amg.hip, evolution.hip, mis.hip) and the graph searches (bfs.hip)
// share: the size ceiling, the launch shape of one lane per row, the clamp of a row offset and the one-allocation scratch arena.
#pragma once
#include "setup_scan.h"

namespace cmi {

constexpr int64_t kAmgCeiling = (int64_t)INT32_MAX - 65536; // entries of a CSR matrix
constexpr int kAmgBlock = 256;

inline unsigned amg_blocks(int64_t n) { return (unsigned)(n < 1 ? 1 : ceil_div(n, kAmgBlock)); }

__device__ __forceinline__ int amg_clamp(int p, int64_t entries) { return p < 0 ? 0 : ((int64_t)p > entries ? (int)entries : p); }

// One device allocation per call, carved in 256-byte steps: a dozen allocate / free pairs of N-sized arrays cost more than
// the sweeps they serve.  take() returns null once the reservation is used up (the caller sized it: a bug, reported as one).
struct device_arena {
    device_array<char> block; // released with the arena, on every path out of the call
    size_t used = 0;
    static size_t padded(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
    hipError_t open(size_t bytes) { return block.alloc(bytes); }
    template <typename T> T *take(size_t count)
    {
        const size_t bytes = padded(count * sizeof(T));
        if (!block || used + bytes > block.bytes()) return nullptr;
        T *p = reinterpret_cast<T *>(block.get() + used);
        used += bytes;
        return p;
    }
};

} // namespace cmi

// cusp/detail/random_hash.h -- the ONE definition of the values of cusp::random_array, compiled for the host by the header layer and for the
// device by csrc/eigen.hip (cmi_random_fill_*), so that an array filled on either side holds the same bits.
//   random_hash(i, seed)   splitmix64's output function (Steele, Lea, Flood 2014) of the state seed + (i + 1) * 0x9E3779B97F4A7C15: a function of
//                          (position, seed) alone.  The library's own choice -- NOT the reference's integer hash, whose values are not reproduced.
//   random_unit(h, T *)    uniform in [0, 1): double (h >> 11) * 2^-53, float (h >> 40) * 2^-24.  Both conversions are exact, so 1.0 never comes out.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CUSP_HOST_DEVICE __host__ __device__
#else
#define CUSP_HOST_DEVICE
#endif

namespace cusp {
namespace detail {

CUSP_HOST_DEVICE inline uint64_t random_hash(uint64_t i, uint64_t seed)
{
    uint64_t z = seed + (i + 1u) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
CUSP_HOST_DEVICE inline double random_unit(uint64_t h, double *) { return static_cast<double>(h >> 11) * (1.0 / 9007199254740992.0); }
CUSP_HOST_DEVICE inline float random_unit(uint64_t h, float *) { return static_cast<float>(h >> 40) * (1.0f / 16777216.0f); }

} // namespace detail
} // namespace cusp

// setup_scan.h -- what set-up code shares on top of rocPRIM (a library primitive of ROCm, not a hot-path kernel): its temporary
// storage protocol written once, and row offsets from per-row counts.  Kept out of common.h: rocPRIM costs every translation unit
// that includes it some 15 s of compile time.
#pragma once
#include "common.h"

#include <rocprim/rocprim.hpp>

namespace cmi {

// A rocPRIM call is given ONCE, as a callable of (void *temp, size_t &bytes) that passes both on: with a null `temp` it only
// reports the bytes it needs.  temp_size() asks for them; with_temp() asks, allocates them in `temp` and runs the call.  `temp`
// is the caller's because the block must outlive the enqueued work.  A site that sizes once and runs many times, or that sizes
// several calls into one block, uses temp_size(), allocates, and then calls `call(block, bytes)` itself.
template <typename F> inline hipError_t temp_size(F &&call, size_t *bytes)
{
    *bytes = 0;
    return call(nullptr, *bytes);
}
template <typename F> inline hipError_t with_temp(device_array<unsigned char> &temp, F &&call)
{
    size_t bytes = 0;
    hipError_t e = temp_size(call, &bytes);
    if (e == hipSuccess) e = temp.alloc(bytes);
    if (e == hipSuccess) e = call(temp.get(), bytes);
    return e;
}

// Row offsets from per-row counts: out[0 .. n] = exclusive prefix sums of in[0 .. n] (in[n] must be 0: the total lands in
// out[n]); `temp` keeps the temporary.  Does not synchronise: a caller that needs the stream idle says so itself.
// offsets_scan() is that scan as a callable for temp_size() / with_temp(), for the caller that brings its own block.
// (Templates on the count type, so that rocPRIM's scan kernels are instantiated only in the translation units that scan.)
template <typename I> inline auto offsets_scan(const I *in, I *out, int64_t n, hipStream_t s)
{
    return [=](void *temp, size_t &bytes) { return rocprim::exclusive_scan(temp, bytes, in, out, I(0), (size_t)(n + 1), rocprim::plus<I>(), s); };
}
template <typename I> inline hipError_t exclusive_offsets(device_array<unsigned char> &temp, const I *in, I *out, int64_t n, hipStream_t s)
{
    return with_temp(temp, offsets_scan(in, out, n, s));
}

} // namespace cmi

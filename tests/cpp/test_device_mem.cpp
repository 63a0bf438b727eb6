// The two owner types of the library's set-up code (cusp-autotuned_amd/csrc/common.h): device_array<T>, one device
// allocation, and device_counters<W, N>, N zeroed words that kernels add into and the host reads back.  Built with hipcc
// (common.h is a HIP header).  Tests named host_* touch no device; tests named gpu_* need one.
#include "../../cusp-autotuned_amd/csrc/common.h"
#include "unittest.h"

using cmi::device_array;
using cmi::device_counters;

static_assert(!std::is_copy_constructible<device_array<int>>::value && !std::is_copy_assignable<device_array<int>>::value, "move-only");
static_assert(std::is_nothrow_move_constructible<device_array<int>>::value && std::is_nothrow_move_assignable<device_array<int>>::value, "moves cannot fail");
static_assert(!std::is_convertible<device_array<int>, int *>::value && !std::is_convertible<device_array<int>, bool>::value, "no implicit conversions");

void host_empty_owner_is_false_and_holds_nothing()
{
    device_array<double> a;
    ASSERT_TRUE(!a);
    ASSERT_TRUE(a.get() == nullptr);
    ASSERT_EQUAL(a.bytes(), (size_t)0);
}
DECLARE_UNITTEST(host_empty_owner_is_false_and_holds_nothing);

void host_moving_and_resetting_an_empty_owner_is_harmless()
{
    device_array<int> a, b(std::move(a));
    a = std::move(b);
    a.reset();
    b.reset();
    ASSERT_TRUE(!a && !b);
    ASSERT_EQUAL(a.bytes() + b.bytes(), (size_t)0);
    device_counters<unsigned long long, 3> c; // not opened: no device block, the host copy reads zero
    ASSERT_TRUE(c.dev() == nullptr);
    ASSERT_EQUAL(c.host[0] + c.host[1] + c.host[2], 0ull);
}
DECLARE_UNITTEST(host_moving_and_resetting_an_empty_owner_is_harmless);

void gpu_alloc_reports_the_bytes_asked_for()
{
    device_array<double> a;
    ASSERT_EQUAL(a.alloc(0), hipSuccess); // (one byte, so that the block has an address)
    ASSERT_TRUE((bool)a && a.get() != nullptr);
    ASSERT_EQUAL(a.bytes(), (size_t)0);
    ASSERT_EQUAL(a.alloc(1000), hipSuccess);
    ASSERT_TRUE((bool)a);
    ASSERT_EQUAL(a.bytes(), (size_t)8000);
    a.reset();
    ASSERT_TRUE(!a);
    ASSERT_EQUAL(a.bytes(), (size_t)0);
}
DECLARE_UNITTEST(gpu_alloc_reports_the_bytes_asked_for);

void gpu_a_move_leaves_the_source_empty()
{
    device_array<int> a;
    ASSERT_EQUAL(a.alloc(300), hipSuccess);
    int *const p = a.get();
    device_array<int> b(std::move(a));
    ASSERT_TRUE(!a && a.bytes() == 0);
    ASSERT_TRUE(b.get() == p && b.bytes() == 1200);
    device_array<int> c;
    ASSERT_EQUAL(c.alloc(7), hipSuccess);
    c = std::move(b); // (c's own block is freed)
    ASSERT_TRUE(!b && b.bytes() == 0);
    ASSERT_TRUE(c.get() == p && c.bytes() == 1200);
}
DECLARE_UNITTEST(gpu_a_move_leaves_the_source_empty);

void gpu_a_second_alloc_replaces_the_first()
{
    device_array<unsigned char> a;
    ASSERT_EQUAL(a.alloc((size_t)1 << 20), hipSuccess);
    unsigned char *const first = a.get();
    ASSERT_EQUAL(a.alloc(4096), hipSuccess);
    ASSERT_TRUE((bool)a);
    ASSERT_EQUAL(a.bytes(), (size_t)4096);
    ASSERT_EQUAL(hipMemset(a.get(), 0, 4096), hipSuccess);
    if (a.get() != first) { // the first block is no device allocation any more (the same address again: it was freed and reused)
        hipPointerAttribute_t attr;
        const hipError_t e = hipPointerGetAttributes(&attr, first);
        (void)hipGetLastError();
        ASSERT_TRUE(e != hipSuccess || attr.type == hipMemoryTypeUnregistered);
    }
}
DECLARE_UNITTEST(gpu_a_second_alloc_replaces_the_first);

__global__ void add_lane_kernel(unsigned long long *out)
{
    atomicAdd(out + threadIdx.x % 3, (unsigned long long)threadIdx.x);
}

void gpu_counters_read_zero_after_open_and_what_a_kernel_added()
{
    hipStream_t s = nullptr;
    device_counters<unsigned long long, 3> c;
    c.host[0] = c.host[1] = c.host[2] = 99;
    ASSERT_EQUAL(c.open(s), hipSuccess);
    ASSERT_EQUAL(c.block.bytes(), (size_t)24);
    ASSERT_EQUAL(c.fetch(s), hipSuccess);
    ASSERT_EQUAL(c.host[0], 0ull);
    ASSERT_EQUAL(c.host[1], 0ull);
    ASSERT_EQUAL(c.host[2], 0ull);
    hipLaunchKernelGGL(add_lane_kernel, dim3(2), dim3(64), 0, s, c.dev());
    ASSERT_EQUAL(hipGetLastError(), hipSuccess);
    ASSERT_EQUAL(c.fetch(s), hipSuccess);
    unsigned long long want[3] = {0, 0, 0};
    for (int b = 0; b < 2; b++)
        for (int t = 0; t < 64; t++) want[t % 3] += t;
    ASSERT_EQUAL(c.host[0], want[0]);
    ASSERT_EQUAL(c.host[1], want[1]);
    ASSERT_EQUAL(c.host[2], want[2]);
}
DECLARE_UNITTEST(gpu_counters_read_zero_after_open_and_what_a_kernel_added);

int main(int argc, char **argv) { return unittest::run_all(argc, argv); }

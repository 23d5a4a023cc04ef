// A stand-in for <hip/hip_runtime.h>, for tests/cpp/decay_bands_kernel_host.cpp only: just enough to compile the TEXT of a kernel that
// uses nothing but blockIdx / threadIdx for the host, one "lane" per call.  Never part of the product.
#pragma once
#include <cstdint>
struct wv_stub_dim3 {
    unsigned x, y, z;
};
static thread_local wv_stub_dim3 blockIdx, threadIdx;
#define __global__
#define __launch_bounds__(n)

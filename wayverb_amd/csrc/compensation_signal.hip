// compensation_signal.hip -- transparent sources: the folded free-field waveguide that produces the mesh's own impulse
// response at the excitation node (wv_compressed_waveguide_run, kernel in compressed_kernels.hip.h), and the host-side
// subtraction of that response from an input (wv_make_transparent).
//
// Replaces compressed_rectangular_waveguide::run (src/waveguide/compensation_signal/lib/include/compensation_signal/
// waveguide.h:42-131) and waveguide::make_transparent (src/waveguide/src/make_transparent.cpp:10-30).  The reference steps
// the mesh with two host round trips per step (write node 0, read node 0); here the input is uploaded once, node 0 is
// written and recorded on the device, and the outputs come back in one copy.
#include "compressed_kernels.hip.h"
#include "engine_base.h"

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

using wv::cw_tetrahedron;
using wv::DeviceGuard;
using wv::fail;
using wv::ScopedDevice;

namespace {

// The largest shell worth updating at step k of K = 2 dim (shells run 0 .. dim - 1; shell dim is the clamp and stays 0):
//   forward:  before step k the current field is zero beyond shell k and the previous one beyond shell k - 1 (node 0, shell 0,
//             is the only source; the stencil moves one shell per step), so every node beyond shell k + 1 computes 0 and
//             already holds 0 -- the buffers are zeroed at the start of every run and such a node has never been written;
//   backward: a value written at step k on shell x reaches node 0 at step k + x at the earliest (it is read one shell further
//             in at every later step), and the last output is node 0 after step K - 1: nodes beyond shell K - 1 - k cannot
//             reach it.  Whatever they would have held is only ever read by nodes that the same bound skips later on.
// Total work: sum_k tetrahedron(r_k + 1) ~ dim^4 / 12 node updates instead of dim^4 / 3 for the whole wedge every step.
int64_t largest_shell(int64_t k, int64_t dim) {
    return std::min(std::min(k + 1, 2 * dim - 1 - k), dim - 1);
}

}  // namespace

extern "C" {

int wv_compressed_waveguide_run(int32_t device, uint64_t steps, int32_t source_kind, const float* input, uint64_t n_input,
                                float* output) {
    if (!output || (n_input && !input)) return fail(WV_E_INVALID_ARGUMENT, "null argument");
    if (source_kind != WV_SOURCE_HARD && source_kind != WV_SOURCE_SOFT)
        return fail(WV_E_INVALID_ARGUMENT, "source_kind must be WV_SOURCE_HARD or WV_SOURCE_SOFT");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
        return fail(WV_E_NO_DEVICE, "no HIP device visible; this engine has no CPU fallback");
    if (steps > (uint64_t)1 << 16)  // (coordinates below 2^15: compressed_kernels.hip.h; fields of 47 TB)
        return fail(WV_E_INVALID_ARGUMENT, "compressed waveguide: more than 65536 steps");
    const int64_t dim = (int64_t)((steps + 1) / 2);
    if (dim == 0) return WV_OK;
    DeviceGuard guard(device);

    const size_t field_bytes = (size_t)cw_tetrahedron(dim + 1) * sizeof(float);
    const size_t out_n = (size_t)(2 * dim);
    size_t free_bytes = 0, total_bytes = 0;
    WV_HIP(hipMemGetInfo(&free_bytes, &total_bytes));
    if (2 * field_bytes + 2 * out_n * sizeof(float) > free_bytes)
        return fail(WV_E_INVALID_ARGUMENT, "compressed waveguide of " + std::to_string(steps) + " steps needs two fields of " +
                                               std::to_string(field_bytes) + " bytes; the device has " +
                                               std::to_string(free_bytes) + " bytes free");

    std::vector<float> padded(out_n, 0.0f);  // the reference feeds 0 once the input is over
    std::copy(input, input + std::min<uint64_t>(n_input, out_n), padded.begin());
    ScopedDevice m_prev, m_cur, m_in, m_out;
    WV_HIP(hipMalloc(&m_prev.p, field_bytes));
    WV_HIP(hipMalloc(&m_cur.p, field_bytes));
    WV_HIP(hipMalloc(&m_in.p, out_n * sizeof(float)));
    WV_HIP(hipMalloc(&m_out.p, out_n * sizeof(float)));
    hipStream_t stream = nullptr;
    WV_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    struct StreamGuard {
        hipStream_t s;
        ~StreamGuard() { (void)hipStreamDestroy(s); }
    } stream_guard{stream};
    // zeroed at the start of every run (waveguide.h:88-98): the light cone relies on it
    WV_HIP(hipMemsetAsync(m_prev.p, 0, field_bytes, stream));
    WV_HIP(hipMemsetAsync(m_cur.p, 0, field_bytes, stream));
    WV_HIP(hipMemcpyAsync(m_in.p, padded.data(), out_n * sizeof(float), hipMemcpyHostToDevice, stream));

    wv::CompressedArgs a{};
    a.prev = static_cast<float*>(m_prev.p);
    a.cur = static_cast<float*>(m_cur.p);
    a.input = static_cast<const float*>(m_in.p);
    a.output = static_cast<float*>(m_out.p);
    a.soft = source_kind == WV_SOURCE_SOFT ? 1 : 0;
    constexpr int64_t block = 256, max_blocks = 256 * 64;  // grid-stride beyond 64 blocks per CU
    for (int64_t k = 0; k < 2 * dim; ++k) {
        a.step = k;
        a.nodes = cw_tetrahedron(largest_shell(k, dim) + 1);
        const int64_t blocks = std::min((a.nodes + block - 1) / block, max_blocks);
        hipLaunchKernelGGL(wv::compressed_waveguide_kernel, dim3((unsigned)blocks), dim3((unsigned)block), 0, stream, a);
        std::swap(a.prev, a.cur);  // waveguide.h:115-117
    }
    WV_HIP(hipGetLastError());
    WV_HIP(hipMemcpyAsync(output, m_out.p, out_n * sizeof(float), hipMemcpyDeviceToHost, stream));
    WV_HIP(hipStreamSynchronize(stream));
    return WV_OK;
}

int wv_make_transparent(const float* input, uint64_t n, const float* response, uint32_t taps, float* out) {
    if ((n && !input) || !response || !out) return fail(WV_E_INVALID_ARGUMENT, "null argument");
    if (taps < 2) return fail(WV_E_INVALID_ARGUMENT, "make_transparent: the response needs at least 2 taps");
    // core::right_hanning(taps) (core/sinc.h:59-72): double arithmetic, stored as float; elementwise_multiply in float
    std::vector<double> windowed(taps);
    for (uint32_t i = 0; i < taps; ++i) {
        const float w = (float)(0.5 - 0.5 * std::cos(2 * M_PI * (0.5 + (i / (2 * (taps - 1.0))))));
        windowed[i] = (double)(w * response[i]);
    }
    // out[i] = (i < n ? input[i] : 0) - (input * windowed)[i], the convolution accumulated in double
    const uint64_t len = n + taps - 1;
    for (uint64_t i = 0; i < len; ++i) {
        const uint64_t j0 = i >= taps - 1 ? i - (taps - 1) : 0, j1 = std::min<uint64_t>(i + 1, n);
        double acc = 0.0;
        for (uint64_t j = j0; j < j1; ++j) acc += (double)input[j] * windowed[i - j];
        out[i] = (float)((i < n ? (double)input[i] : 0.0) - acc);
    }
    return WV_OK;
}

}  // extern "C"

// spectrum_kernels.hip.h -- the fold kernel of field spectra (wv_set_spectrum; engine_spectrum.hip.h launches it).
//
// The captures themselves are snapshot_gather_kernel's (snapshot_kernels.hip.h), unchanged: each writes one dense float box of B
// nodes into a slot of the device-only stage float[T][B].  spectrum_fold_kernel<WIDE> folds the first t staged captures into the
// planar sums double acc[K][2][B] (re plane, im plane per frequency):
//
//     re[k] = re[k] + (double)p_j * c(j, k)        im[k] = im[k] - (double)p_j * s(j, k)        j = 0 .. t-1 in order
//
// a rounded product and a rounded sum each (-ffp-contract=off), so that a NumPy loop over the snapshots reproduces the sums bit
// for bit.  The twiddles tw[t][K][2] come from the host (wv_spectrum_twiddle); their indices depend on loop counters and kernel
// arguments only, never on the lane, so the compiler fetches them through the scalar path.  The device evaluates no trigonometric
// function.
//
// Lanes run along the dense node index.  A lane reads its t staged floats once and keeps them in registers (the j loop is unrolled
// over the T slots behind a wave-uniform `j < t`), then walks the frequencies in chunks of kSpectrumChunk: load re and im of the
// chunk, apply the t captures in order, store.  No LDS, no atomics, no scratch; the tail of B is a bounds check on the lane.
//
//   WIDE   (B even; the engine decides) two nodes per lane: 8-byte loads from the stage, 16-byte loads and stores on the sums
//          (every plane of the stage and of the sums then starts on a 16-byte boundary: hipMalloc's alignment plus a multiple of
//          8 floats / 2 doubles)
//   !WIDE  one node per lane
//
// Traffic bound: B * (4 t + 32 K) bytes per fold.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "spectrum_plan.h"

namespace wv {

constexpr int kSpectrumChunk = 4;  // frequencies whose sums a lane holds at a time (tuned against the resource remarks: DESIGN.md 4.9)

// stage [T][B]: the first t slots hold captures; acc [K][2][B]; tw [t][K][2]: cos, sin of capture j at frequency k; nodes = B;
// t = staged captures to fold, 1 .. kSpectrumStage; n_freqs = K.  (Three __restrict__ kernel arguments, not members of a struct: the
// stores to acc must be known not to touch tw, or its loads cannot go through the scalar path.)
template <bool WIDE>
__global__ void __launch_bounds__(256) spectrum_fold_kernel(const float* __restrict__ stage, double* __restrict__ acc, const double* __restrict__ tw,
                                                            const uint64_t nodes, const int32_t t, const int32_t n_freqs) {
    constexpr int N = WIDE ? 2 : 1;  // nodes per lane
    typedef float FloatV2 __attribute__((ext_vector_type(2)));
    typedef double DoubleV2 __attribute__((ext_vector_type(2)));
    const uint64_t item = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t node = item * N;
    if (node >= nodes) return;  // (WIDE: B is even, so a lane has both its nodes or none)
    const int K = n_freqs;
    float p[kSpectrumStage][N];  // (as floats: half the registers; the conversion at each use is exact)
#pragma unroll
    for (int j = 0; j < kSpectrumStage; ++j) {
        if (j < t) {
            const float* src = stage + (uint64_t)j * nodes + node;
            if (WIDE) {
                const FloatV2 v = *reinterpret_cast<const FloatV2*>(src);
                p[j][0] = v.x;
                p[j][N - 1] = v.y;
            } else {
                p[j][0] = *src;
            }
        }
    }
    for (int k0 = 0; k0 < K; k0 += kSpectrumChunk) {
        double re[kSpectrumChunk][N], im[kSpectrumChunk][N];
#pragma unroll
        for (int kk = 0; kk < kSpectrumChunk; ++kk) {
            if (k0 + kk < K) {
                double* plane = acc + (uint64_t)(k0 + kk) * 2 * nodes + node;
                if (WIDE) {
                    const DoubleV2 r = *reinterpret_cast<const DoubleV2*>(plane);
                    const DoubleV2 i = *reinterpret_cast<const DoubleV2*>(plane + nodes);
                    re[kk][0] = r.x, re[kk][N - 1] = r.y;
                    im[kk][0] = i.x, im[kk][N - 1] = i.y;
                } else {
                    re[kk][0] = plane[0];
                    im[kk][0] = plane[nodes];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kSpectrumStage; ++j) {
            if (j < t) {
#pragma unroll
                for (int kk = 0; kk < kSpectrumChunk; ++kk) {
                    if (k0 + kk < K) {
                        const double* w = tw + ((int64_t)j * K + (k0 + kk)) * 2;  // (no lane in it)
                        const double c = w[0], s = w[1];
#pragma unroll
                        for (int n = 0; n < N; ++n) {
                            re[kk][n] = re[kk][n] + (double)p[j][n] * c;
                            im[kk][n] = im[kk][n] - (double)p[j][n] * s;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int kk = 0; kk < kSpectrumChunk; ++kk) {
            if (k0 + kk < K) {
                double* plane = acc + (uint64_t)(k0 + kk) * 2 * nodes + node;
                if (WIDE) {
                    *reinterpret_cast<DoubleV2*>(plane) = DoubleV2{re[kk][0], re[kk][N - 1]};
                    *reinterpret_cast<DoubleV2*>(plane + nodes) = DoubleV2{im[kk][0], im[kk][N - 1]};
                } else {
                    plane[0] = re[kk][0];
                    plane[nodes] = im[kk][0];
                }
            }
        }
    }
}

}  // namespace wv

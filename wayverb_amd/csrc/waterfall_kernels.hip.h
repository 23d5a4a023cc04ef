// waterfall_kernels.hip.h -- the fold kernel of waterfall maps (wv_set_waterfall; engine_waterfall.hip.h launches it).
//
// The captures themselves are snapshot_gather_kernel's (snapshot_kernels.hip.h), unchanged: each writes one dense float box of B
// nodes into a slot of the device-only stage float[T][B].  waterfall_fold_kernel<WIDE> folds the first t staged captures into the
// planar sums double acc[n_bins][K][2][B] (per time bin and frequency a re plane, then an im plane):
//
//     re[bin[j]][k] = re[bin[j]][k] + (double)p_j * c(j, k)        im[bin[j]][k] = im[bin[j]][k] - (double)p_j * s(j, k)        j = 0 .. t-1 in order
//
// a rounded product and a rounded sum each (-ffp-contract=off), so that a NumPy loop over the snapshots reproduces the sums bit for
// bit.  Which bin a staged capture goes to is the host's business (decay_plan.h: decay_bin): it writes int32 bin[t], non-decreasing.
// The twiddles tw[t][K][2] come from the host too (wv_spectrum_twiddle): the device evaluates no trigonometric function.  Both tables
// are reached through __restrict__ arguments with indices that depend on loop counters and kernel arguments only, never on the lane,
// so the compiler fetches them through the scalar path and every branch on them is wave-uniform.
//
// Lanes run along the dense node index.  A lane reads its t staged floats once (fold_parts.hip.h: stage_read), then walks the
// frequencies in chunks of kWaterfallChunk (spectrum_fold_kernel's registers).  Within a chunk it walks the captures in order holding
// ONE bin (decay_fold_kernel's form): when bin[j] differs from the bin it holds, it stores the chunk's re and im planes and loads the
// new bin's.  No LDS, no atomics, no scratch; the tail of B is a bounds check on the lane.
//
//   WIDE   (B even; the engine decides) two nodes per lane: 8-byte loads from the stage, 16-byte loads and stores on the sums
//          (every plane of the stage and of the sums then starts on a 16-byte boundary: hipMalloc's alignment plus a multiple of
//          8 floats / 2 doubles)
//   !WIDE  one node per lane
//
// Traffic model: B * (4 t + 32 K r') bytes per fold, r' the number of distinct bins among the t captures.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fold_parts.hip.h"
#include "waterfall_plan.h"

namespace wv {

constexpr int kWaterfallChunk = 4;  // frequencies whose sums a lane holds at a time (spectrum_kernels.hip.h: kSpectrumChunk)

// stage [T][B]: the first t slots hold captures; acc [n_bins][K][2][B]; bin [t]: the bin of staged capture j, each inside
// 0 .. n_bins - 1; tw [t][K][2]: cos, sin of capture j at frequency k; nodes = B; t = staged captures to fold, 1 .. kWaterfallStage;
// n_freqs = K.  (Four __restrict__ kernel arguments, not members of a struct: the stores to acc must be known not to touch either
// table, or their loads cannot go through the scalar path.)
template <bool WIDE>
__global__ void __launch_bounds__(256) waterfall_fold_kernel(const float* __restrict__ stage, double* __restrict__ acc, const int32_t* __restrict__ bin,
                                                             const double* __restrict__ tw, const uint64_t nodes, const int32_t t, const int32_t n_freqs) {
    constexpr int N = WIDE ? 2 : 1;  // nodes per lane
    const uint64_t node = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * N;
    if (node >= nodes || t < 1) return;  // (WIDE: B is even, so a lane has both its nodes or none)
    const int K = n_freqs;
    float p[kWaterfallStage][N];  // (as floats: half the registers; the conversion at each use is exact)
    stage_read(stage, nodes, node, t, p);
    for (int k0 = 0; k0 < K; k0 += kWaterfallChunk) {
        double re[kWaterfallChunk][N], im[kWaterfallChunk][N];
        int32_t held = bin[0];
#pragma unroll
        for (int kk = 0; kk < kWaterfallChunk; ++kk) {
            if (k0 + kk < K) {
                const double* plane = acc + ((uint64_t)held * K + (k0 + kk)) * 2 * nodes + node;
                plane_load<N, FoldDouble2>(plane, re[kk]);
                plane_load<N, FoldDouble2>(plane + nodes, im[kk]);
            }
        }
#pragma unroll
        for (int j = 0; j < kWaterfallStage; ++j) {
            if (j < t) {
                const int32_t b = bin[j];  // (no lane in it)
                if (b != held) {
#pragma unroll
                    for (int kk = 0; kk < kWaterfallChunk; ++kk) {
                        if (k0 + kk < K) {
                            double* plane = acc + ((uint64_t)held * K + (k0 + kk)) * 2 * nodes + node;
                            plane_store<N, FoldDouble2>(plane, re[kk]);
                            plane_store<N, FoldDouble2>(plane + nodes, im[kk]);
                        }
                    }
                    held = b;
#pragma unroll
                    for (int kk = 0; kk < kWaterfallChunk; ++kk) {
                        if (k0 + kk < K) {
                            const double* plane = acc + ((uint64_t)held * K + (k0 + kk)) * 2 * nodes + node;
                            plane_load<N, FoldDouble2>(plane, re[kk]);
                            plane_load<N, FoldDouble2>(plane + nodes, im[kk]);
                        }
                    }
                }
#pragma unroll
                for (int kk = 0; kk < kWaterfallChunk; ++kk) {
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
        for (int kk = 0; kk < kWaterfallChunk; ++kk) {
            if (k0 + kk < K) {
                double* plane = acc + ((uint64_t)held * K + (k0 + kk)) * 2 * nodes + node;
                plane_store<N, FoldDouble2>(plane, re[kk]);
                plane_store<N, FoldDouble2>(plane + nodes, im[kk]);
            }
        }
    }
}

}  // namespace wv

// decay_kernels.hip.h -- the fold kernel of energy decay maps (wv_set_decay; engine_decay.hip.h launches it).
//
// The captures themselves are snapshot_gather_kernel's (snapshot_kernels.hip.h), unchanged: each writes one dense float box of B
// nodes into a slot of the device-only stage float[T][B].  decay_fold_kernel<WIDE> folds the first t staged captures into the
// time-binned energies double bins[n_bins][B]:
//
//     E[bin[j]] = E[bin[j]] + (double)p_j * (double)p_j        j = 0 .. t-1 in order
//
// The product of two converted floats is exact in double (48 significant bits at the most), so the sum's rounding is the only one per
// capture and a NumPy loop over the snapshots reproduces the bins bit for bit.  Which bin a staged capture goes to is the host's
// business (decay_plan.h: decay_bin): it writes int32 bin[t], non-decreasing, and the kernel reaches the table through a __restrict__
// argument with indices that depend on the unrolled loop counter only, never on the lane, so the compiler fetches it through the
// scalar path and every branch on it is wave-uniform.
//
// Lanes run along the dense node index.  A lane reads its t staged floats once (fold_parts.hip.h: stage_read), then walks the captures
// in order with ONE accumulator: when bin[j] differs from the bin it holds, it stores the sum and loads the new bin's.  The tail of B
// is a bounds check on the lane.
//
//   WIDE   (B even; the engine decides) two nodes per lane: 8-byte loads from the stage, 16-byte loads and stores on the bins
//          (every plane of the stage and of the bins then starts on a 16-byte boundary: hipMalloc's alignment plus a multiple of
//          8 floats / 2 doubles)
//   !WIDE  one node per lane
//
// Traffic model: B * (4 t + 16 r) bytes per fold, r the number of distinct bins among the t captures.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "decay_plan.h"
#include "fold_parts.hip.h"

namespace wv {

// stage [T][B]: the first t slots hold captures; bins [n_bins][B]; bin [t]: the bin of staged capture j, each inside 0 .. n_bins - 1;
// nodes = B; t = staged captures to fold, 1 .. kDecayStage.  (Three __restrict__ kernel arguments, not members of a struct: the stores
// to bins must be known not to touch the table, or its loads cannot go through the scalar path.)
template <bool WIDE>
__global__ void __launch_bounds__(256) decay_fold_kernel(const float* __restrict__ stage, double* __restrict__ bins, const int32_t* __restrict__ bin,
                                                         const uint64_t nodes, const int32_t t) {
    constexpr int N = WIDE ? 2 : 1;  // nodes per lane
    const uint64_t node = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * N;
    if (node >= nodes || t < 1) return;  // (WIDE: B is even, so a lane has both its nodes or none)
    float p[kDecayStage][N];
    stage_read(stage, nodes, node, t, p);
    int32_t held = bin[0];
    double e[N];
    plane_load<N, FoldDouble2>(bins + (uint64_t)held * nodes + node, e);
#pragma unroll
    for (int j = 0; j < kDecayStage; ++j) {
        if (j < t) {
            const int32_t b = bin[j];  // (no lane in it)
            if (b != held) {
                plane_store<N, FoldDouble2>(bins + (uint64_t)held * nodes + node, e);
                held = b;
                plane_load<N, FoldDouble2>(bins + (uint64_t)held * nodes + node, e);
            }
#pragma unroll
            for (int n = 0; n < N; ++n) e[n] = e[n] + (double)p[j][n] * (double)p[j][n];
        }
    }
    plane_store<N, FoldDouble2>(bins + (uint64_t)held * nodes + node, e);
}

}  // namespace wv

// decay_bands_kernels.hip.h -- the fold kernel of band-limited energy decay maps (wv_set_decay_bands; engine_decay.hip.h launches it).
//
// decay_fold_kernel's sibling (decay_kernels.hip.h): the same stage float[T][B] filled by snapshot_gather_kernel, the same host-made
// table int32 bin[t], but between the capture and the square every node runs the capture through a cascade of S biquad sections per
// band, transposed direct form II, all doubles, every product and sum rounded on its own (the build's -ffp-contract=off):
//
//     x = (double)p_j
//     for s = 0 .. S-1:   out = x * b0 + z1;   z1 = (x * b1 - a1 * out) + z2;   z2 = x * b2 - a2 * out;   x = out
//     E[band][bin[j]] = E[band][bin[j]] + x * x                                 j = 0 .. t-1 in order
//
// Lanes run along the dense node index; blockIdx.y is the band.  Everything that depends on the band is therefore wave-uniform: the
// 5 S coefficients and the plane offsets into state and bins.  Coefficients and the bin table are reached through __restrict__
// arguments with indices that hold no lane, so the compiler fetches them through the scalar path and they live in SGPRs.
//
//   state  double[n_bands][S][2][B]       z1, z2 of every section, planar: a wave reads and writes 512 contiguous bytes per plane
//   bins   double[n_bands][n_bins][B]     planar, as the plain plan's
//
// A lane reads its t staged floats once (fold_parts.hip.h: stage_read), loads its 2 S state doubles,
// walks the captures in order through the sections with ONE bin accumulator (store and reload when bin[j] changes), and stores the
// state and the held bin.  S is a template parameter and the section loop is unrolled, so the state stays in registers.  No LDS, no
// atomics, no scratch; the tail of B is a bounds check on the lane.  One node per lane: with up to 8 bands the grid is already 8 times
// the plain fold's, and the per-lane work is a dependent chain of 9 S + 2 double operations per capture, not bytes.
//
// Traffic model: B * n_bands * (4 t + 32 S + 16 r) bytes per fold, r the distinct bins among the t captures; the
// n_bands - 1 re-reads of the stage are expected from L2.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fold_parts.hip.h"
#include "decay_plan.h"

namespace wv {

// stage [T][B]: the first t slots hold captures; state [n_bands][S][2][B]; bins [n_bands][n_bins][B]; coef [n_bands][S][5]: b0 b1 b2
// a1 a2; bin [t]: the bin of staged capture j, each inside 0 .. n_bins - 1; nodes = B; t = staged captures to fold, 1 .. kDecayStage.
// gridDim.y = n_bands.
template <int S>
__global__ void __launch_bounds__(256) decay_bands_fold_kernel(const float* __restrict__ stage, double* __restrict__ state, double* __restrict__ bins,
                                                               const double* __restrict__ coef, const int32_t* __restrict__ bin, const uint64_t nodes,
                                                               const uint32_t n_bins, const int32_t t) {
    static_assert(S >= 1 && S <= kDecayMaxSections, "1 .. 4 sections");
    const uint64_t node = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (node >= nodes || t < 1) return;
    const uint32_t band = blockIdx.y;
    float p[kDecayStage][1];
    stage_read(stage, nodes, node, t, p);
    const double* c = coef + (uint64_t)band * (S * 5);
    double b0[S], b1[S], b2[S], a1[S], a2[S];
#pragma unroll
    for (int s = 0; s < S; ++s) b0[s] = c[5 * s], b1[s] = c[5 * s + 1], b2[s] = c[5 * s + 2], a1[s] = c[5 * s + 3], a2[s] = c[5 * s + 4];
    double* zs = state + (uint64_t)band * (S * 2) * nodes + node;
    double z1[S], z2[S];
#pragma unroll
    for (int s = 0; s < S; ++s) z1[s] = zs[(uint64_t)(2 * s) * nodes], z2[s] = zs[(uint64_t)(2 * s + 1) * nodes];
    double* planes = bins + (uint64_t)band * n_bins * nodes + node;
    int32_t held = bin[0];
    double e = planes[(uint64_t)held * nodes];
#pragma unroll
    for (int j = 0; j < kDecayStage; ++j) {
        if (j < t) {
            const int32_t b = bin[j];  // (no lane in it)
            if (b != held) {
                planes[(uint64_t)held * nodes] = e;
                held = b;
                e = planes[(uint64_t)held * nodes];
            }
            double x = (double)p[j][0];
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const double out = x * b0[s] + z1[s];
                z1[s] = (x * b1[s] - a1[s] * out) + z2[s];
                z2[s] = x * b2[s] - a2[s] * out;
                x = out;
            }
            e = e + x * x;
        }
    }
    planes[(uint64_t)held * nodes] = e;
#pragma unroll
    for (int s = 0; s < S; ++s) zs[(uint64_t)(2 * s) * nodes] = z1[s], zs[(uint64_t)(2 * s + 1) * nodes] = z2[s];
}

}  // namespace wv

// modulation_kernels.hip.h -- the fold kernel of modulation maps (wv_set_modulation; engine_modulation.hip.h launches it).
//
// decay_bands_fold_kernel's cascade (decay_bands_kernels.hip.h) ahead of spectrum_fold_kernel's running Fourier sum
// (spectrum_kernels.hip.h), in one launch: the same stage float[T][B] filled by snapshot_gather_kernel, the same host-made twiddles
// (wv_spectrum_twiddle), but what is transformed is the band-filtered, SQUARED capture.  Per node and band, all doubles, every product
// and sum rounded on its own (the build's -ffp-contract=off):
//
//     x = (double)p_j
//     for s = 0 .. S-1:   out = x * b0 + z1;   z1 = (x * b1 - a1 * out) + z2;   z2 = x * b2 - a2 * out;   x = out
//     e = x * x;   E = E + e
//     Re[m] = Re[m] + e * c(j, m);   Im[m] = Im[m] - e * s(j, m)                m = 0 .. M-1          j = 0 .. t-1 in order
//
// Lanes run along the dense node index; blockIdx.y is the band.  Everything that depends on the band or the frequency is therefore
// wave-uniform: the 5 S coefficients, the twiddles tw[t][M][2] and the plane offsets into state and sums.  They are reached through
// __restrict__ arguments with indices that hold no lane, so the compiler fetches them through the scalar path and they live in SGPRs.
// The device evaluates no trigonometric function.
//
//   state  double[n_bands][S][2][B]          z1, z2 of every section, planar: a wave reads and writes 512 contiguous bytes per plane
//   sums   double[n_bands][1 + 2 M][B]       E, then Re, Im per frequency, planar
//
// A lane reads its t staged floats once (fold_parts.hip.h: stage_read, as doubles), loads its 2 S state doubles and
// runs the cascade over the captures in order; e_j takes p_j's place in registers, E is added and E and the state are stored.  Then
// it walks the frequencies in chunks of kModulationChunk, as spectrum_fold_kernel does: load Re and Im of the chunk, apply the t values
// of e in order, store.  S is a template parameter and the section loop is unrolled, so the state stays in registers.  No LDS, no
// atomics, no scratch; the tail of B is a bounds check on the lane.  One node per lane: with up to 8 bands the grid is already 8 times
// a plain fold's, and the 16 doubles of e are twice the registers the floats took (profiles/r16/modulation_kernel_resources.txt).
//
// Traffic model: B * n_bands * (4 t + 32 S + 16 + 32 M) bytes per fold; the n_bands - 1 re-reads of the stage are
// expected from L2.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fold_parts.hip.h"
#include "modulation_plan.h"

namespace wv {

constexpr int kModulationChunk = 4;  // frequencies whose sums a lane holds at a time (against the resource remarks: DESIGN.md 4.16)

// stage [T][B]: the first t slots hold captures; state [n_bands][S][2][B]; sums [n_bands][1 + 2 M][B]; coef [n_bands][S][5]: b0 b1 b2
// a1 a2; tw [t][M][2]: cos, sin of capture j at frequency m; nodes = B; n_freqs = M; t = staged captures to fold, 1 .. kModulationStage.
// gridDim.y = n_bands.  (Five __restrict__ kernel arguments, not members of a struct: the stores to state and sums must be known not to
// touch coef and tw, or their loads cannot go through the scalar path.)
template <int S>
__global__ void __launch_bounds__(256) modulation_fold_kernel(const float* __restrict__ stage, double* __restrict__ state, double* __restrict__ sums,
                                                              const double* __restrict__ coef, const double* __restrict__ tw, const uint64_t nodes,
                                                              const int32_t n_freqs, const int32_t t) {
    static_assert(S >= 1 && S <= kModulationMaxSections, "1 .. 4 sections");
    const uint64_t node = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (node >= nodes || t < 1) return;
    const uint32_t band = blockIdx.y;
    const int M = n_freqs;
    double e[kModulationStage][1];  // the captures, then their filtered squares
    stage_read(stage, nodes, node, t, e);
    const double* c = coef + (uint64_t)band * (S * 5);
    double b0[S], b1[S], b2[S], a1[S], a2[S];
#pragma unroll
    for (int s = 0; s < S; ++s) b0[s] = c[5 * s], b1[s] = c[5 * s + 1], b2[s] = c[5 * s + 2], a1[s] = c[5 * s + 3], a2[s] = c[5 * s + 4];
    double* zs = state + (uint64_t)band * (S * 2) * nodes + node;
    double z1[S], z2[S];
#pragma unroll
    for (int s = 0; s < S; ++s) z1[s] = zs[(uint64_t)(2 * s) * nodes], z2[s] = zs[(uint64_t)(2 * s + 1) * nodes];
    double* planes = sums + (uint64_t)band * (uint64_t)(1 + 2 * M) * nodes + node;  // E; Re[m] at 1 + 2 m, Im[m] behind it
    double energy = planes[0];
#pragma unroll
    for (int j = 0; j < kModulationStage; ++j) {
        if (j < t) {
            double x = e[j][0];
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const double out = x * b0[s] + z1[s];
                z1[s] = (x * b1[s] - a1[s] * out) + z2[s];
                z2[s] = x * b2[s] - a2[s] * out;
                x = out;
            }
            e[j][0] = x * x;
            energy = energy + e[j][0];
        }
    }
    planes[0] = energy;
#pragma unroll
    for (int s = 0; s < S; ++s) zs[(uint64_t)(2 * s) * nodes] = z1[s], zs[(uint64_t)(2 * s + 1) * nodes] = z2[s];
    for (int m0 = 0; m0 < M; m0 += kModulationChunk) {
        double re[kModulationChunk], im[kModulationChunk];
#pragma unroll
        for (int mm = 0; mm < kModulationChunk; ++mm) {
            if (m0 + mm < M) {
                const double* plane = planes + (uint64_t)(1 + 2 * (m0 + mm)) * nodes;
                re[mm] = plane[0];
                im[mm] = plane[nodes];
            }
        }
#pragma unroll
        for (int j = 0; j < kModulationStage; ++j) {
            if (j < t) {
#pragma unroll
                for (int mm = 0; mm < kModulationChunk; ++mm) {
                    if (m0 + mm < M) {
                        const double* w = tw + ((int64_t)j * M + (m0 + mm)) * 2;  // (no lane in it)
                        re[mm] = re[mm] + e[j][0] * w[0];
                        im[mm] = im[mm] - e[j][0] * w[1];
                    }
                }
            }
        }
#pragma unroll
        for (int mm = 0; mm < kModulationChunk; ++mm) {
            if (m0 + mm < M) {
                double* plane = planes + (uint64_t)(1 + 2 * (m0 + mm)) * nodes;
                plane[0] = re[mm];
                plane[nodes] = im[mm];
            }
        }
    }
}

}  // namespace wv

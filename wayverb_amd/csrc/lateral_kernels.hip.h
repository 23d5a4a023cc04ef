// lateral_kernels.hip.h -- the fold kernel of lateral maps (wv_set_lateral; engine_lateral.hip.h launches it).
//
// The captures themselves are intensity_gather_kernel's (intensity_kernels.hip.h), unchanged: each writes four dense float planes
// stage[slot][4][B] = pressure, gx, gy, gz.  lateral_fold_kernel folds the first t staged captures, which are captures number first,
// first + 1, ... since the plan was set, into the per-node state.  Per node and capture c, in capture order (include/wayverb_amd.h
// has the contract):
//
//     a = fabsf(pressure)
//     if (onset == NONE && a >= thr)   onset = c;
//     m = (double)g[i] * 0.5;  v[i] = v[i] - m / k                 i = x, y, z; EVERY capture: the integrator does not wait for the onset
//     p = (double)pressure
//     if (onset == NONE)  pre = pre + p * p;
//     else { rel = c - onset;  b = arrival_bin(rel);
//            E[b] = E[b] + p * p;  Ii[b] = Ii[b] + v[i] * p;  Qij[b] = Qij[b] + v[i] * v[j]; }     ij = xx, yy, zz, xy, xz, yz
//
// Every line rounds once (the library is built with -ffp-contract=off), so a NumPy loop over the snapshots of the box's hull
// (wayverb_amd/lateral.py: lateral_fold) reproduces all of it bit for bit.  This is arrival_fold_kernel's handling of the onset and
// of a bin that differs from lane to lane (arrival_kernels.hip.h), around intensity_fold_kernel's integrator:
//   - lanes run along the dense node index; all planes are planar, so every access of a wave is contiguous in whichever plane it is
//     in.  No LDS, no atomics, no scratch; the tail of B is a bounds check on the lane
//   - the edge table and `first` are kernel ARGUMENTS (the table by value, in arrival_fold_kernel's type: arrival_bin walks all of its
//     entries' places, so the ones behind the plan's eight exist); every index into the table is a loop counter, so it stays in scalar
//     registers and nothing is indexed by a lane's value
//   - rel only grows, so a lane's bin never decreases: TEN held accumulators, stored and reloaded only when the lane's bin changes
//   - state that cannot have changed is not touched: before its onset a node touches no bin, behind it `pre` is final
//
// Traffic model (lateral_plan.h: lateral_fold_traffic): B * (16 t + 52 + 160 r) bytes per fold, + 4 B with a map.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "arrival_kernels.hip.h"
#include "fold_parts.hip.h"
#include "lateral_plan.h"

namespace wv {

// stage [T][4][B]: the first t slots hold captures first .. first + t - 1; pre [B]; velocity [3][B]; bins [10][n_bins][B]; onset [B];
// threshold_map [B] or NULL (then `threshold` for every node); edges: the plan's n_bins entries first; nodes = B; k = ambient_density *
// sample_rate; t = staged captures to fold, 1 .. kLateralStage; first + t <= 2^32 - 1.  (Every pointer a __restrict__ kernel
// argument: the stores must be known not to touch what is read later.)
__global__ void __launch_bounds__(256)
    lateral_fold_kernel(const float* __restrict__ stage, double* __restrict__ pre, double* __restrict__ velocity, double* __restrict__ bins,
                        uint32_t* __restrict__ onset, const float* __restrict__ threshold_map, const float threshold, const ArrivalEdges edges,
                        const uint32_t n_bins, const uint32_t first, const uint64_t nodes, const double k, const int32_t t) {
    const uint64_t node = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (node >= nodes || t < 1) return;
    const float thr = threshold_map ? threshold_map[node] : threshold;
    const uint32_t onset_was = onset[node];
    uint32_t on = onset_was;
    double pr = onset_was == kLateralNone ? pre[node] : 0.0;  // (final behind the onset: not touched again)
    double v[3], e[kLateralPlanes];
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] = velocity[(uint64_t)a * nodes + node];
#pragma unroll
    for (int a = 0; a < (int)kLateralPlanes; ++a) e[a] = 0.0;
    auto load = [&](uint32_t b) {
#pragma unroll
        for (int a = 0; a < (int)kLateralPlanes; ++a) e[a] = bins[((uint64_t)a * n_bins + (uint64_t)b) * nodes + node];
    };
    auto store = [&](uint32_t b) {
#pragma unroll
        for (int a = 0; a < (int)kLateralPlanes; ++a) bins[((uint64_t)a * n_bins + (uint64_t)b) * nodes + node] = e[a];
    };
    uint32_t held = kLateralNone;  // the bin whose sums `e` holds; none yet
#pragma unroll
    for (int j = 0; j < kLateralStage; ++j) {
        if (j < t) {
            const float* src = stage + (uint64_t)j * 4u * nodes + node;
            const float pressure = src[0];
            const float g[3] = {src[nodes], src[2 * nodes], src[3 * nodes]};
            const uint32_t c = first + (uint32_t)j;  // (no lane in it)
            const float a = __builtin_fabsf(pressure);
            on = onset_update(on, a, thr, c, kLateralNone);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                v[i] = integrate(v[i], g[i], k);
            }
            const double p = (double)pressure;
            if (on == kLateralNone) {
                pr = pr + p * p;
            } else {
                const uint32_t rel = c - on;
                const uint32_t b = arrival_bin(rel, edges.e, n_bins);
                if (b != held) {
                    if (held != kLateralNone) store(held);
                    held = b;
                    load(held);
                }
                e[0] = e[0] + p * p;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    e[1 + i] = e[1 + i] + v[i] * p;
                    e[4 + i] = e[4 + i] + v[i] * v[i];
                }
                e[7] = e[7] + v[0] * v[1];
                e[8] = e[8] + v[0] * v[2];
                e[9] = e[9] + v[1] * v[2];
            }
        }
    }
    if (held != kLateralNone) store(held);
    if (on != onset_was) onset[node] = on;
    if (onset_was == kLateralNone) pre[node] = pr;
#pragma unroll
    for (int a = 0; a < 3; ++a) velocity[(uint64_t)a * nodes + node] = v[a];
}

}  // namespace wv

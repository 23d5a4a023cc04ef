// arrival_kernels.hip.h -- the fold kernel of arrival-aligned energy maps (wv_set_arrival; engine_arrival.hip.h launches it).
//
// The captures themselves are snapshot_gather_kernel's (snapshot_kernels.hip.h), unchanged: each writes one dense float box of B
// nodes into a slot of the device-only stage float[T][B].  arrival_fold_kernel folds the first t staged captures, which are captures
// number first, first + 1, ... since the plan was set, into the per-node state.  Per node and capture c, in capture order
// (include/wayverb_amd.h has the contract):
//
//     a  = fabsf(p_c)
//     if (a > peak)                    { peak = a; peak_capture = c; }
//     if (onset == NONE && a >= thr)   onset = c;
//     sq = (double)p_c * (double)p_c
//     if (onset == NONE)  pre = pre + sq;
//     else { rel = c - onset;  k = arrival_bin(rel);  E[k] = E[k] + sq;  M = M + (double)rel * sq; }
//
// The product of two converted floats is exact in double, so every line rounds once and a NumPy loop over the snapshots
// (wayverb_amd/arrival.py: arrival_fold) reproduces all of it bit for bit.  This is decay_fold_kernel's fold with a bin that differs
// from lane to lane:
//   - lanes run along the dense node index; a lane reads its t staged floats once (fold_parts.hip.h: stage_read; the onset rule is
//     its onset_update), loads its state, walks the captures in order and stores what changed; the tail of B is a bounds check on the lane
//   - the edge table and `first` are kernel ARGUMENTS (the table by value): they live in the kernel argument segment, every index into
//     the table is a loop counter (arrival_plan.h: arrival_bin counts the edges at or below rel), so the compiler fetches them through
//     the scalar path and keeps them in scalar registers; nothing is indexed by a lane's value, so nothing goes to scratch
//   - rel only grows, so a lane's bin never decreases: ONE held accumulator, stored and reloaded when the lane's bin changes.  The
//     branch is divergent and so is the plane the access goes to, but consecutive lanes still touch consecutive doubles of whichever
//     plane they are in: a wave whose lanes sit in r different bins touches r runs of its 512 bytes, not 64 scattered ones
//   - state that cannot have changed is neither loaded nor stored: before its onset a node has M = +0.0 and no bin, behind it `pre`
//     is final.  Steady state: 20 B read and 8 B written per node and fold beside the bins
//
// Traffic model (arrival_plan.h: arrival_fold_traffic): B * (4 t + 28 + 16 r) bytes per fold, + 4 B with a threshold map.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "arrival_plan.h"
#include "fold_parts.hip.h"

namespace wv {

struct ArrivalEdges {
    uint32_t e[kArrivalMaxBins];  // wv_arrival_plan::edges, as it lies
};

// stage [T][B]: the first t slots hold captures first .. first + t - 1; pre, moment [B]; bins [n_bins][B]; onset, peak, peak_capture
// [B]; threshold_map [B] or NULL (then `threshold` for every node); nodes = B; t = staged captures to fold, 1 .. kArrivalStage;
// first + t <= 2^32 - 1.  (Every pointer a __restrict__ kernel argument: the stores must be known not to touch what is read later.)
__global__ void __launch_bounds__(256)
    arrival_fold_kernel(const float* __restrict__ stage, double* __restrict__ pre, double* __restrict__ moment, double* __restrict__ bins,
                        uint32_t* __restrict__ onset, float* __restrict__ peak, uint32_t* __restrict__ peak_capture,
                        const float* __restrict__ threshold_map, const float threshold, const ArrivalEdges edges, const uint32_t n_bins,
                        const uint32_t first, const uint64_t nodes, const int32_t t) {
    const uint64_t node = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (node >= nodes || t < 1) return;
    float p[kArrivalStage][1];
    stage_read(stage, nodes, node, t, p);
    const float thr = threshold_map ? threshold_map[node] : threshold;
    const uint32_t onset_was = onset[node];
    const uint32_t peak_capture_was = peak_capture[node];
    uint32_t on = onset_was, pc = peak_capture_was;
    float pk = peak[node];
    double pr = onset_was == kArrivalNone ? pre[node] : 0.0;     // (final behind the onset: not touched again)
    double mo = onset_was == kArrivalNone ? 0.0 : moment[node];  // (+0.0 before the onset: nothing has been added)
    uint32_t held = kArrivalNone;                                // the bin whose sum `e` holds; none yet
    double e = 0.0;
#pragma unroll
    for (int j = 0; j < kArrivalStage; ++j) {
        if (j < t) {
            const uint32_t c = first + (uint32_t)j;  // (no lane in it)
            const float a = __builtin_fabsf(p[j][0]);
            if (a > pk) {  // strict: the first occurrence; false for a NaN
                pk = a;
                pc = c;
            }
            on = onset_update(on, a, thr, c, kArrivalNone);
            const double sq = (double)p[j][0] * (double)p[j][0];
            if (on == kArrivalNone) {
                pr = pr + sq;
            } else {
                const uint32_t rel = c - on;
                const uint32_t k = arrival_bin(rel, edges.e, n_bins);
                if (k != held) {
                    if (held != kArrivalNone) bins[(uint64_t)held * nodes + node] = e;
                    held = k;
                    e = bins[(uint64_t)held * nodes + node];
                }
                e = e + sq;
                mo = mo + (double)rel * sq;
            }
        }
    }
    if (held != kArrivalNone) bins[(uint64_t)held * nodes + node] = e;
    if (on != onset_was) onset[node] = on;
    if (pc != peak_capture_was) {
        peak[node] = pk;
        peak_capture[node] = pc;
    }
    if (onset_was == kArrivalNone) pre[node] = pr;
    if (on != kArrivalNone) moment[node] = mo;
}

}  // namespace wv

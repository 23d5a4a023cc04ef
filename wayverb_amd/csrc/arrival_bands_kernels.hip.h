// arrival_bands_kernels.hip.h -- the fold kernel of band-limited arrival maps (wv_set_arrival_bands; engine_arrival_bands.hip.h
// launches it).
//
// arrival_fold_kernel (arrival_kernels.hip.h) with decay_bands_fold_kernel's cascade (decay_bands_kernels.hip.h) ahead of the square:
// the same stage float[T][B] filled by snapshot_gather_kernel; the first t staged captures are captures number first, first + 1, ...
// since the plan was set.  Per node, per band k and per capture c, in capture order (include/wayverb_amd.h has the contract):
//
//     a  = fabsf(p_c);  if (a > peak) { peak = a; peak_capture = c; }                                    (band 0's lanes only)
//     if (onset == NONE && a >= thr) onset = c;                                                          (the BROADBAND onset)
//     x = (double)p_c
//     for s = 0 .. S-1:   out = x * b0 + z1;   z1 = (x * b1 - a1 * out) + z2;   z2 = x * b2 - a2 * out;   x = out
//     sq = x * x
//     if (onset == NONE)  pre[k] = pre[k] + sq;
//     else { d = c - onset;  rel = d > lag[k] ? d - lag[k] : 0;  b = arrival_bands_bin(rel);
//            E[k][b] = E[k][b] + sq;  M[k] = M[k] + (double)rel * sq; }
//
// every product and sum rounded on its own (the build's -ffp-contract=off); wayverb_amd/arrival.py: banded_arrival_fold reproduces all
// outputs and the filter states bit for bit.
//   - lanes run along the dense node index, blockIdx.y is the band: coefficients, the lag and the plane offsets are wave-uniform.
//     Coefficients come through a __restrict__ argument with lane-free indices, the edge table, the tail and the lags by value in
//     the kernel argument segment; every index into them is a loop counter, so they travel the scalar path and nothing is indexed by
//     a lane's value: no scratch
//   - THE ONSET IS KEPT ONCE PER BAND, uint32[K][B].  Every (node, band) lane needs the node's onset, and a fold changes it; with one
//     shared word band 0's store would race the other bands' loads of the same launch.  Each band's lane evolves its own copy from
//     the same p and thr, so all K copies are always equal and no lane reads what another lane of the launch writes.  (Bands looped
//     inside one lane instead would hold K cascades' state and K accumulators per lane, or walk the stage K times serially with an
//     eighth of the lanes: the grid row per band is what keeps the registers at the banded decay fold's.)  Only band 0's lanes touch
//     peak and peak_capture
//   - rel never decreases, so a lane's bin never does: ONE held accumulator, stored and reloaded when the lane's bin changes; state
//     that cannot have changed is neither loaded nor stored (before the onset M = +0.0 and there is no bin; behind it pre is final)
//   - neither the edges nor the tail cost a search or a division per capture.  rel grows by at most one per capture, so a lane keeps
//     its bin k and `next`, the rel at which it moves on to bin k + 1, and a capture costs one comparison.  Where a lane stands as
//     the fold begins is found ONCE, ahead of the capture loop, through the scalar path: arrival_bin's count over the edges in the
//     argument segment, or the fold's one division if the lane is in the tail.  (The edges held in scalar registers through the
//     unrolled loop, beside 10 S for the coefficients, spilled 10 S scalar registers.)  `next` comes from `bin_first` in MEMORY --
//     uint32[n_bins + 1], the first rel of every bin and NONE behind the last, written by the host when the plan is set
//     (arrival_bands_plan.h: arrival_bands_bin_first; 16 KB at the most) -- the one table indexed by a lane's value, which is why it is
//     in memory: one load per lane and fold, and one whenever the lane moves on
//
// Traffic model (arrival_bands_plan.h: arrival_bands_fold_traffic): B * K * (4 t + 32 S + 20 + 16 r) + 8 B bytes per fold.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "arrival_bands_plan.h"
#include "fold_parts.hip.h"

namespace wv {

// stage [T][B]: the first t slots hold captures first .. first + t - 1; state [K][S][2][B]; pre, moment [K][B]; bins [K][n_bins][B];
// onset [K][B]; peak, peak_capture [B]; threshold_map [B] or NULL (then `threshold` for every node); coef [K][S][5]: b0 b1 b2 a1 a2;
// bin_first [n_bins + 1] (arrival_bands_plan.h: arrival_bands_bin_first); nodes = B; t = staged captures to fold,
// 1 .. kArrivalBandsStage; first + t <= 2^32 - 1.  gridDim.y = K.
template <int S>
__global__ void __launch_bounds__(256)
    arrival_bands_fold_kernel(const float* __restrict__ stage, double* __restrict__ state, double* __restrict__ pre, double* __restrict__ moment,
                              double* __restrict__ bins, uint32_t* __restrict__ onset, float* __restrict__ peak, uint32_t* __restrict__ peak_capture,
                              const float* __restrict__ threshold_map, const float threshold, const double* __restrict__ coef,
                              const uint32_t* __restrict__ bin_first, const ArrivalBandsTable table, const uint32_t first, const uint64_t nodes,
                              const int32_t t) {
    static_assert(S >= 1 && S <= kDecayMaxSections, "1 .. 4 sections");
    const uint64_t node = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (node >= nodes || t < 1) return;
    const uint32_t band = blockIdx.y;
    const bool first_band = band == 0;  // (its lanes keep the node's peak)
    uint32_t lag = 0;
#pragma unroll
    for (uint32_t m = 0; m < kArrivalBandsMaxBands; ++m)
        if (m == band) lag = table.lag[m];  // (no lane in it)
    const uint32_t n_bins = table.n_edges + table.n_tail;
    const uint64_t plane = (uint64_t)band * nodes + node;  // the lane's place in a [K][B] array
    const uint32_t onset_was = onset[plane];
    // where the lane stands: its bin k and `next`, the rel at which it moves on (NONE: never).  Before its onset: bin 0
    uint32_t k = 0;
    if (onset_was != kArrivalNone) k = arrival_bands_bin(arrival_bands_rel(first - onset_was, lag), table);  // (the tail's division is this one)
    uint32_t next = bin_first[k + 1];
    float p[kArrivalBandsStage][1];
    stage_read(stage, nodes, node, t, p);
    const double* c5 = coef + (uint64_t)band * (S * 5);
    double b0[S], b1[S], b2[S], a1[S], a2[S];
#pragma unroll
    for (int s = 0; s < S; ++s) b0[s] = c5[5 * s], b1[s] = c5[5 * s + 1], b2[s] = c5[5 * s + 2], a1[s] = c5[5 * s + 3], a2[s] = c5[5 * s + 4];
    double* zs = state + (uint64_t)band * (S * 2) * nodes + node;
    double z1[S], z2[S];
#pragma unroll
    for (int s = 0; s < S; ++s) z1[s] = zs[(uint64_t)(2 * s) * nodes], z2[s] = zs[(uint64_t)(2 * s + 1) * nodes];
    double* planes = bins + (uint64_t)band * n_bins * nodes + node;
    const float thr = threshold_map ? threshold_map[node] : threshold;
    uint32_t on = onset_was;
    uint32_t peak_capture_was = kArrivalNone, pc = kArrivalNone;
    float pk = __builtin_inff();  // (another band's lane: no magnitude is above it)
    if (first_band) {
        peak_capture_was = pc = peak_capture[node];
        pk = peak[node];
    }
    double pr = onset_was == kArrivalNone ? pre[plane] : 0.0;     // (final behind the onset: not touched again)
    double mo = onset_was == kArrivalNone ? 0.0 : moment[plane];  // (+0.0 before the onset: nothing has been added)
    bool held = false;  // `e` holds bin k's sum
    double e = 0.0;
#pragma unroll
    for (int j = 0; j < kArrivalBandsStage; ++j) {
        if (j < t) {
            const uint32_t c = first + (uint32_t)j;  // (no lane in it)
            const float a = __builtin_fabsf(p[j][0]);
            if (a > pk) {  // strict: the first occurrence; false for a NaN
                pk = a;
                pc = c;
            }
            on = onset_update(on, a, thr, c, kArrivalNone);
            double x = (double)p[j][0];
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const double out = x * b0[s] + z1[s];
                z1[s] = (x * b1[s] - a1[s] * out) + z2[s];
                z2[s] = x * b2[s] - a2[s] * out;
                x = out;
            }
            const double sq = x * x;
            if (on == kArrivalNone) {
                pr = pr + sq;
            } else {
                const uint32_t rel = arrival_bands_rel(c - on, lag);
                if (!held) {
                    held = true;
                    e = planes[(uint64_t)k * nodes];
                } else if (rel >= next) {  // rel == next: this capture is the first of bin k + 1
                    planes[(uint64_t)k * nodes] = e;
                    ++k;
                    next = bin_first[k + 1];
                    e = planes[(uint64_t)k * nodes];
                }
                e = e + sq;
                mo = mo + (double)rel * sq;
            }
        }
    }
    if (held) planes[(uint64_t)k * nodes] = e;
    if (on != onset_was) onset[plane] = on;
    if (pc != peak_capture_was) {
        peak[node] = pk;
        peak_capture[node] = pc;
    }
    if (onset_was == kArrivalNone) pre[plane] = pr;
    if (on != kArrivalNone) moment[plane] = mo;
#pragma unroll
    for (int s = 0; s < S; ++s) zs[(uint64_t)(2 * s) * nodes] = z1[s], zs[(uint64_t)(2 * s + 1) * nodes] = z2[s];
}

}  // namespace wv

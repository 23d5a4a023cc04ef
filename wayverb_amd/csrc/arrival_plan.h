// arrival_plan.h -- (host only, no HIP, nothing but the standard library) the integer logic of arrival-aligned energy maps
// (wv_set_arrival, include/wayverb_amd.h) that is the plan's own: which edge tables are refused, the bin of a capture counted from a
// node's own onset, and the sizes and places of everything that is allocated for a plan.  The stage -- 16 slots, free slots, when a
// fold is due, the good captures after a stop -- is spectrum_plan.h's (capture_stage.h holds its bookkeeping for every plan that
// folds on the device); which steps are plan steps and whether a box lies inside the mesh is snapshot_plan.h's.
// arrival_bin is constexpr so that arrival_fold_kernel (arrival_kernels.hip.h) evaluates THIS text on the device: the rule exists once.
// tests/cpp/arrival_plan_test.cpp covers this file on the CPU.
#pragma once
#include <cmath>
#include <cstdint>

#include "decay_plan.h"

namespace wv {

constexpr int kArrivalStage = kDecayStage;        // T: captures the stage holds
constexpr uint32_t kArrivalMaxBins = 16;          // n_bins at the most (wv_arrival_plan::edges has that many entries)
constexpr uint32_t kArrivalNone = 0xFFFFFFFFu;    // "no onset yet" / "no peak yet": no capture has this number
constexpr uint64_t kArrivalMaxCaptures = kArrivalNone;  // captures 0 .. 2^32 - 2 can be counted; the engine refuses the next one

// edges[0] == 0 < edges[1] < ... < edges[n_bins - 1], 1 <= n_bins <= 16 (entries behind n_bins are not looked at)
inline bool arrival_edges_valid(const uint32_t* edges, uint32_t n_bins) {
    if (!edges || n_bins < 1 || n_bins > kArrivalMaxBins || edges[0] != 0) return false;
    for (uint32_t k = 1; k < n_bins; ++k)
        if (edges[k] <= edges[k - 1]) return false;
    return true;
}

// >= 0 and finite (-0.0 counts as 0; NaN is refused)
inline bool arrival_threshold_valid(float thr) { return thr >= 0.0f && std::isfinite(thr); }

// The bin of a capture `rel` captures behind the node's onset: the largest k with edges[k] <= rel, the last bin open-ended.  Counted,
// not searched: every index depends on the loop counter only, so that on the device the table stays in scalar registers and nothing
// is indexed by a lane's value.  (n_bins = 0: bin 0; the engine refuses it.)
constexpr uint32_t arrival_bin(uint32_t rel, const uint32_t* edges, uint32_t n_bins) {
    uint32_t k = 0;
    for (uint32_t m = 1; m < kArrivalMaxBins; ++m)
        if (m < n_bins) k += edges[m] <= rel ? 1u : 0u;
    return k;
}

// Everything a fold reads AND writes per node lies in ONE allocation, the doubles first so that every part is aligned whatever B is:
//   double pre[B], moment[B], bins[n_bins][B]; uint32 onset[B]; float peak[B]; uint32 peak_capture[B]
// (a checkpoint is then one copy).  Offsets in bytes from its start; kDecayNoSize where the size leaves 64 bits.
inline uint64_t arrival_pre_offset() { return 0; }
inline uint64_t arrival_moment_offset(uint64_t nodes) { return decay_mul(nodes, sizeof(double)); }
inline uint64_t arrival_bins_offset(uint64_t nodes) { return decay_mul(nodes, 2 * sizeof(double)); }
inline uint64_t arrival_bins_bytes(uint64_t nodes, uint32_t n_bins) { return decay_mul(nodes, (uint64_t)n_bins * sizeof(double)); }
inline uint64_t arrival_onset_offset(uint64_t nodes, uint32_t n_bins) { return decay_mul(nodes, (2ull + n_bins) * sizeof(double)); }
inline uint64_t arrival_add(uint64_t a, uint64_t b) { return a == kDecayNoSize || b == kDecayNoSize || b > kDecayNoSize - 1 - a ? kDecayNoSize : a + b; }
inline uint64_t arrival_peak_offset(uint64_t nodes, uint32_t n_bins) { return arrival_add(arrival_onset_offset(nodes, n_bins), decay_mul(nodes, 4)); }
inline uint64_t arrival_peak_capture_offset(uint64_t nodes, uint32_t n_bins) { return arrival_add(arrival_onset_offset(nodes, n_bins), decay_mul(nodes, 8)); }
inline uint64_t arrival_state_bytes(uint64_t nodes, uint32_t n_bins) { return arrival_add(arrival_onset_offset(nodes, n_bins), decay_mul(nodes, 12)); }
// the stage float[T][B] and the optional threshold map float[B]
inline uint64_t arrival_stage_bytes(uint64_t nodes) { return decay_stage_bytes(nodes); }
inline uint64_t arrival_map_bytes(uint64_t nodes) { return decay_mul(nodes, sizeof(float)); }

// Bytes one fold of t staged captures moves per node, in the steady state where every node has its onset behind it:
// t floats read; onset, peak, peak_capture and the moment read (20 B), the moment written (8 B); r bins read and written; the
// threshold where a map gives it (4 B).  Before its onset a node reads and writes `pre` in the moment's place and touches no bin.
inline uint64_t arrival_fold_traffic(uint64_t nodes, uint32_t t, uint32_t r, bool map) {
    return decay_mul(nodes, 4ull * t + 28ull + 16ull * r + (map ? 4ull : 0ull));
}

}  // namespace wv

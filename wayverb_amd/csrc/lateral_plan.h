// lateral_plan.h -- (host only, no HIP, nothing but the standard library) the logic of lateral maps (wv_set_lateral,
// include/wayverb_amd.h) that is the plan's own: what a plan is refused for, and the sizes and places of everything that is
// allocated for one.  The capture is the intensity plan's (intensity_plan.h: the box, the refusal of a node on a mesh face, the
// stage float[T][4][B]); the bin of a capture counted from a node's own onset, which edge tables and thresholds are refused, are
// the arrival plan's (arrival_plan.h: arrival_bin, arrival_edges_valid, arrival_threshold_valid -- the rule exists once); the stage's
// bookkeeping is capture_stage.h's.
// tests/cpp/lateral_plan_test.cpp covers this file on the CPU.
#pragma once
#include <cstdint>

#include "arrival_plan.h"
#include "intensity_plan.h"

namespace wv {

constexpr int kLateralStage = kIntensityStage;       // T: captures the stage holds
constexpr uint32_t kLateralMaxBins = 8;              // n_bins at the most (wv_lateral_plan::edges has that many entries)
constexpr uint32_t kLateralPlanes = 10;              // per bin: E, Ix, Iy, Iz, Qxx, Qyy, Qzz, Qxy, Qxz, Qyz
constexpr uint32_t kLateralNone = kArrivalNone;      // "no onset yet"
constexpr uint64_t kLateralMaxCaptures = kArrivalMaxCaptures;

static_assert(kLateralMaxBins <= kArrivalMaxBins, "arrival_bin counts the edges of a lateral plan");

inline SnapshotBox lateral_box(const wv_lateral_plan& p) { return plan_box(p); }

// WV_OK, or WV_E_INVALID_ARGUMENT with *why (never NULL then) = what is wrong, in the order wv_set_arrival and wv_set_intensity
// check what they share with this plan
inline int lateral_plan_check(const wv_lateral_plan& p, int32_t mesh_nx, int32_t mesh_ny, int32_t mesh_nz, const char** why) {
    static const PlanSentences says = WV_PLAN_SENTENCES("wv_set_lateral");
    const char* dummy = nullptr;
    const char*& w = why ? *why : dummy;
    if (p.n_bins < 1 || p.n_bins > kLateralMaxBins) w = "wv_set_lateral: n_bins must be 1 .. 8";
    else if (!arrival_edges_valid(p.edges, p.n_bins)) w = "wv_set_lateral: edges[0] must be 0 and the edges strictly increasing";
    else if (!arrival_threshold_valid(p.threshold)) w = "wv_set_lateral: the threshold must be >= 0 and finite";
    else w = gradient_plan_refusal(p, mesh_nx, mesh_ny, mesh_nz, says, "wv_set_lateral: spacing, sample rate and ambient density must be positive and finite");
    return w ? WV_E_INVALID_ARGUMENT : WV_OK;
}

// Everything a fold reads AND writes per node lies in ONE allocation, the doubles first so that every part is aligned whatever B is:
//   double pre[B], velocity[3][B], bins[10][n_bins][B]; uint32 onset[B]
// (a checkpoint is then one copy).  Offsets in bytes from its start; kDecayNoSize where the size leaves 64 bits.
inline uint64_t lateral_pre_offset() { return 0; }
inline uint64_t lateral_velocity_offset(uint64_t nodes) { return decay_mul(nodes, sizeof(double)); }
inline uint64_t lateral_velocity_bytes(uint64_t nodes) { return decay_mul(nodes, 3 * sizeof(double)); }
inline uint64_t lateral_bins_offset(uint64_t nodes) { return decay_mul(nodes, 4 * sizeof(double)); }
inline uint64_t lateral_bins_bytes(uint64_t nodes, uint32_t n_bins) { return decay_mul(nodes, (uint64_t)kLateralPlanes * n_bins * sizeof(double)); }
inline uint64_t lateral_onset_offset(uint64_t nodes, uint32_t n_bins) { return decay_mul(nodes, (4ull + (uint64_t)kLateralPlanes * n_bins) * sizeof(double)); }
inline uint64_t lateral_state_bytes(uint64_t nodes, uint32_t n_bins) { return arrival_add(lateral_onset_offset(nodes, n_bins), decay_mul(nodes, 4)); }
// the stage float[T][4][B] (the intensity plan's) and the optional threshold map float[B]
inline uint64_t lateral_stage_bytes(uint64_t nodes) { return intensity_stage_bytes(nodes); }
inline uint64_t lateral_map_bytes(uint64_t nodes) { return decay_mul(nodes, sizeof(float)); }

// Bytes one fold of t staged captures moves per node, in the steady state where every node has its onset behind it:
// four floats per capture read; the onset read (4 B), three velocities read and written (48 B); ten sums read and written for each
// of the r bins the node passes through; the threshold where a map gives it (4 B).  Before its onset a node reads and writes `pre`
// beside that and touches no bin.
inline uint64_t lateral_fold_traffic(uint64_t nodes, uint32_t t, uint32_t r, bool map) {
    return decay_mul(nodes, 16ull * t + 52ull + 160ull * r + (map ? 4ull : 0ull));
}

}  // namespace wv

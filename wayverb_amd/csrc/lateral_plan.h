// lateral_plan.h -- (host only, no HIP, nothing but the standard library) the logic of lateral maps (wv_set_lateral,
// include/wayverb_amd.h) that is the plan's own: what a plan is refused for, and the sizes and places of everything that is
// allocated for one.  The capture is the intensity plan's (intensity_plan.h: the box, the refusal of a node on a mesh face, the
// stage float[T][4][B]); the bin of a capture counted from a node's own onset, which edge tables and thresholds are refused, are
// the arrival plan's (arrival_plan.h: arrival_bin, arrival_edges_valid, arrival_threshold_valid -- the rule exists once); the stage's
// bookkeeping is capture_stage.h's.
// tests/cpp/lateral_plan_test.cpp covers this file on the CPU.
#pragma once
#include <cmath>
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

inline SnapshotBox lateral_box(const wv_lateral_plan& p) {
    SnapshotBox b;
    b.x0 = p.x0, b.y0 = p.y0, b.z0 = p.z0;
    b.nx = p.nx, b.ny = p.ny, b.nz = p.nz;
    b.sx = p.sx, b.sy = p.sy, b.sz = p.sz;
    return b;
}

// WV_OK, or WV_E_INVALID_ARGUMENT with *why (never NULL then) = what is wrong, in the order wv_set_arrival and wv_set_intensity
// check what they share with this plan
inline int lateral_plan_check(const wv_lateral_plan& p, int32_t mesh_nx, int32_t mesh_ny, int32_t mesh_nz, const char** why) {
    const char* dummy = nullptr;
    const char*& w = why ? *why : dummy;
    w = nullptr;
    if (p.n_bins < 1 || p.n_bins > kLateralMaxBins) w = "wv_set_lateral: n_bins must be 1 .. 8";
    else if (!arrival_edges_valid(p.edges, p.n_bins)) w = "wv_set_lateral: edges[0] must be 0 and the edges strictly increasing";
    else if (!arrival_threshold_valid(p.threshold)) w = "wv_set_lateral: the threshold must be >= 0 and finite";
    else if (p.sx < 1 || p.sy < 1 || p.sz < 1) w = "wv_set_lateral: strides must be >= 1";
    else if (p.period < 1) w = "wv_set_lateral: period must be >= 1";
    else if (!(p.spacing > 0) || !(p.sample_rate > 0) || !(p.ambient_density > 0) || !std::isfinite(p.spacing) || !std::isfinite(p.sample_rate) ||
             !std::isfinite(p.ambient_density))
        w = "wv_set_lateral: spacing, sample rate and ambient density must be positive and finite";
    else if (!snapshot_box_valid(lateral_box(p), mesh_nx, mesh_ny, mesh_nz)) w = "wv_set_lateral: the box leaves the mesh";
    else if (!intensity_axis_inside(p.x0, p.nx, p.sx, mesh_nx) || !intensity_axis_inside(p.y0, p.ny, p.sy, mesh_ny) ||
             !intensity_axis_inside(p.z0, p.nz, p.sz, mesh_nz))
        w = kIntensityEdge;
    // (the capture kernel indexes a dense plane with 32 bits)
    else if ((uint64_t)p.nx * (uint64_t)p.ny >= (1ull << 31)) w = "wv_set_lateral: more than 2^31 nodes per plane of the box";
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

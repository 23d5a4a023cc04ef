// interaural_plan.h -- (host only, no HIP, nothing but the standard library) the logic of interaural maps (wv_set_interaural,
// include/wayverb_amd.h) that is the plan's own: what a plan is refused for and in which order, the lag class its fold kernel is
// built for, the sizes and places of everything that is allocated for a plan, the slot of a capture in the lag history, and the
// traffic model of a fold.  The bin of a capture counted from a node's own onset, which edge tables and thresholds are refused, are
// the arrival plan's (arrival_plan.h: arrival_bin, arrival_edges_valid, arrival_threshold_valid -- the rule exists once); the stage's
// bookkeeping is capture_stage.h's; which steps are plan steps and whether a box lies inside the mesh is snapshot_plan.h's.
// tests/cpp/interaural_plan_test.cpp covers this file on the CPU.
#pragma once
#include <cstdint>

#include "../../include/wayverb_amd.h"
#include "arrival_plan.h"
#include "snapshot_plan.h"

namespace wv {

constexpr int kInterauralStage = kArrivalStage;        // T: captures the stage holds (two float planes each)
constexpr uint32_t kInterauralMaxBins = 4;             // n_bins at the most (wv_interaural_plan::edges has that many entries)
constexpr uint32_t kInterauralMaxLag = 16;             // L at the most
constexpr int32_t kInterauralMaxEar = 8;               // |component| of an ear offset at the most, in mesh nodes
constexpr uint32_t kInterauralMaxSections = (uint32_t)kDecayMaxSections;
constexpr uint32_t kInterauralNone = kArrivalNone;     // "no onset yet"
constexpr uint64_t kInterauralMaxCaptures = kArrivalMaxCaptures;
constexpr int kInterauralLagChunk = 4;                 // lags on either side whose sums a lane holds at a time

static_assert(kInterauralMaxBins <= kArrivalMaxBins, "arrival_bin counts the edges of an interaural plan");

// planes of one bin: Ea, Eb, C[-L] .. C[+L]
inline uint32_t interaural_planes(uint32_t max_lag) { return 2 * max_lag + 3; }
// the plane of lag tau (-L .. L) inside a bin
inline uint32_t interaural_lag_plane(uint32_t max_lag, int32_t tau) { return (uint32_t)((int32_t)(2 + max_lag) + tau); }

// The bin of a capture `rel` captures behind the node's onset: arrival_bin's rule (the largest w with edges[w] <= rel, the last bin
// open-ended; counted, not searched) over this plan's four entries.  constexpr: interaural_fold_kernel evaluates THIS text.
constexpr uint32_t interaural_bin(uint32_t rel, const uint32_t* edges, uint32_t n_bins) {
    uint32_t k = 0;
    for (uint32_t m = 1; m < kInterauralMaxBins; ++m)
        if (m < n_bins) k += edges[m] <= rel ? 1u : 0u;
    return k;
}

// The lag class the fold kernel is built for: the smallest of 0, 4, 8, 16 that holds L (a lane keeps that many earlier samples per ear).
inline uint32_t interaural_lag_class(uint32_t max_lag) { return max_lag == 0 ? 0u : max_lag <= 4 ? 4u : max_lag <= 8 ? 8u : 16u; }

// one axis: every node taken (first, first + stride, ..., count of them) plus `ear` lies inside [0, mesh).  The axis itself is valid.
inline bool interaural_axis_holds(int64_t first, int64_t count, int64_t stride, int64_t ear, int64_t mesh) {
    const int64_t last = first + (count - 1) * stride;
    return first + ear >= 0 && last + ear < mesh;
}
inline bool interaural_ear_inside(const SnapshotBox& b, const int32_t* ear, int32_t mesh_nx, int32_t mesh_ny, int32_t mesh_nz) {
    return interaural_axis_holds(b.x0, b.nx, b.sx, ear[0], mesh_nx) && interaural_axis_holds(b.y0, b.ny, b.sy, ear[1], mesh_ny) &&
           interaural_axis_holds(b.z0, b.nz, b.sz, ear[2], mesh_nz);
}

// WV_OK (0), or WV_E_INVALID_ARGUMENT with *why (never NULL then) = what is wrong.  The order is behaviour: n_bins, edges, threshold,
// max_lag, the ears' range, n_sections, the sections, strides, period, the box, the ears on the mesh, the plane's size.  (The
// threshold map is the engine's check, behind these: it needs the box.)
inline int interaural_plan_check(const wv_interaural_plan& p, const wv_biquad* sections, int32_t mesh_nx, int32_t mesh_ny, int32_t mesh_nz, const char** why) {
    static const PlanSentences says = WV_PLAN_SENTENCES("wv_set_interaural");
    const char* dummy = nullptr;
    const char*& w = why ? *why : dummy;
    w = nullptr;
    bool ears_in_range = true;
    for (int i = 0; i < 3; ++i)
        ears_in_range = ears_in_range && p.ear_a[i] >= -kInterauralMaxEar && p.ear_a[i] <= kInterauralMaxEar && p.ear_b[i] >= -kInterauralMaxEar &&
                        p.ear_b[i] <= kInterauralMaxEar;
    if (p.n_bins < 1 || p.n_bins > kInterauralMaxBins) w = "wv_set_interaural: n_bins must be 1 .. 4";
    else if (!arrival_edges_valid(p.edges, p.n_bins)) w = "wv_set_interaural: edges[0] must be 0 and the edges strictly increasing";
    else if (!arrival_threshold_valid(p.threshold)) w = "wv_set_interaural: the threshold must be >= 0 and finite";
    else if (p.max_lag > kInterauralMaxLag) w = "wv_set_interaural: max_lag must be 0 .. 16";
    else if (!ears_in_range) w = "wv_set_interaural: every component of an ear offset must be -8 .. 8";
    else if (p.n_sections > kInterauralMaxSections) w = "wv_set_interaural: n_sections must be 0 .. 4";
    else if (p.n_sections && !sections) w = "null argument";
    else if (p.n_sections && !biquads_finite(sections, p.n_sections)) w = "wv_set_interaural: every coefficient must be finite";
    else if ((w = plan_refusal(p, mesh_nx, mesh_ny, mesh_nz, says, kPlanStrides, kPlanLeavesMesh))) {
    } else if (!interaural_ear_inside(plan_box(p), p.ear_a, mesh_nx, mesh_ny, mesh_nz) || !interaural_ear_inside(plan_box(p), p.ear_b, mesh_nx, mesh_ny, mesh_nz))
        w = "wv_set_interaural: an ear leaves the mesh";
    else w = plan_refusal(p, mesh_nx, mesh_ny, mesh_nz, says, kPlanPlaneSize, kPlanPlaneSize);
    return w ? WV_E_INVALID_ARGUMENT : WV_OK;
}

// Block 0 is what a fetch returns, the doubles first so that every part is aligned whatever B is:
//   double pre[2][B], bins[n_bins][2 L + 3][B]; uint32 onset[B]
// Block 1 is what only the fold sees (absent when L == 0 and n_sections == 0):
//   double history[2][L][B] (ear a's L slots, then ear b's; capture c lies in slot c % L), z[2][n_sections][2][B] (ear, section, z1 / z2)
// Offsets in bytes from the block's start; kDecayNoSize where the size leaves 64 bits.
inline uint64_t interaural_pre_offset() { return 0; }
inline uint64_t interaural_bins_offset(uint64_t nodes) { return decay_mul(nodes, 2 * sizeof(double)); }
inline uint64_t interaural_bins_bytes(uint64_t nodes, uint32_t n_bins, uint32_t max_lag) {
    return decay_mul(nodes, (uint64_t)n_bins * interaural_planes(max_lag) * sizeof(double));
}
inline uint64_t interaural_onset_offset(uint64_t nodes, uint32_t n_bins, uint32_t max_lag) {
    return decay_mul(nodes, (2ull + (uint64_t)n_bins * interaural_planes(max_lag)) * sizeof(double));
}
inline uint64_t interaural_sums_bytes(uint64_t nodes, uint32_t n_bins, uint32_t max_lag) {
    return arrival_add(interaural_onset_offset(nodes, n_bins, max_lag), decay_mul(nodes, 4));
}
inline uint64_t interaural_history_bytes(uint64_t nodes, uint32_t max_lag) { return decay_mul(nodes, 2ull * max_lag * sizeof(double)); }
inline uint64_t interaural_filter_offset(uint64_t nodes, uint32_t max_lag) { return interaural_history_bytes(nodes, max_lag); }
inline uint64_t interaural_carry_bytes(uint64_t nodes, uint32_t max_lag, uint32_t n_sections) {
    return decay_mul(nodes, (2ull * max_lag + 4ull * n_sections) * sizeof(double));
}
// the stage float[T][2][B], the optional threshold map float[B], the coefficients double[n_sections][5]
inline uint64_t interaural_stage_bytes(uint64_t nodes) { return decay_mul(nodes, (uint64_t)kInterauralStage * 2 * sizeof(float)); }
inline uint64_t interaural_map_bytes(uint64_t nodes) { return decay_mul(nodes, sizeof(float)); }
inline uint64_t interaural_coef_bytes(uint32_t n_sections) { return (uint64_t)n_sections * kBiquadDoubles * sizeof(double); }
// bytes that cross the link per fetch of everything
inline uint64_t interaural_fetch_bytes(uint64_t nodes, uint32_t n_bins, uint32_t max_lag) { return interaural_sums_bytes(nodes, n_bins, max_lag); }

// The slot of capture c in an ear's history of L slots (L >= 1).
inline uint32_t interaural_history_slot(uint32_t c, uint32_t max_lag) { return c % max_lag; }

// Bytes one fold of t staged captures moves per node, in the steady state where every node has its onset behind it (a MODEL: DESIGN.md
// 4.19): two floats per capture read; the onset read (4 B); min(t, L) history slots per ear read and written, and L read;
// 2 n_sections filter states per ear read and written; 2 L + 3 sums read and written for each of the r bins the node passes through;
// the threshold where a map gives it (4 B).
inline uint64_t interaural_fold_traffic(uint64_t nodes, uint32_t t, uint32_t max_lag, uint32_t n_sections, uint32_t r, bool map) {
    const uint64_t stored = t < max_lag ? t : max_lag;
    return decay_mul(nodes, 8ull * t + 4ull + 16ull * max_lag + 16ull * stored + 64ull * n_sections + 16ull * interaural_planes(max_lag) * r + (map ? 4ull : 0ull));
}

}  // namespace wv

// intensity_plan.h -- (host only, no HIP) the logic of intensity maps (wv_set_intensity, include/wayverb_amd.h) that is the plan's own:
// what a plan is refused for, the sizes of everything that is allocated for one, and the traffic model of a fold.  Which bin a
// capture goes to is decay_plan.h's decay_bin, unchanged; the stage -- 16 slots, free slots, when a fold is due, the good captures
// after a stop -- is spectrum_plan.h's (capture_stage.h holds its bookkeeping for every plan that folds on the device); which steps
// are plan steps and whether a box lies inside the mesh is snapshot_plan.h's.
// tests/cpp/intensity_plan_test.cpp covers this file on the CPU.
#pragma once
#include <cstdint>

#include "../../include/wayverb_amd.h"
#include "decay_plan.h"
#include "snapshot_plan.h"

namespace wv {

constexpr int kIntensityStage = kDecayStage;   // T: captures the stage holds
constexpr uint32_t kIntensityPlanes = 4;       // per staged capture: pressure, gx, gy, gz; per bin: Ix, Iy, Iz, E

// the reference's sentence for a node with a neighbour off the grid (directional_receiver.cpp:18-22), as wv_set_directional_receivers says it
constexpr const char* kIntensityEdge = "Can't place directional_receiver at this node as it is adjacent to a boundary.";

// one axis of a valid box: every taken node has both neighbours on the grid
inline bool intensity_axis_inside(int64_t first, int64_t count, int64_t stride, int64_t mesh) {
    return first >= 1 && first + (count - 1) * stride <= mesh - 2;
}

// What a plan that captures gradients (this one, and the lateral plan) is refused for behind its own counts, in the order both setters
// ask: the shared refusals of snapshot_plan.h with the physical constants between period and box and the mesh's faces ahead of the plane's
// size.  `says`, `constants`: the sentences with the setter's name.
template <typename Plan>
inline const char* gradient_plan_refusal(const Plan& p, int32_t mesh_nx, int32_t mesh_ny, int32_t mesh_nz, const PlanSentences& says, const char* constants) {
    if (const char* w = plan_refusal(p, mesh_nx, mesh_ny, mesh_nz, says, kPlanStrides, kPlanPeriod)) return w;
    if (!physical_constants_valid(p.spacing, p.sample_rate, p.ambient_density)) return constants;
    if (const char* w = plan_refusal(p, mesh_nx, mesh_ny, mesh_nz, says, kPlanLeavesMesh, kPlanLeavesMesh)) return w;
    if (!intensity_axis_inside(p.x0, p.nx, p.sx, mesh_nx) || !intensity_axis_inside(p.y0, p.ny, p.sy, mesh_ny) || !intensity_axis_inside(p.z0, p.nz, p.sz, mesh_nz))
        return kIntensityEdge;
    return plan_refusal(p, mesh_nx, mesh_ny, mesh_nz, says, kPlanPlaneSize, kPlanPlaneSize);
}

// WV_OK, or WV_E_INVALID_ARGUMENT with *why (never NULL then) = what is wrong, in the order wv_set_decay checks what the two share
inline int intensity_plan_check(const wv_intensity_plan& p, int32_t mesh_nx, int32_t mesh_ny, int32_t mesh_nz, const char** why) {
    static const PlanSentences says = WV_PLAN_SENTENCES("wv_set_intensity");
    const char* dummy = nullptr;
    const char*& w = why ? *why : dummy;
    if (p.n_bins < 1 || p.n_bins > kDecayMaxBins) w = "wv_set_intensity: n_bins must be 1 .. 4096";
    else if (p.bin_captures < 1) w = "wv_set_intensity: bin_captures must be >= 1";
    else w = gradient_plan_refusal(p, mesh_nx, mesh_ny, mesh_nz, says, "wv_set_intensity: spacing, sample rate and ambient density must be positive and finite");
    return w ? WV_E_INVALID_ARGUMENT : WV_OK;
}

// bytes of the stage float[T][4][B], of the bins double[4][n_bins][B], of the velocities double[3][B] (kDecayNoSize: past 64 bits)
inline uint64_t intensity_stage_bytes(uint64_t nodes) { return decay_mul(nodes, (uint64_t)kIntensityStage * kIntensityPlanes * sizeof(float)); }
inline uint64_t intensity_bins_bytes(uint64_t nodes, uint32_t n_bins) { return decay_mul(decay_bins_bytes(nodes, n_bins), kIntensityPlanes); }
inline uint64_t intensity_velocity_bytes(uint64_t nodes) { return decay_mul(nodes, 3 * sizeof(double)); }

// bytes one fold of t staged captures into r distinct bins moves, per node: four floats per capture read, three velocities and
// four sums per bin read and written (a model, not a bound)
inline uint64_t intensity_fold_traffic(uint64_t nodes, uint32_t t, uint32_t r) { return decay_mul(nodes, 16ull * t + 48ull + 64ull * r); }

}  // namespace wv

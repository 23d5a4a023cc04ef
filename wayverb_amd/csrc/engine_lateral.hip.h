// engine_lateral.hip.h -- wv_set_lateral / wv_lateral_count / wv_fetch_lateral: a box of the field, decimated, captured every `period`
// steps while wv_run keeps going -- as an intensity plan captures it -- the reference's directional_receiver integrator
// (src/waveguide/src/postprocessor/directional_receiver.cpp:29-69) run at every node taken and, per node and ON THE DEVICE, the
// capture at which the direct sound arrived and p^2, p v and the second-moment tensor v v^T summed into bins counted from the node's
// OWN arrival.  What crosses the link is 36 + 80 n_bins bytes per node when the caller asks for them, however long the run
// (wayverb_amd/lateral.py turns them into the early lateral energy fraction, the direct direction and the diffuseness).
//
// Part of the engine behind the C ABI of include/wayverb_amd.h (engine.hip is the translation unit; see engine.hip.h for the class).
//
// The life cycle -- capture, commit, fold, checkpoint, rollback, release -- is engine_staged.hip.h's.  What is the lateral plan's own:
//   capture   intensity_gather_kernel (intensity_kernels.hip.h, unchanged) -> the device-only stage float[T][4][B]
//   fold      lateral_fold_kernel (lateral_kernels.hip.h) folds all staged captures, in order, into the per-node state.  Which bin a
//             capture goes to differs from node to node, so there is no table for the host to write: the edge table and the number of
//             the first staged capture are kernel arguments, and a fold without kernel timing records no event.
// The state is only ever touched by a fold, and a fold only ever sees committed captures: after a stop on a flag no onset, velocity
// or sum is of a step that was never completed.
#pragma once
#include "engine.hip.h"

namespace wv {

template <typename Real>
void Engine<Real>::Lateral::free_own() {
    if (threshold_map) (void)hipFree(threshold_map);
}

template <typename Real>
int Engine<Real>::set_lateral(const wv_lateral_plan* plan, const float* threshold_map) {
    DeviceGuard guard(device_);
    if (!plan) return staged_stop(lat_);
    if (const int rc = plan_refused("wv_set_lateral", kLateralRow)) return rc;
    const char* why = nullptr;
    if (wv::lateral_plan_check(*plan, nx_, ny_, nz_, &why)) return fail(WV_E_INVALID_ARGUMENT, why);
    const wv::SnapshotBox box = wv::plan_box(*plan);
    const uint64_t nodes = wv::decay_nodes(box.nx, box.ny, box.nz);
    if (const int rc = threshold_map_refused("wv_set_lateral", threshold_map, nodes)) return rc;
    Lateral d;
    d.plan = *plan;
    d.box = box;
    d.spacing = plan->spacing;
    d.nodes = nodes;
    d.k = plan->ambient_density * plan->sample_rate;
    hipError_t rc = staged_allocate(d, wv::lateral_stage_bytes(nodes), wv::lateral_state_bytes(nodes, plan->n_bins));
    // +0.0 everywhere, then NONE (all bits set) into the onsets
    if (rc == hipSuccess) rc = hipMemsetAsync(d.state(), 0, d.block_bytes[0], stream_);
    if (rc == hipSuccess) rc = hipMemsetAsync(d.state() + wv::lateral_onset_offset(nodes, plan->n_bins), 0xFF, (size_t)nodes * 4, stream_);
    if (rc == hipSuccess) rc = threshold_map_upload(d.threshold_map, threshold_map, nodes);
    return staged_install(lat_, d, rc, "wv_set_lateral: no room for the stage and the state", plan->first_step, plan->period);
}

// The lateral plan's part of a fold (staged_fold): the launch.  Staged capture j is capture number folded + j since the plan was set
// (staged_capture keeps it inside 32 bits).
template <typename Real>
int Engine<Real>::lateral_enqueue(Lateral& d, int b, int t, unsigned blocks) {
    const int rc = staged_fold_begins(d, b);
    if (rc) return rc;
    const uint32_t n_bins = d.plan.n_bins;
    // the plan's entries first; what lies behind them is not looked at (arrival_bin stops at n_bins)
    wv::ArrivalEdges edges;
    for (uint32_t m = 0; m < wv::kArrivalMaxBins; ++m) edges.e[m] = m < wv::kLateralMaxBins ? d.plan.edges[m] : wv::kLateralNone;
    unsigned char* const state = d.state();
    hipLaunchKernelGGL(wv::lateral_fold_kernel, dim3(blocks), dim3(256), 0, stream_, d.stage, reinterpret_cast<double*>(state + wv::lateral_pre_offset()),
                       reinterpret_cast<double*>(state + wv::lateral_velocity_offset(d.nodes)), reinterpret_cast<double*>(state + wv::lateral_bins_offset(d.nodes)),
                       reinterpret_cast<uint32_t*>(state + wv::lateral_onset_offset(d.nodes, n_bins)), (const float*)d.threshold_map, d.plan.threshold, edges,
                       n_bins, (uint32_t)d.st.folded, d.nodes, d.k, (int32_t)t);
    return WV_OK;
}

// Folds what is staged, then every part the caller gave a destination for -> the host as it lies.  The plan keeps running.
template <typename Real>
int Engine<Real>::fetch_lateral(uint32_t* onset, double* pre, double* velocity, double* bins, uint64_t* captures) {
    DeviceGuard guard(device_);
    Lateral& d = lat_;
    if (!d.active) return fail(WV_E_STATE, "wv_fetch_lateral: no lateral plan is set");
    const int rc = staged_settle(d);
    if (rc) return rc;
    const uint64_t B = d.nodes;
    const uint32_t n_bins = d.plan.n_bins;
    if (onset) WV_HIP(hipMemcpy(onset, d.state() + wv::lateral_onset_offset(B, n_bins), (size_t)B * 4, hipMemcpyDeviceToHost));
    if (pre) WV_HIP(hipMemcpy(pre, d.state() + wv::lateral_pre_offset(), (size_t)B * 8, hipMemcpyDeviceToHost));
    if (velocity) WV_HIP(hipMemcpy(velocity, d.state() + wv::lateral_velocity_offset(B), (size_t)wv::lateral_velocity_bytes(B), hipMemcpyDeviceToHost));
    if (bins) WV_HIP(hipMemcpy(bins, d.state() + wv::lateral_bins_offset(B), (size_t)wv::lateral_bins_bytes(B, n_bins), hipMemcpyDeviceToHost));
    if (captures) *captures = d.st.folded;
    return WV_OK;
}

}  // namespace wv

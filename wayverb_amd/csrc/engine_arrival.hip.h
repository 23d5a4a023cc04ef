// engine_arrival.hip.h -- wv_set_arrival / wv_arrival_count / wv_fetch_arrival: a box of the field, decimated, captured every `period`
// steps while wv_run keeps going -- as a decay plan captures it -- and per node, ON THE DEVICE, the capture at which the direct sound
// arrived, the peak, the squares summed into bins counted from the node's OWN arrival, the energy ahead of it and the first time
// moment of the energy behind it.  What crosses the link is 28 + 8 n_bins bytes per node when the caller asks for them, however long
// the run (wayverb_amd/arrival.py turns them into arrival time, clarity, definition and centre time).
//
// Part of the engine behind the C ABI of include/wayverb_amd.h (engine.hip is the translation unit; see engine.hip.h for the class).
//
// The life cycle -- capture, commit, fold, checkpoint, rollback, release -- is engine_staged.hip.h's.  What is the arrival plan's own:
//   capture   snapshot_gather_kernel (snapshot_kernels.hip.h, unchanged) -> the device-only stage float[T][B]
//   fold      arrival_fold_kernel (arrival_kernels.hip.h) folds all staged captures, in order, into the per-node state.  Which bin a
//             capture goes to differs from node to node, so there is no table for the host to write: the edge table and the number of
//             the first staged capture are kernel arguments, and a fold without kernel timing records no event.
// The state is only ever touched by a fold, and a fold only ever sees committed captures: after a stop on a flag no onset, peak or
// sum is of a step that was never completed.
#pragma once
#include "engine.hip.h"

namespace wv {

static_assert(sizeof(((wv_arrival_plan*)nullptr)->edges) == sizeof(ArrivalEdges), "the edge table goes to the kernel as it lies in the plan");

template <typename Real>
void Engine<Real>::Arrival::free_own() {
    if (threshold_map) (void)hipFree(threshold_map);
}

template <typename Real>
int Engine<Real>::set_arrival(const wv_arrival_plan* plan, const float* threshold_map) {
    DeviceGuard guard(device_);
    if (!plan) return staged_stop(arr_);
    if (const int rc = plan_refused("wv_set_arrival", kArrivalRow)) return rc;
    if (plan->n_bins < 1 || plan->n_bins > wv::kArrivalMaxBins) return fail(WV_E_INVALID_ARGUMENT, "wv_set_arrival: n_bins must be 1 .. 16");
    if (!wv::arrival_edges_valid(plan->edges, plan->n_bins))
        return fail(WV_E_INVALID_ARGUMENT, "wv_set_arrival: edges[0] must be 0 and the edges strictly increasing");
    if (!wv::arrival_threshold_valid(plan->threshold)) return fail(WV_E_INVALID_ARGUMENT, "wv_set_arrival: the threshold must be >= 0 and finite");
    static const wv::PlanSentences says = WV_PLAN_SENTENCES("wv_set_arrival");
    if (const char* why = wv::plan_refusal(*plan, nx_, ny_, nz_, says)) return fail(WV_E_INVALID_ARGUMENT, why);
    const wv::SnapshotBox box = wv::plan_box(*plan);
    const uint64_t nodes = wv::decay_nodes(box.nx, box.ny, box.nz);
    if (const int rc = threshold_map_refused("wv_set_arrival", threshold_map, nodes)) return rc;
    Arrival d;
    d.plan = *plan;
    d.box = box;
    d.nodes = nodes;
    d.gather_wide = wv::gather_wide(box);
    hipError_t rc = staged_allocate(d, wv::arrival_stage_bytes(nodes), wv::arrival_state_bytes(nodes, plan->n_bins));
    // +0.0 / +0.0f everywhere, then NONE (all bits set) into the onsets and the peak captures
    if (rc == hipSuccess) rc = hipMemsetAsync(d.state(), 0, d.block_bytes[0], stream_);
    if (rc == hipSuccess) rc = hipMemsetAsync(d.state() + wv::arrival_onset_offset(nodes, plan->n_bins), 0xFF, (size_t)nodes * 4, stream_);
    if (rc == hipSuccess) rc = hipMemsetAsync(d.state() + wv::arrival_peak_capture_offset(nodes, plan->n_bins), 0xFF, (size_t)nodes * 4, stream_);
    if (rc == hipSuccess) rc = threshold_map_upload(d.threshold_map, threshold_map, nodes);
    return staged_install(arr_, d, rc, "wv_set_arrival: no room for the stage and the state", plan->first_step, plan->period);
}

// The arrival plan's part of a fold (staged_fold): the launch.  Staged capture j is capture number folded + j since the plan was set
// (staged_capture keeps it inside 32 bits).
template <typename Real>
int Engine<Real>::arrival_enqueue(Arrival& d, int b, int t, unsigned blocks) {
    const int rc = staged_fold_begins(d, b);
    if (rc) return rc;
    const uint32_t n_bins = d.plan.n_bins;
    wv::ArrivalEdges edges;
    for (uint32_t k = 0; k < wv::kArrivalMaxBins; ++k) edges.e[k] = d.plan.edges[k];
    unsigned char* const state = d.state();
    hipLaunchKernelGGL(wv::arrival_fold_kernel, dim3(blocks), dim3(256), 0, stream_, d.stage, reinterpret_cast<double*>(state + wv::arrival_pre_offset()),
                       reinterpret_cast<double*>(state + wv::arrival_moment_offset(d.nodes)), reinterpret_cast<double*>(state + wv::arrival_bins_offset(d.nodes)),
                       reinterpret_cast<uint32_t*>(state + wv::arrival_onset_offset(d.nodes, n_bins)),
                       reinterpret_cast<float*>(state + wv::arrival_peak_offset(d.nodes, n_bins)),
                       reinterpret_cast<uint32_t*>(state + wv::arrival_peak_capture_offset(d.nodes, n_bins)), (const float*)d.threshold_map, d.plan.threshold,
                       edges, n_bins, (uint32_t)d.st.folded, d.nodes, (int32_t)t);
    return WV_OK;
}

// Folds what is staged, then every part the caller gave a destination for -> the host as it lies.  The plan keeps running.
template <typename Real>
int Engine<Real>::fetch_arrival(uint32_t* onset, float* peak, uint32_t* peak_capture, double* pre, double* moment, double* bins, uint64_t* captures) {
    DeviceGuard guard(device_);
    Arrival& d = arr_;
    if (!d.active) return fail(WV_E_STATE, "wv_fetch_arrival: no arrival plan is set");
    const int rc = staged_settle(d);
    if (rc) return rc;
    const uint64_t B = d.nodes;
    const uint32_t n_bins = d.plan.n_bins;
    if (onset) WV_HIP(hipMemcpy(onset, d.state() + wv::arrival_onset_offset(B, n_bins), (size_t)B * 4, hipMemcpyDeviceToHost));
    if (peak) WV_HIP(hipMemcpy(peak, d.state() + wv::arrival_peak_offset(B, n_bins), (size_t)B * 4, hipMemcpyDeviceToHost));
    if (peak_capture) WV_HIP(hipMemcpy(peak_capture, d.state() + wv::arrival_peak_capture_offset(B, n_bins), (size_t)B * 4, hipMemcpyDeviceToHost));
    if (pre) WV_HIP(hipMemcpy(pre, d.state() + wv::arrival_pre_offset(), (size_t)B * 8, hipMemcpyDeviceToHost));
    if (moment) WV_HIP(hipMemcpy(moment, d.state() + wv::arrival_moment_offset(B), (size_t)B * 8, hipMemcpyDeviceToHost));
    if (bins) WV_HIP(hipMemcpy(bins, d.state() + wv::arrival_bins_offset(B), (size_t)wv::arrival_bins_bytes(B, n_bins), hipMemcpyDeviceToHost));
    if (captures) *captures = d.st.folded;
    return WV_OK;
}

}  // namespace wv

// engine_interaural.hip.h -- wv_set_interaural / wv_interaural_count / wv_fetch_interaural: for every node taken by a box, decimated,
// the field at TWO nodes an ear-distance apart, captured every `period` steps while wv_run keeps going, and per node, ON THE DEVICE,
// the capture at which the direct sound arrived and the energies and lagged products of the two (band-passed) signals summed into
// bins counted from the node's OWN arrival: the inter-aural cross-correlation function of ISO 3382-1 Annex B in its head-less
// ("spaced omni") form.  What crosses the link is 20 + 8 n_bins (2 L + 3) bytes per node when the caller asks for them, however long
// the run (wayverb_amd/interaural.py turns them into IACF, IACC and the lag of the maximum).
//
// Part of the engine behind the C ABI of include/wayverb_amd.h (engine.hip is the translation unit; see engine.hip.h for the class).
//
// The life cycle -- capture, commit, fold, checkpoint, rollback, release -- is engine_staged.hip.h's.  What is the interaural plan's own:
//   capture   ear_gather_kernel (interaural_kernels.hip.h; launched in engine_snapshot.hip.h beside the other two captures) -> the
//             device-only stage float[T][2][B]
//   fold      interaural_fold_kernel (interaural_kernels.hip.h) folds all staged captures, in order, into the per-node state.  Which
//             bin a capture goes to differs from node to node, so there is no table for the host to write: the edge table, the number
//             of the first staged capture, L and n_sections are kernel arguments, and a fold without kernel timing records no event.
// The state is only ever touched by a fold, and a fold only ever sees committed captures: after a stop on a flag no onset, sum,
// history slot or filter state is of a step that was never completed.
#pragma once
#include "engine.hip.h"

namespace wv {

static_assert(sizeof(((wv_interaural_plan*)nullptr)->edges) == sizeof(InterauralEdges), "the edge table goes to the kernel as it lies in the plan");
static_assert(sizeof(wv_interaural_plan) == 112, "include/wayverb_amd.h states the layout");

template <typename Real>
void Engine<Real>::Interaural::free_own() {
    if (threshold_map) (void)hipFree(threshold_map);
    if (coef) (void)hipFree(coef);
}

template <typename Real>
int Engine<Real>::set_interaural(const wv_interaural_plan* plan, const wv_biquad* sections, const float* threshold_map) {
    DeviceGuard guard(device_);
    if (!plan) return staged_stop(ia_);
    if (const int rc = plan_refused("wv_set_interaural", kInterauralRow)) return rc;
    const char* why = nullptr;
    if (wv::interaural_plan_check(*plan, sections, nx_, ny_, nz_, &why)) return fail(WV_E_INVALID_ARGUMENT, why);
    const wv::SnapshotBox box = wv::plan_box(*plan);
    const uint64_t nodes = wv::decay_nodes(box.nx, box.ny, box.nz);
    if (const int rc = threshold_map_refused("wv_set_interaural", threshold_map, nodes)) return rc;
    Interaural d;
    d.plan = *plan;
    d.box = box;
    d.nodes = nodes;
    for (int i = 0; i < 3; ++i) d.ear_a[i] = plan->ear_a[i], d.ear_b[i] = plan->ear_b[i];
    const size_t coef_bytes = (size_t)wv::interaural_coef_bytes(plan->n_sections);
    static_assert(sizeof(wv_biquad) == wv::kBiquadDoubles * sizeof(double), "wv_biquad is five doubles: the coefficient table is the caller's array as it lies");
    hipError_t rc = staged_allocate(d, wv::interaural_stage_bytes(nodes), wv::interaural_sums_bytes(nodes, plan->n_bins, plan->max_lag),
                                    wv::interaural_carry_bytes(nodes, plan->max_lag, plan->n_sections));
    if (coef_bytes && rc == hipSuccess && (rc = hipMalloc((void**)&d.coef, coef_bytes)) != hipSuccess) d.coef = nullptr;
    // +0.0 everywhere, then NONE (all bits set) into the onsets
    if (rc == hipSuccess) rc = hipMemsetAsync(d.sums(), 0, d.block_bytes[0], stream_);
    if (rc == hipSuccess) rc = hipMemsetAsync(d.sums() + wv::interaural_onset_offset(nodes, plan->n_bins, plan->max_lag), 0xFF, (size_t)nodes * 4, stream_);
    if (rc == hipSuccess && d.block_bytes[1]) rc = hipMemsetAsync(d.carry(), 0, d.block_bytes[1], stream_);
    if (coef_bytes && rc == hipSuccess) rc = hipMemcpyAsync(d.coef, sections, coef_bytes, hipMemcpyHostToDevice, stream_);
    if (rc == hipSuccess) rc = threshold_map_upload(d.threshold_map, threshold_map, nodes);
    return staged_install(ia_, d, rc, "wv_set_interaural: no room for the stage and the state", plan->first_step, plan->period);
}

// The interaural plan's part of a fold (staged_fold): the launch of the instance for the plan's lag class, with or without the cascade.
// Staged capture j is capture number folded + j since the plan was set (staged_capture keeps it inside 32 bits).
template <typename Real>
int Engine<Real>::interaural_enqueue(Interaural& d, int b, int t, unsigned blocks) {
    const int rc = staged_fold_begins(d, b);
    if (rc) return rc;
    const uint32_t n_bins = d.plan.n_bins, L = d.plan.max_lag, S = d.plan.n_sections;
    wv::InterauralEdges edges;
    for (uint32_t k = 0; k < wv::kInterauralMaxBins; ++k) edges.e[k] = d.plan.edges[k];
    unsigned char* const sums = d.sums();
    double* const history = reinterpret_cast<double*>(d.carry());
    double* const zstate = reinterpret_cast<double*>(d.carry() + wv::interaural_filter_offset(d.nodes, L));
#define WV_INTERAURAL_FOLD(SMAX, LMAX)                                                                                                       \
    hipLaunchKernelGGL((wv::interaural_fold_kernel<SMAX, LMAX>), dim3(blocks), dim3(256), 0, stream_, d.stage,                               \
                       reinterpret_cast<double*>(sums + wv::interaural_pre_offset()), reinterpret_cast<double*>(sums + wv::interaural_bins_offset(d.nodes)), \
                       reinterpret_cast<uint32_t*>(sums + wv::interaural_onset_offset(d.nodes, n_bins, L)), history, zstate, (const double*)d.coef, \
                       (const float*)d.threshold_map, d.plan.threshold, edges, n_bins, L, S, (uint32_t)d.st.folded, d.nodes, (int32_t)t)
    switch (wv::interaural_lag_class(L) + (S ? 1u : 0u)) {
        case 0: WV_INTERAURAL_FOLD(0, 0); break;
        case 1: WV_INTERAURAL_FOLD(4, 0); break;
        case 4: WV_INTERAURAL_FOLD(0, 4); break;
        case 5: WV_INTERAURAL_FOLD(4, 4); break;
        case 8: WV_INTERAURAL_FOLD(0, 8); break;
        case 9: WV_INTERAURAL_FOLD(4, 8); break;
        case 16: WV_INTERAURAL_FOLD(0, 16); break;
        default: WV_INTERAURAL_FOLD(4, 16); break;
    }
#undef WV_INTERAURAL_FOLD
    return WV_OK;
}

// Folds what is staged, then every part the caller gave a destination for -> the host as it lies.  The plan keeps running.
template <typename Real>
int Engine<Real>::fetch_interaural(uint32_t* onset, double* pre, double* bins, uint64_t* captures) {
    DeviceGuard guard(device_);
    Interaural& d = ia_;
    if (!d.active) return fail(WV_E_STATE, "wv_fetch_interaural: no interaural plan is set");
    const int rc = staged_settle(d);
    if (rc) return rc;
    const uint64_t B = d.nodes;
    const uint32_t n_bins = d.plan.n_bins, L = d.plan.max_lag;
    if (onset) WV_HIP(hipMemcpy(onset, d.sums() + wv::interaural_onset_offset(B, n_bins, L), (size_t)B * 4, hipMemcpyDeviceToHost));
    if (pre) WV_HIP(hipMemcpy(pre, d.sums() + wv::interaural_pre_offset(), (size_t)B * 16, hipMemcpyDeviceToHost));
    if (bins) WV_HIP(hipMemcpy(bins, d.sums() + wv::interaural_bins_offset(B), (size_t)wv::interaural_bins_bytes(B, n_bins, L), hipMemcpyDeviceToHost));
    if (captures) *captures = d.st.folded;
    return WV_OK;
}

}  // namespace wv

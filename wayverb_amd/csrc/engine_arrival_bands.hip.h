// engine_arrival_bands.hip.h -- wv_set_arrival_bands / wv_arrival_bands_count / wv_fetch_arrival_bands: the arrival plan with the
// banded decay plan's filter bank ahead of the square, and a bin table that can carry a uniform tail.  A box of the field, decimated,
// captured every `period` steps while wv_run keeps going, and per node ON THE DEVICE: the broadband onset and peak, and per octave band
// the energy ahead of the onset, the first time moment and the squares binned from the node's OWN onset less the band's lag -- early
// windows for C50 / C80 / D50 / Ts and, in the tail, the Schroeder curve for EDT / T20 / T30, from one run (wayverb_amd/arrival.py).
//
// Part of the engine behind the C ABI of include/wayverb_amd.h (engine.hip is the translation unit; see engine.hip.h for the class).
//
// The life cycle -- capture, commit, fold, checkpoint, rollback, release -- is engine_staged.hip.h's.  What is the plan's own:
//   capture   snapshot_gather_kernel (snapshot_kernels.hip.h, unchanged) -> the device-only stage float[T][B]
//   fold      arrival_bands_fold_kernel (arrival_bands_kernels.hip.h), one grid row per band, folds all staged captures, in order, into
//             block 0 (arrival_bands_plan.h has the places) carrying block 1, the filter states.  Which bin a capture goes to differs
//             from node to node, so there is no table for the host to write per fold: edges, tail, lags and the number of the first
//             staged capture are kernel arguments, the bins' first rels a table written once, when the plan is set; a fold without
//             kernel timing records no event.
// The state is only ever touched by a fold, and a fold only ever sees committed captures: after a stop on a flag no onset, peak, sum
// or filter state is of a step that was never completed.
#pragma once
#include "engine.hip.h"

namespace wv {

static_assert(sizeof(((wv_arrival_bands_plan*)nullptr)->edges) == sizeof(((ArrivalBandsTable*)nullptr)->edges) &&
                  sizeof(((wv_arrival_bands_plan*)nullptr)->lag) == sizeof(((ArrivalBandsTable*)nullptr)->lag),
              "edges and lags go to the kernel as they lie in the plan");

template <typename Real>
void Engine<Real>::ArrivalBands::free_own() {
    if (threshold_map) (void)hipFree(threshold_map);
    if (coef) (void)hipFree(coef);
}

template <typename Real>
int Engine<Real>::set_arrival_bands(const wv_arrival_bands_plan* plan, const float* threshold_map, const wv_biquad* sections, uint32_t n_bands,
                                    uint32_t n_sections) {
    DeviceGuard guard(device_);
    if (!plan) return staged_stop(arrb_);
    if (const int rc = plan_refused("wv_set_arrival_bands", kArrivalBandsRow)) return rc;
    static const wv::PlanSentences says = WV_PLAN_SENTENCES("wv_set_arrival_bands");
    if (const char* why = wv::plan_refusal(*plan, nx_, ny_, nz_, says)) return fail(WV_E_INVALID_ARGUMENT, why);
    if (!wv::decay_bands_valid(n_bands, n_sections)) return fail(WV_E_INVALID_ARGUMENT, "wv_set_arrival_bands: n_bands must be 1 .. 8 and n_sections 1 .. 4");
    if (!sections) return fail(WV_E_INVALID_ARGUMENT, "null argument");
    if (!wv::biquads_finite(sections, n_bands * n_sections)) return fail(WV_E_INVALID_ARGUMENT, "wv_set_arrival_bands: every coefficient must be finite");
    if (plan->n_edges < 1 || plan->n_edges > wv::kArrivalMaxBins) return fail(WV_E_INVALID_ARGUMENT, "wv_set_arrival_bands: n_edges must be 1 .. 16");
    if (!wv::arrival_edges_valid(plan->edges, plan->n_edges))
        return fail(WV_E_INVALID_ARGUMENT, "wv_set_arrival_bands: edges[0] must be 0 and the edges strictly increasing");
    if (!wv::arrival_threshold_valid(plan->threshold)) return fail(WV_E_INVALID_ARGUMENT, "wv_set_arrival_bands: the threshold must be >= 0 and finite");
    const wv::SnapshotBox box = wv::plan_box(*plan);
    const uint64_t nodes = wv::decay_nodes(box.nx, box.ny, box.nz);
    if (const int rc = threshold_map_refused("wv_set_arrival_bands", threshold_map, nodes)) return rc;
    if (!wv::arrival_bands_tail_count_valid(plan->n_edges, plan->n_tail))
        return fail(WV_E_INVALID_ARGUMENT, "wv_set_arrival_bands: n_tail must be 0 .. 4096 - n_edges");
    if (!wv::arrival_bands_tail_first_valid(plan->edges, plan->n_edges, plan->n_tail, plan->tail_first))
        return fail(WV_E_INVALID_ARGUMENT, "wv_set_arrival_bands: tail_first must lie behind the last edge");
    if (!wv::arrival_bands_tail_captures_valid(plan->n_tail, plan->tail_captures))
        return fail(WV_E_INVALID_ARGUMENT, "wv_set_arrival_bands: tail_captures must be >= 1");
    if (plan->reserved != 0) return fail(WV_E_INVALID_ARGUMENT, "wv_set_arrival_bands: reserved must be 0");
    ArrivalBands d;
    d.plan = *plan;
    d.box = box;
    d.nodes = nodes;
    d.gather_wide = wv::gather_wide(box);
    d.n_bands = n_bands;
    d.n_sections = n_sections;
    d.n_bins = plan->n_edges + plan->n_tail;
    for (uint32_t k = 0; k < wv::kArrivalMaxBins; ++k) d.table.edges[k] = plan->edges[k];
    for (uint32_t k = 0; k < wv::kArrivalBandsMaxBands; ++k) d.table.lag[k] = k < n_bands ? plan->lag[k] : 0;
    d.table.n_edges = plan->n_edges;
    d.table.n_tail = plan->n_tail;
    d.table.tail_first = plan->n_tail ? plan->tail_first : 0;
    d.table.tail_captures = plan->n_tail ? plan->tail_captures : 1;
    const size_t coef_bytes = (size_t)wv::arrival_bands_coef_bytes(n_bands, n_sections);
    static_assert(sizeof(wv_biquad) == wv::kBiquadDoubles * sizeof(double), "wv_biquad is five doubles: the coefficient table is the caller's array as it lies");
    hipError_t rc = staged_allocate(d, wv::arrival_bands_stage_bytes(nodes), wv::arrival_bands_sums_bytes(nodes, n_bands, d.n_bins),
                                    wv::arrival_bands_state_bytes(nodes, n_bands, n_sections));
    std::vector<uint32_t> bin_first(wv::arrival_bands_bin_first_entries(d.n_bins));
    wv::arrival_bands_bin_first(d.table, bin_first.data());
    if (rc == hipSuccess && (rc = hipMalloc((void**)&d.coef, (size_t)wv::arrival_bands_tables_bytes(n_bands, n_sections, d.n_bins))) != hipSuccess) d.coef = nullptr;
    // +0.0 / +0.0f everywhere, then NONE (all bits set) into the onsets of every band and the peak captures
    if (rc == hipSuccess) rc = hipMemsetAsync(d.sums(), 0, d.block_bytes[0], stream_);
    if (rc == hipSuccess) rc = hipMemsetAsync(d.sums() + wv::arrival_bands_onset_offset(nodes, n_bands, d.n_bins), 0xFF, (size_t)nodes * 4 * n_bands, stream_);
    if (rc == hipSuccess) rc = hipMemsetAsync(d.sums() + wv::arrival_bands_peak_capture_offset(nodes, n_bands, d.n_bins), 0xFF, (size_t)nodes * 4, stream_);
    if (rc == hipSuccess) rc = hipMemsetAsync(d.state(), 0, d.block_bytes[1], stream_);
    if (rc == hipSuccess) rc = hipMemcpyAsync(d.coef, sections, coef_bytes, hipMemcpyHostToDevice, stream_);
    if (rc == hipSuccess) rc = hipMemcpyAsync(d.bin_first(), bin_first.data(), bin_first.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream_);  // (staged_install synchronises: the vector outlives the copy)
    if (rc == hipSuccess) rc = threshold_map_upload(d.threshold_map, threshold_map, nodes);
    return staged_install(arrb_, d, rc, "wv_set_arrival_bands: no room for the stage, the sums and the filter states", plan->first_step, plan->period);
}

// The plan's part of a fold (staged_fold): the launch.  Staged capture j is capture number folded + j since the plan was set
// (staged_capture keeps it inside 32 bits).
template <typename Real>
int Engine<Real>::arrival_bands_enqueue(ArrivalBands& d, int b, int t, unsigned blocks) {
    const int rc = staged_fold_begins(d, b);
    if (rc) return rc;
    const uint32_t K = d.n_bands;
    unsigned char* const sums = d.sums();
    const dim3 grid(blocks, K);  // (blockIdx.y = the band; one node per lane)
#define WV_ARRIVAL_BANDS_FOLD(S)                                                                                                                  \
    hipLaunchKernelGGL((wv::arrival_bands_fold_kernel<S>), grid, dim3(256), 0, stream_, d.stage, d.state(),                                         \
                       reinterpret_cast<double*>(sums + wv::arrival_bands_pre_offset()),                                                           \
                       reinterpret_cast<double*>(sums + wv::arrival_bands_moment_offset(d.nodes, K)),                                              \
                       reinterpret_cast<double*>(sums + wv::arrival_bands_bins_offset(d.nodes, K)),                                                \
                       reinterpret_cast<uint32_t*>(sums + wv::arrival_bands_onset_offset(d.nodes, K, d.n_bins)),                                   \
                       reinterpret_cast<float*>(sums + wv::arrival_bands_peak_offset(d.nodes, K, d.n_bins)),                                       \
                       reinterpret_cast<uint32_t*>(sums + wv::arrival_bands_peak_capture_offset(d.nodes, K, d.n_bins)), (const float*)d.threshold_map, \
                       d.plan.threshold, (const double*)d.coef, (const uint32_t*)d.bin_first(), d.table, (uint32_t)d.st.folded, d.nodes, (int32_t)t)
    switch (d.n_sections) {
        case 1: WV_ARRIVAL_BANDS_FOLD(1); break;
        case 2: WV_ARRIVAL_BANDS_FOLD(2); break;
        case 3: WV_ARRIVAL_BANDS_FOLD(3); break;
        default: WV_ARRIVAL_BANDS_FOLD(4); break;
    }
#undef WV_ARRIVAL_BANDS_FOLD
    return WV_OK;
}

// (the plan's name is two words: the sentence staged_count would make of it names no function)
template <typename Real>
int Engine<Real>::arrival_bands_count(uint64_t* captures, uint64_t* last_step) {
    if (!arrb_.active) return fail(WV_E_STATE, "wv_arrival_bands_count: no banded arrival plan is set");
    return staged_count(arrb_, captures, last_step);
}

// Folds what is staged, then every part the caller gave a destination for -> the host as it lies (the onset: band 0's copy).  The plan
// keeps running.
template <typename Real>
int Engine<Real>::fetch_arrival_bands(uint32_t* onset, float* peak, uint32_t* peak_capture, double* pre, double* moment, double* bins, uint64_t* captures) {
    DeviceGuard guard(device_);
    ArrivalBands& d = arrb_;
    if (!d.active) return fail(WV_E_STATE, "wv_fetch_arrival_bands: no banded arrival plan is set");
    const int rc = staged_settle(d);
    if (rc) return rc;
    const uint64_t B = d.nodes;
    const uint32_t K = d.n_bands, n_bins = d.n_bins;
    if (onset) WV_HIP(hipMemcpy(onset, d.sums() + wv::arrival_bands_onset_offset(B, K, n_bins), (size_t)B * 4, hipMemcpyDeviceToHost));
    if (peak) WV_HIP(hipMemcpy(peak, d.sums() + wv::arrival_bands_peak_offset(B, K, n_bins), (size_t)B * 4, hipMemcpyDeviceToHost));
    if (peak_capture) WV_HIP(hipMemcpy(peak_capture, d.sums() + wv::arrival_bands_peak_capture_offset(B, K, n_bins), (size_t)B * 4, hipMemcpyDeviceToHost));
    if (pre) WV_HIP(hipMemcpy(pre, d.sums() + wv::arrival_bands_pre_offset(), (size_t)B * 8 * K, hipMemcpyDeviceToHost));
    if (moment) WV_HIP(hipMemcpy(moment, d.sums() + wv::arrival_bands_moment_offset(B, K), (size_t)B * 8 * K, hipMemcpyDeviceToHost));
    if (bins) WV_HIP(hipMemcpy(bins, d.sums() + wv::arrival_bands_bins_offset(B, K), (size_t)wv::arrival_bands_bins_bytes(B, K, n_bins), hipMemcpyDeviceToHost));
    if (captures) *captures = d.st.folded;
    return WV_OK;
}

}  // namespace wv

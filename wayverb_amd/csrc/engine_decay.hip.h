// engine_decay.hip.h -- wv_set_decay / wv_decay_count / wv_fetch_decay: a box of the field, decimated, captured every `period` steps
// while wv_run keeps going -- as a snapshot plan captures it -- and its squares summed per node into time bins ON THE DEVICE.  What
// crosses the link is n_bins doubles per node when the caller asks for them, however long the run; the backward sums of the bins are
// the Schroeder integral at the bin edges (wayverb_amd/decay.py).
//
// Part of the engine behind the C ABI of include/wayverb_amd.h (engine.hip is the translation unit; see engine.hip.h for the class).
//
// The life cycle -- capture, commit, fold, checkpoint, rollback, release -- is engine_staged.hip.h's.  What is the decay plan's own:
//   capture   snapshot_gather_kernel (snapshot_kernels.hip.h, unchanged) -> the device-only stage float[T][B]
//   fold      decay_fold_kernel (decay_kernels.hip.h) folds all staged captures into the bins double[n_bins][B].  The bins of the t
//             staged captures, int32[t], are written by the host (decay_plan.h: decay_bin of the capture's number since the plan was
//             set) into one of two page-locked tables and copied ahead of the launch (BinTable, which the intensity plan uses too).
//
// wv_set_decay_bands / wv_fetch_decay_bands are the same plan with a filter bank ahead of the square: n_bands cascades of n_sections
// biquad sections per node, their state double[n_bands][n_sections][2][B] and the coefficient table beside the bins, which grow to
// double[n_bands][n_bins][B]; decay_bands_fold_kernel (decay_bands_kernels.hip.h) takes decay_fold_kernel's place, one grid row per
// band.  Capture, commit, the fold's timing, the cut of batches, the exclusions and the queries are the plain plan's, unchanged:
// the state is only ever touched by a fold, and a fold only ever sees committed captures.
#pragma once
#include "engine.hip.h"

namespace wv {

// Turn b's table for a fold of plan p's t staged captures: staged capture j is capture number folded + j since the plan was set.
template <typename Real>
int Engine<Real>::bin_table_write(BinTable& table, const StagedPlan& p, int b, int t, uint32_t bin_captures, uint32_t n_bins) {
    for (int j = 0; j < t; ++j) table.host[b][j] = (int32_t)wv::decay_bin(p.st.folded + (uint64_t)j, bin_captures, n_bins);
    WV_HIP(hipMemcpyAsync(table.dev[b], table.host[b], (size_t)t * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
    return WV_OK;
}

template <typename Real>
void Engine<Real>::Decay::free_own() {
    if (coef) (void)hipFree(coef);
    host_table_free(table);
}

template <typename Real>
int Engine<Real>::set_decay(const wv_decay_plan* plan) {
    return decay_set(plan, nullptr, 0, 0, false);
}

template <typename Real>
int Engine<Real>::set_decay_bands(const wv_decay_plan* plan, const wv_biquad* sections, uint32_t n_bands, uint32_t n_sections) {
    return decay_set(plan, sections, n_bands, n_sections, true);
}

// Both setters: `banded` says which one was called (a plain plan has n_bands = 0 and neither state nor coefficients).
template <typename Real>
int Engine<Real>::decay_set(const wv_decay_plan* plan, const wv_biquad* sections, uint32_t n_bands, uint32_t n_sections, bool banded) {
    DeviceGuard guard(device_);
    const std::string who = banded ? "wv_set_decay_bands" : "wv_set_decay";
    if (!plan) return staged_stop(decay_);
    // the two kinds of decay plan answer to different fetches: neither setter turns one into the other behind the caller's back (a
    // plain plan under a banded one is refused with the other plans, in plan_refused's words)
    if (decay_.active && banded && !decay_.n_bands)
        return fail(WV_E_STATE, "wv_set_decay_bands: a plain decay plan is active (wv_set_decay(e, NULL) stops it); the plans exclude each other");
    if (const int rc = plan_refused(who, banded ? kBandedDecayRow : kPlainDecayRow)) return rc;
    if (banded) {
        if (!wv::decay_bands_valid(n_bands, n_sections)) return fail(WV_E_INVALID_ARGUMENT, "wv_set_decay_bands: n_bands must be 1 .. 8 and n_sections 1 .. 4");
        if (!sections) return fail(WV_E_INVALID_ARGUMENT, "null argument");
        if (!wv::biquads_finite(sections, n_bands * n_sections)) return fail(WV_E_INVALID_ARGUMENT, "wv_set_decay_bands: every coefficient must be finite");
    }
    if (plan->n_bins < 1 || plan->n_bins > wv::kDecayMaxBins) return fail(WV_E_INVALID_ARGUMENT, who + ": n_bins must be 1 .. 4096");
    if (plan->bin_captures < 1) return fail(WV_E_INVALID_ARGUMENT, who + ": bin_captures must be >= 1");
    static const wv::PlanSentences says[2] = {WV_PLAN_SENTENCES("wv_set_decay"), WV_PLAN_SENTENCES("wv_set_decay_bands")};
    if (const char* why = wv::plan_refusal(*plan, nx_, ny_, nz_, says[banded])) return fail(WV_E_INVALID_ARGUMENT, why);
    const wv::SnapshotBox box = wv::plan_box(*plan);
    Decay d;
    d.plan = *plan;
    d.box = box;
    d.nodes = wv::decay_nodes(box.nx, box.ny, box.nz);
    d.gather_wide = wv::gather_wide(box);
    d.fold_wide = !banded && d.nodes % 2 == 0;  // two nodes per lane, 16-byte accesses on the bins
    d.n_bands = banded ? n_bands : 0;
    d.n_sections = banded ? n_sections : 0;
    const uint64_t bins_bytes = banded ? wv::decay_band_bins_bytes(d.nodes, plan->n_bins, n_bands) : wv::decay_bins_bytes(d.nodes, plan->n_bins);
    const uint64_t state_bytes = banded ? wv::decay_band_state_bytes(d.nodes, n_bands, n_sections) : 0;
    const size_t coef_bytes = banded ? (size_t)wv::decay_band_coef_bytes(n_bands, n_sections) : 0;
    static_assert(sizeof(wv_biquad) == wv::kBiquadDoubles * sizeof(double), "wv_biquad is five doubles: the coefficient table is the caller's array as it lies");
    hipError_t rc = staged_allocate(d, wv::decay_stage_bytes(d.nodes), bins_bytes, state_bytes);
    if (banded && rc == hipSuccess && (rc = hipMalloc((void**)&d.coef, coef_bytes)) != hipSuccess) d.coef = nullptr;
    if (rc == hipSuccess) rc = host_table_allocate(d.table, (size_t)wv::decay_table_bytes());
    if (rc == hipSuccess) rc = hipMemsetAsync(d.bins(), 0, d.block_bytes[0], stream_);  // (+0.0 everywhere)
    if (banded && rc == hipSuccess) rc = hipMemsetAsync(d.state(), 0, d.block_bytes[1], stream_);
    if (banded && rc == hipSuccess) rc = hipMemcpyAsync(d.coef, sections, coef_bytes, hipMemcpyHostToDevice, stream_);
    return staged_install(decay_, d, rc, who + ": no room for the stage and the bins", plan->first_step, plan->period);
}

// The decay plan's part of a fold (staged_fold): the bins of the t staged captures into turn b's table, its copy, the launch.
template <typename Real>
int Engine<Real>::decay_enqueue(Decay& d, int b, int t, unsigned blocks) {
    int rc = bin_table_write(d.table, d, b, t, d.plan.bin_captures, d.plan.n_bins);
    if (rc || (rc = staged_fold_begins(d, b))) return rc;
    if (d.n_bands) {
        const dim3 grid(blocks, d.n_bands);  // (blockIdx.y = the band; one node per lane)
#define WV_BANDS_FOLD(S)                                                                                                                  \
    hipLaunchKernelGGL((wv::decay_bands_fold_kernel<S>), grid, dim3(256), 0, stream_, d.stage, d.state(), d.bins(), d.coef, d.table.dev[b], d.nodes, \
                       d.plan.n_bins, (int32_t)t)
        switch (d.n_sections) {
            case 1: WV_BANDS_FOLD(1); break;
            case 2: WV_BANDS_FOLD(2); break;
            case 3: WV_BANDS_FOLD(3); break;
            default: WV_BANDS_FOLD(4); break;
        }
#undef WV_BANDS_FOLD
    } else if (d.fold_wide)
        hipLaunchKernelGGL((wv::decay_fold_kernel<true>), dim3(blocks), dim3(256), 0, stream_, d.stage, d.bins(), d.table.dev[b], d.nodes, (int32_t)t);
    else
        hipLaunchKernelGGL((wv::decay_fold_kernel<false>), dim3(blocks), dim3(256), 0, stream_, d.stage, d.bins(), d.table.dev[b], d.nodes, (int32_t)t);
    return WV_OK;
}

// Folds what is staged, then the bins -> the host as they lie: [n_bins][nz][ny][nx].  The plan keeps running.
template <typename Real>
int Engine<Real>::fetch_decay(double* dst, uint64_t* captures) {
    return decay_fetch(dst, captures, false);
}

// ... a banded plan's: [n_bands][n_bins][nz][ny][nx].
template <typename Real>
int Engine<Real>::fetch_decay_bands(double* dst, uint64_t* captures) {
    return decay_fetch(dst, captures, true);
}

template <typename Real>
int Engine<Real>::decay_fetch(double* dst, uint64_t* captures, bool banded) {
    DeviceGuard guard(device_);
    Decay& d = decay_;
    if (!d.active) return fail(WV_E_STATE, banded ? "wv_fetch_decay_bands: no decay plan is set" : "wv_fetch_decay: no decay plan is set");
    if (banded && !d.n_bands) return fail(WV_E_STATE, "wv_fetch_decay_bands: the decay plan is a plain one (wv_fetch_decay fetches its bins)");
    if (!banded && d.n_bands) return fail(WV_E_STATE, "wv_fetch_decay: the decay plan is a banded one (wv_fetch_decay_bands fetches its bins)");
    if (!dst) return fail(WV_E_INVALID_ARGUMENT, "null argument");
    const int rc = staged_settle(d);
    if (rc) return rc;
    WV_HIP(hipMemcpy(dst, d.bins(), d.block_bytes[0], hipMemcpyDeviceToHost));
    if (captures) *captures = d.st.folded;
    return WV_OK;
}

}  // namespace wv

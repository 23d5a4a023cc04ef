// engine_waterfall.hip.h -- wv_set_waterfall / wv_waterfall_count / wv_fetch_waterfall: a box of the field, decimated, captured every
// `period` steps while wv_run keeps going -- as a spectrum plan captures it -- and Fourier-transformed ON THE DEVICE at K given
// frequencies PER TIME BIN: the short-time spectrum of every node taken, whose backward cumulative sums are the cumulative spectral
// decay at the bin edges (wayverb_amd/waterfall.py).  What crosses the link is n_bins * K complex numbers per node when the caller asks
// for them, however long the run.
//
// Part of the engine behind the C ABI of include/wayverb_amd.h (engine.hip is the translation unit; see engine.hip.h for the class).
//
// The life cycle -- capture, commit, fold, checkpoint, rollback, release -- is engine_staged.hip.h's.  What is the waterfall plan's own:
//   capture   snapshot_gather_kernel (snapshot_kernels.hip.h, unchanged) -> the device-only stage float[T][B]
//   fold      waterfall_fold_kernel (waterfall_kernels.hip.h) folds all staged captures into the sums double[n_bins][K][2][B]; a fold
//             moves 32 K bytes per node and bin it touches.  It reads TWO host-written tables, each in one of two
//             page-locked buffers taken in turn and copied ahead of the launch (engine_staged.hip.h): the bins int32[t] of the staged
//             captures (BinTable: decay_plan.h's decay_bin of the capture's number since the plan was set) and their twiddles
//             double[t][K][2] (TwiddleTable: wv_spectrum_twiddle at the staged steps).
#pragma once
#include "engine.hip.h"

namespace wv {

template <typename Real>
int Engine<Real>::set_waterfall(const wv_waterfall_plan* plan, const double* cycles_per_step) {
    DeviceGuard guard(device_);
    if (!plan) return staged_stop(wf_);
    if (const int rc = plan_refused("wv_set_waterfall", kWaterfallRow)) return rc;
    if (plan->n_freqs < 1 || plan->n_freqs > wv::kWaterfallMaxFreqs) return fail(WV_E_INVALID_ARGUMENT, "wv_set_waterfall: n_freqs must be 1 .. 64");
    if (!cycles_per_step) return fail(WV_E_INVALID_ARGUMENT, "null argument");
    for (uint32_t k = 0; k < plan->n_freqs; ++k)
        if (!wv::frequency_valid(cycles_per_step[k]))
            return fail(WV_E_INVALID_ARGUMENT, "wv_set_waterfall: a frequency outside [0, 0.5] cycles per step");
    if (plan->n_bins < 1 || plan->n_bins > wv::kWaterfallMaxBins) return fail(WV_E_INVALID_ARGUMENT, "wv_set_waterfall: n_bins must be 1 .. 4096");
    if (plan->bin_captures < 1) return fail(WV_E_INVALID_ARGUMENT, "wv_set_waterfall: bin_captures must be >= 1");
    if (!wv::waterfall_sums_valid(plan->n_freqs, plan->n_bins))
        return fail(WV_E_INVALID_ARGUMENT, "wv_set_waterfall: n_freqs * n_bins must be <= 4096 (64 KiB of sums per node)");
    static const wv::PlanSentences says = WV_PLAN_SENTENCES("wv_set_waterfall");
    if (const char* why = wv::plan_refusal(*plan, nx_, ny_, nz_, says)) return fail(WV_E_INVALID_ARGUMENT, why);
    const wv::SnapshotBox box = wv::plan_box(*plan);
    Waterfall w;
    w.plan = *plan;
    w.box = box;
    w.freqs.assign(cycles_per_step, cycles_per_step + plan->n_freqs);
    w.nodes = wv::waterfall_nodes(box.nx, box.ny, box.nz);
    w.gather_wide = wv::gather_wide(box);
    w.fold_wide = w.nodes % 2 == 0;  // two nodes per lane, 16-byte accesses on the sums
    hipError_t rc = staged_allocate(w, wv::waterfall_stage_bytes(w.nodes), wv::waterfall_sum_bytes(w.nodes, plan->n_bins, plan->n_freqs));
    if (rc == hipSuccess) rc = host_table_allocate(w.table, (size_t)wv::waterfall_bin_table_bytes());
    if (rc == hipSuccess) rc = host_table_allocate(w.tw, (size_t)wv::waterfall_twiddle_table_bytes(plan->n_freqs));
    if (rc == hipSuccess) rc = hipMemsetAsync(w.acc(), 0, w.block_bytes[0], stream_);  // (+0.0 everywhere)
    return staged_install(wf_, w, rc, "wv_set_waterfall: no room for the stage and the sums", plan->first_step, plan->period);
}

// The waterfall plan's part of a fold (staged_fold): the bins and the twiddles of the t staged captures into turn b's tables, their
// copies, the launch.
template <typename Real>
int Engine<Real>::waterfall_enqueue(Waterfall& w, int b, int t, unsigned blocks) {
    int rc = bin_table_write(w.table, w, b, t, w.plan.bin_captures, w.plan.n_bins);
    if (rc || (rc = twiddle_table_write(w.tw, w, b, t, w.freqs)) || (rc = staged_fold_begins(w, b))) return rc;
    const auto kernel = w.fold_wide ? wv::waterfall_fold_kernel<true> : wv::waterfall_fold_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, stream_, w.stage, w.acc(), w.table.dev[b], w.tw.dev[b], w.nodes, (int32_t)t, (int32_t)w.plan.n_freqs);
    return WV_OK;
}

// Folds what is staged, then the planar sums -> the host, interleaved to [n_bins][K][nz][ny][nx][2] there (not on the hot path).  The
// plan keeps running.
template <typename Real>
int Engine<Real>::fetch_waterfall(double* dst, uint64_t* captures) {
    DeviceGuard guard(device_);
    Waterfall& w = wf_;
    if (!w.active) return fail(WV_E_STATE, "wv_fetch_waterfall: no waterfall plan is set");
    if (!dst) return fail(WV_E_INVALID_ARGUMENT, "null argument");
    if (const int rc = staged_settle(w)) return rc;
    std::vector<double> planes((size_t)w.nodes * 2);
    const uint64_t pairs = (uint64_t)w.plan.n_bins * w.plan.n_freqs;  // (bin-major, then frequency: as the sums lie)
    for (uint64_t i = 0; i < pairs; ++i)
        if (const int rc = fetch_interleaved(w.acc() + i * 2 * w.nodes, w.nodes, dst + i * 2 * w.nodes, planes)) return rc;
    if (captures) *captures = w.st.folded;
    return WV_OK;
}

}  // namespace wv

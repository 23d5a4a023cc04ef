// engine_spectrum.hip.h -- wv_set_spectrum / wv_spectrum_count / wv_fetch_spectrum: a box of the field, decimated, captured every
// `period` steps while wv_run keeps going -- as a snapshot plan captures it -- and Fourier-transformed ON THE DEVICE at K given
// frequencies.  What crosses the link is K complex numbers per node when the caller asks for them, however long the run.
//
// Part of the engine behind the C ABI of include/wayverb_amd.h (engine.hip is the translation unit; see engine.hip.h for the class).
//
// The life cycle -- capture, commit, fold, checkpoint, rollback, release -- is engine_staged.hip.h's.  What is the spectrum's own:
//   capture   snapshot_gather_kernel (snapshot_kernels.hip.h, unchanged) -> the device-only stage float[T][B]
//   fold      spectrum_fold_kernel (spectrum_kernels.hip.h) folds all staged captures into the sums double[K][2][B]; a fold moves
//             32 K bytes per node whatever the number of captures.
//             Its twiddle table double[t][K][2] is written by the host (wv_spectrum_twiddle) into one of two page-locked buffers
//             and copied ahead of the launch (TwiddleTable, engine_staged.hip.h); two, so that the host never rewrites a table a queued
//             copy still reads.
#pragma once
#include "engine.hip.h"

namespace wv {

template <typename Real>
int Engine<Real>::set_spectrum(const wv_spectrum_plan* plan, const double* cycles_per_step) {
    DeviceGuard guard(device_);
    if (!plan) return staged_stop(spec_);
    if (const int rc = plan_refused("wv_set_spectrum", kSpectrumRow)) return rc;
    if (plan->n_freqs < 1 || plan->n_freqs > wv::kSpectrumMaxFreqs) return fail(WV_E_INVALID_ARGUMENT, "wv_set_spectrum: n_freqs must be 1 .. 64");
    if (!cycles_per_step) return fail(WV_E_INVALID_ARGUMENT, "null argument");
    for (uint32_t k = 0; k < plan->n_freqs; ++k)
        if (!wv::frequency_valid(cycles_per_step[k]))
            return fail(WV_E_INVALID_ARGUMENT, "wv_set_spectrum: a frequency outside [0, 0.5] cycles per step");
    static const wv::PlanSentences says = WV_PLAN_SENTENCES("wv_set_spectrum");
    if (const char* why = wv::plan_refusal(*plan, nx_, ny_, nz_, says)) return fail(WV_E_INVALID_ARGUMENT, why);
    const wv::SnapshotBox box = wv::plan_box(*plan);
    Spectrum s;
    s.plan = *plan;
    s.box = box;
    s.freqs.assign(cycles_per_step, cycles_per_step + plan->n_freqs);
    s.nodes = wv::spectrum_nodes(box.nx, box.ny, box.nz);
    s.gather_wide = wv::gather_wide(box);
    s.fold_wide = s.nodes % 2 == 0;  // two nodes per lane, 16-byte accesses on the sums
    const size_t table_bytes = (size_t)wv::spectrum_table_bytes(plan->n_freqs);
    hipError_t rc = staged_allocate(s, wv::spectrum_stage_bytes(s.nodes), wv::spectrum_sum_bytes(s.nodes, plan->n_freqs));
    if (rc == hipSuccess) rc = host_table_allocate(s.tw, table_bytes);
    if (rc == hipSuccess) rc = hipMemsetAsync(s.acc(), 0, s.block_bytes[0], stream_);  // (+0.0 everywhere)
    return staged_install(spec_, s, rc, "wv_set_spectrum: no room for the stage and the sums", plan->first_step, plan->period);
}

// The spectrum's part of a fold (staged_fold): the twiddles of the t staged captures into turn b's table, its copy, the launch.
template <typename Real>
int Engine<Real>::spectrum_enqueue(Spectrum& s, int b, int t, unsigned blocks) {
    int rc = twiddle_table_write(s.tw, s, b, t, s.freqs);
    if (rc || (rc = staged_fold_begins(s, b))) return rc;
    const uint32_t K = s.plan.n_freqs;
    if (s.fold_wide)
        hipLaunchKernelGGL((wv::spectrum_fold_kernel<true>), dim3(blocks), dim3(256), 0, stream_, s.stage, s.acc(), s.tw.dev[b], s.nodes, (int32_t)t, (int32_t)K);
    else
        hipLaunchKernelGGL((wv::spectrum_fold_kernel<false>), dim3(blocks), dim3(256), 0, stream_, s.stage, s.acc(), s.tw.dev[b], s.nodes, (int32_t)t, (int32_t)K);
    return WV_OK;
}

// Folds what is staged, then the planar sums -> the host, interleaved to [K][nz][ny][nx][2] there (not on the hot path).  The plan
// keeps running.
template <typename Real>
int Engine<Real>::fetch_spectrum(double* dst, uint64_t* captures) {
    DeviceGuard guard(device_);
    Spectrum& s = spec_;
    if (!s.active) return fail(WV_E_STATE, "wv_fetch_spectrum: no spectrum plan is set");
    if (!dst) return fail(WV_E_INVALID_ARGUMENT, "null argument");
    if (const int rc = staged_settle(s)) return rc;
    std::vector<double> planes((size_t)s.nodes * 2);
    for (uint32_t k = 0; k < s.plan.n_freqs; ++k)
        if (const int rc = fetch_interleaved(s.acc() + (uint64_t)k * 2 * s.nodes, s.nodes, dst + (uint64_t)k * 2 * s.nodes, planes)) return rc;
    if (captures) *captures = s.st.folded;
    return WV_OK;
}

}  // namespace wv

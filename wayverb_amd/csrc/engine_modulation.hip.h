// engine_modulation.hip.h -- wv_set_modulation / wv_modulation_count / wv_fetch_modulation: a box of the field, decimated, captured
// every `period` steps while wv_run keeps going -- as a snapshot plan captures it -- run through n_bands biquad cascades per node,
// squared, and the squares summed and Fourier-transformed at M modulation frequencies ON THE DEVICE.  What crosses the link is
// n_bands (1 + 2 M) doubles per node when the caller asks for them, however long the run: the energy and the complex modulation sums,
// whose ratio is Schroeder's modulation transfer function (wayverb_amd/modulation.py turns it into the speech transmission index).
//
// Part of the engine behind the C ABI of include/wayverb_amd.h (engine.hip is the translation unit; see engine.hip.h for the class).
//
// The life cycle -- capture, commit, fold, checkpoint, rollback, release -- is engine_staged.hip.h's.  What is the plan's own:
//   capture   snapshot_gather_kernel (snapshot_kernels.hip.h, unchanged) -> the device-only stage float[T][B]
//   fold      modulation_fold_kernel (modulation_kernels.hip.h), one grid row per band, folds all staged captures into block 0, the
//             sums double[n_bands][1 + 2 M][B], carrying block 1, the filter states double[n_bands][n_sections][2][B].  Its twiddle
//             table double[t][M][2] is written by the host (wv_spectrum_twiddle) into one of two page-locked buffers and copied ahead
//             of the launch (TwiddleTable, engine_staged.hip.h); two, so that the host never rewrites a table a queued copy still reads.
#pragma once
#include "engine.hip.h"

namespace wv {

template <typename Real>
void Engine<Real>::Modulation::free_own() {
    if (coef) (void)hipFree(coef);
    host_table_free(tw);
}

template <typename Real>
int Engine<Real>::set_modulation(const wv_modulation_plan* plan, const double* cycles_per_step, const wv_biquad* sections, uint32_t n_bands,
                                 uint32_t n_sections) {
    DeviceGuard guard(device_);
    if (!plan) return staged_stop(mod_);
    if (const int rc = plan_refused("wv_set_modulation", kModulationRow)) return rc;
    if (!wv::decay_bands_valid(n_bands, n_sections)) return fail(WV_E_INVALID_ARGUMENT, "wv_set_modulation: n_bands must be 1 .. 8 and n_sections 1 .. 4");
    if (plan->n_freqs < 1 || plan->n_freqs > wv::kModulationMaxFreqs) return fail(WV_E_INVALID_ARGUMENT, "wv_set_modulation: n_freqs must be 1 .. 16");
    if (!cycles_per_step || !sections) return fail(WV_E_INVALID_ARGUMENT, "null argument");
    for (uint32_t m = 0; m < plan->n_freqs; ++m)
        if (!wv::frequency_valid(cycles_per_step[m]))
            return fail(WV_E_INVALID_ARGUMENT, "wv_set_modulation: a frequency outside [0, 0.5] cycles per step");
    if (!wv::biquads_finite(sections, n_bands * n_sections)) return fail(WV_E_INVALID_ARGUMENT, "wv_set_modulation: every coefficient must be finite");
    static const wv::PlanSentences says = WV_PLAN_SENTENCES("wv_set_modulation");
    if (const char* why = wv::plan_refusal(*plan, nx_, ny_, nz_, says)) return fail(WV_E_INVALID_ARGUMENT, why);
    const wv::SnapshotBox box = wv::plan_box(*plan);
    Modulation d;
    d.plan = *plan;
    d.box = box;
    d.freqs.assign(cycles_per_step, cycles_per_step + plan->n_freqs);
    d.nodes = wv::modulation_nodes(box.nx, box.ny, box.nz);
    d.gather_wide = wv::gather_wide(box);
    d.n_bands = n_bands;
    d.n_sections = n_sections;
    const size_t coef_bytes = (size_t)wv::modulation_coef_bytes(n_bands, n_sections);
    const size_t table_bytes = (size_t)wv::modulation_table_bytes(plan->n_freqs);
    static_assert(sizeof(wv_biquad) == wv::kBiquadDoubles * sizeof(double), "wv_biquad is five doubles: the coefficient table is the caller's array as it lies");
    hipError_t rc = staged_allocate(d, wv::modulation_stage_bytes(d.nodes), wv::modulation_sums_bytes(d.nodes, n_bands, plan->n_freqs),
                                    wv::modulation_state_bytes(d.nodes, n_bands, n_sections));
    if (rc == hipSuccess && (rc = hipMalloc((void**)&d.coef, coef_bytes)) != hipSuccess) d.coef = nullptr;
    if (rc == hipSuccess) rc = host_table_allocate(d.tw, table_bytes);
    if (rc == hipSuccess) rc = hipMemsetAsync(d.sums(), 0, d.block_bytes[0], stream_);  // (+0.0 everywhere)
    if (rc == hipSuccess) rc = hipMemsetAsync(d.state(), 0, d.block_bytes[1], stream_);
    if (rc == hipSuccess) rc = hipMemcpyAsync(d.coef, sections, coef_bytes, hipMemcpyHostToDevice, stream_);
    return staged_install(mod_, d, rc, "wv_set_modulation: no room for the stage, the sums and the filter states", plan->first_step, plan->period);
}

// The plan's part of a fold (staged_fold): the twiddles of the t staged captures into turn b's table, its copy, the launch.
template <typename Real>
int Engine<Real>::modulation_enqueue(Modulation& d, int b, int t, unsigned blocks) {
    int rc = twiddle_table_write(d.tw, d, b, t, d.freqs);
    if (rc || (rc = staged_fold_begins(d, b))) return rc;
    const uint32_t M = d.plan.n_freqs;
    const dim3 grid(blocks, d.n_bands);  // (blockIdx.y = the band; one node per lane)
#define WV_MODULATION_FOLD(S)                                                                                                                       \
    hipLaunchKernelGGL((wv::modulation_fold_kernel<S>), grid, dim3(256), 0, stream_, d.stage, d.state(), d.sums(), d.coef, d.tw.dev[b], d.nodes, \
                       (int32_t)M, (int32_t)t)
    switch (d.n_sections) {
        case 1: WV_MODULATION_FOLD(1); break;
        case 2: WV_MODULATION_FOLD(2); break;
        case 3: WV_MODULATION_FOLD(3); break;
        default: WV_MODULATION_FOLD(4); break;
    }
#undef WV_MODULATION_FOLD
    return WV_OK;
}

// Folds what is staged, then the planar sums -> the host: the energies as they lie, [n_bands][nz][ny][nx], and Re / Im interleaved to
// [n_bands][M][nz][ny][nx][2] there (not on the hot path).  Either destination may be NULL.  The plan keeps running.
template <typename Real>
int Engine<Real>::fetch_modulation(double* energy, double* sums, uint64_t* captures) {
    DeviceGuard guard(device_);
    Modulation& d = mod_;
    if (!d.active) return fail(WV_E_STATE, "wv_fetch_modulation: no modulation plan is set");
    const int rc = staged_settle(d);
    if (rc) return rc;
    const uint32_t M = d.plan.n_freqs;
    std::vector<double> planes(sums ? (size_t)d.nodes * 2 : 0);
    for (uint32_t k = 0; k < d.n_bands; ++k) {
        if (energy)
            WV_HIP(hipMemcpy(energy + (uint64_t)k * d.nodes, d.sums() + wv::modulation_energy_offset(d.nodes, k, M), (size_t)d.nodes * sizeof(double),
                             hipMemcpyDeviceToHost));
        for (uint32_t m = 0; m < M && sums; ++m)
            if (const int rc = fetch_interleaved(d.sums() + wv::modulation_sum_offset(d.nodes, k, m, M), d.nodes, sums + ((uint64_t)k * M + m) * 2 * d.nodes, planes)) return rc;
    }
    if (captures) *captures = d.st.folded;
    return WV_OK;
}

}  // namespace wv

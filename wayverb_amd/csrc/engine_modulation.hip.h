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
//             table double[t][M][2] is written by the host (wv_spectrum_twiddle, engine_spectrum.hip.h) into one of two page-locked
//             buffers and copied ahead of the launch; two, so that the host never rewrites a table a queued copy still reads.
#pragma once
#include <cmath>

#include "engine.hip.h"
#include "engine_spectrum.hip.h"

namespace wv {

template <typename Real>
void Engine<Real>::Modulation::free_own() {
    if (coef) (void)hipFree(coef);
    for (int i = 0; i < 2; ++i) {
        if (tw_dev[i]) (void)hipFree(tw_dev[i]);
        if (tw_host[i]) (void)hipHostFree(tw_host[i]);
    }
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
        if (!wv::modulation_frequency_valid(cycles_per_step[m]))  // (a NaN fails both comparisons)
            return fail(WV_E_INVALID_ARGUMENT, "wv_set_modulation: a frequency outside [0, 0.5] cycles per step");
    for (uint32_t i = 0; i < n_bands * n_sections; ++i) {
        const wv_biquad& c = sections[i];
        if (!std::isfinite(c.b0) || !std::isfinite(c.b1) || !std::isfinite(c.b2) || !std::isfinite(c.a1) || !std::isfinite(c.a2))
            return fail(WV_E_INVALID_ARGUMENT, "wv_set_modulation: every coefficient must be finite");
    }
    wv::SnapshotBox box;
    box.x0 = plan->x0, box.y0 = plan->y0, box.z0 = plan->z0;
    box.nx = plan->nx, box.ny = plan->ny, box.nz = plan->nz;
    box.sx = plan->sx, box.sy = plan->sy, box.sz = plan->sz;
    if (plan->sx < 1 || plan->sy < 1 || plan->sz < 1) return fail(WV_E_INVALID_ARGUMENT, "wv_set_modulation: strides must be >= 1");
    if (plan->period < 1) return fail(WV_E_INVALID_ARGUMENT, "wv_set_modulation: period must be >= 1");
    if (!wv::snapshot_box_valid(box, nx_, ny_, nz_)) return fail(WV_E_INVALID_ARGUMENT, "wv_set_modulation: the box leaves the mesh");
    // (the capture kernel indexes a dense plane with 32 bits)
    if ((uint64_t)box.nx * (uint64_t)box.ny >= (1ull << 31)) return fail(WV_E_INVALID_ARGUMENT, "wv_set_modulation: more than 2^31 nodes per plane of the box");
    Modulation d;
    d.plan = *plan;
    d.box = box;
    d.freqs.assign(cycles_per_step, cycles_per_step + plan->n_freqs);
    d.nodes = wv::modulation_nodes(box.nx, box.ny, box.nz);
    d.gather_wide = box.sx == 1 && box.x0 % 4 == 0 && box.nx % 4 == 0;  // (as engine_snapshot.hip.h decides it)
    d.n_bands = n_bands;
    d.n_sections = n_sections;
    const size_t coef_bytes = (size_t)wv::modulation_coef_bytes(n_bands, n_sections);
    const size_t table_bytes = (size_t)wv::modulation_table_bytes(plan->n_freqs);
    static_assert(sizeof(wv_biquad) == wv::kBiquadDoubles * sizeof(double), "wv_biquad is five doubles: the coefficient table is the caller's array as it lies");
    hipError_t rc = staged_allocate(d, wv::modulation_stage_bytes(d.nodes), wv::modulation_sums_bytes(d.nodes, n_bands, plan->n_freqs),
                                    wv::modulation_state_bytes(d.nodes, n_bands, n_sections));
    if (rc == hipSuccess && (rc = hipMalloc((void**)&d.coef, coef_bytes)) != hipSuccess) d.coef = nullptr;
    for (int i = 0; i < 2 && rc == hipSuccess; ++i) {
        if ((rc = hipMalloc((void**)&d.tw_dev[i], table_bytes)) != hipSuccess) {
            d.tw_dev[i] = nullptr;
            break;
        }
        if ((rc = hipHostMalloc((void**)&d.tw_host[i], table_bytes, hipHostMallocDefault)) != hipSuccess) d.tw_host[i] = nullptr;
    }
    if (rc == hipSuccess) rc = hipMemsetAsync(d.sums(), 0, d.block_bytes[0], stream_);  // (+0.0 everywhere)
    if (rc == hipSuccess) rc = hipMemsetAsync(d.state(), 0, d.block_bytes[1], stream_);
    if (rc == hipSuccess) rc = hipMemcpyAsync(d.coef, sections, coef_bytes, hipMemcpyHostToDevice, stream_);
    return staged_install(mod_, d, rc, "wv_set_modulation: no room for the stage, the sums and the filter states", plan->first_step, plan->period);
}

// The plan's part of a fold (staged_fold): the twiddles of the t staged captures into turn b's table, its copy, the launch.
template <typename Real>
int Engine<Real>::modulation_enqueue(Modulation& d, int b, int t, unsigned blocks) {
    const uint32_t M = d.plan.n_freqs;
    for (int j = 0; j < t; ++j)
        for (uint32_t m = 0; m < M; ++m) {
            double* w = d.tw_host[b] + wv::modulation_table_index((uint32_t)j, m, M);
            wv::spectrum_twiddle(d.freqs[m], d.st.steps[(size_t)j], w, w + 1);
        }
    WV_HIP(hipMemcpyAsync(d.tw_dev[b], d.tw_host[b], (size_t)t * M * 2 * sizeof(double), hipMemcpyHostToDevice, stream_));
    const int rc = staged_fold_begins(d, b);
    if (rc) return rc;
    const dim3 grid(blocks, d.n_bands);  // (blockIdx.y = the band; one node per lane)
#define WV_MODULATION_FOLD(S)                                                                                                                       \
    hipLaunchKernelGGL((wv::modulation_fold_kernel<S>), grid, dim3(256), 0, stream_, d.stage, d.state(), d.sums(), d.coef, d.tw_dev[b], d.nodes, \
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

template <typename Real>
int Engine<Real>::modulation_count(uint64_t* captures, uint64_t* last_step) {
    return staged_count(mod_, captures, last_step);
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
        for (uint32_t m = 0; m < M && sums; ++m) {
            WV_HIP(hipMemcpy(planes.data(), d.sums() + wv::modulation_sum_offset(d.nodes, k, m, M), planes.size() * sizeof(double), hipMemcpyDeviceToHost));
            double* out = sums + ((uint64_t)k * M + m) * 2 * d.nodes;
            const double *re = planes.data(), *im = planes.data() + d.nodes;
            for (uint64_t i = 0; i < d.nodes; ++i) {
                out[2 * i] = re[i];
                out[2 * i + 1] = im[i];
            }
        }
    }
    if (captures) *captures = d.st.folded;
    return WV_OK;
}

}  // namespace wv

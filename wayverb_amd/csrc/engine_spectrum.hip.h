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
//             and copied ahead of the launch; two, so that the host never rewrites a table a queued copy still reads.
#pragma once
#include <cmath>

#include "engine.hip.h"

namespace wv {

// x = f * step, its fractional part, cos and sin of 2 pi x: three rounded operations ahead of libm, so that NumPy evaluating the
// same three gives the same argument (include/wayverb_amd.h: wv_spectrum_twiddle)
inline void spectrum_twiddle(double cycles_per_step, uint64_t step, double* c, double* s) {
    double x = cycles_per_step * (double)step;
    x -= std::floor(x);
    const double angle = 6.283185307179586476925286766559 * x;
    *c = std::cos(angle);
    *s = std::sin(angle);
}

template <typename Real>
void Engine<Real>::Spectrum::free_own() {
    for (int i = 0; i < 2; ++i) {
        if (tw_dev[i]) (void)hipFree(tw_dev[i]);
        if (tw_host[i]) (void)hipHostFree(tw_host[i]);
    }
}

template <typename Real>
int Engine<Real>::set_spectrum(const wv_spectrum_plan* plan, const double* cycles_per_step) {
    DeviceGuard guard(device_);
    if (!plan) return staged_stop(spec_);
    if (const int rc = plan_refused("wv_set_spectrum", kSpectrumRow)) return rc;
    if (plan->n_freqs < 1 || plan->n_freqs > wv::kSpectrumMaxFreqs) return fail(WV_E_INVALID_ARGUMENT, "wv_set_spectrum: n_freqs must be 1 .. 64");
    if (!cycles_per_step) return fail(WV_E_INVALID_ARGUMENT, "null argument");
    for (uint32_t k = 0; k < plan->n_freqs; ++k)
        if (!(cycles_per_step[k] >= 0.0 && cycles_per_step[k] <= 0.5))  // (a NaN fails both comparisons)
            return fail(WV_E_INVALID_ARGUMENT, "wv_set_spectrum: a frequency outside [0, 0.5] cycles per step");
    wv::SnapshotBox box;
    box.x0 = plan->x0, box.y0 = plan->y0, box.z0 = plan->z0;
    box.nx = plan->nx, box.ny = plan->ny, box.nz = plan->nz;
    box.sx = plan->sx, box.sy = plan->sy, box.sz = plan->sz;
    if (plan->sx < 1 || plan->sy < 1 || plan->sz < 1) return fail(WV_E_INVALID_ARGUMENT, "wv_set_spectrum: strides must be >= 1");
    if (plan->period < 1) return fail(WV_E_INVALID_ARGUMENT, "wv_set_spectrum: period must be >= 1");
    if (!wv::snapshot_box_valid(box, nx_, ny_, nz_)) return fail(WV_E_INVALID_ARGUMENT, "wv_set_spectrum: the box leaves the mesh");
    // (the capture kernel indexes a dense plane with 32 bits)
    if ((uint64_t)box.nx * (uint64_t)box.ny >= (1ull << 31)) return fail(WV_E_INVALID_ARGUMENT, "wv_set_spectrum: more than 2^31 nodes per plane of the box");
    Spectrum s;
    s.plan = *plan;
    s.box = box;
    s.freqs.assign(cycles_per_step, cycles_per_step + plan->n_freqs);
    s.nodes = wv::spectrum_nodes(box.nx, box.ny, box.nz);
    s.gather_wide = box.sx == 1 && box.x0 % 4 == 0 && box.nx % 4 == 0;  // (as engine_snapshot.hip.h decides it)
    s.fold_wide = s.nodes % 2 == 0;                                      // two nodes per lane, 16-byte accesses on the sums
    const size_t table_bytes = (size_t)wv::spectrum_table_bytes(plan->n_freqs);
    hipError_t rc = staged_allocate(s, wv::spectrum_stage_bytes(s.nodes), wv::spectrum_sum_bytes(s.nodes, plan->n_freqs));
    for (int i = 0; i < 2 && rc == hipSuccess; ++i) {
        if ((rc = hipMalloc((void**)&s.tw_dev[i], table_bytes)) != hipSuccess) {
            s.tw_dev[i] = nullptr;
            break;
        }
        if ((rc = hipHostMalloc((void**)&s.tw_host[i], table_bytes, hipHostMallocDefault)) != hipSuccess) s.tw_host[i] = nullptr;
    }
    if (rc == hipSuccess) rc = hipMemsetAsync(s.acc(), 0, s.block_bytes[0], stream_);  // (+0.0 everywhere)
    return staged_install(spec_, s, rc, "wv_set_spectrum: no room for the stage and the sums", plan->first_step, plan->period);
}

// The spectrum's part of a fold (staged_fold): the twiddles of the t staged captures into turn b's table, its copy, the launch.
template <typename Real>
int Engine<Real>::spectrum_enqueue(Spectrum& s, int b, int t, unsigned blocks) {
    const uint32_t K = s.plan.n_freqs;
    for (int j = 0; j < t; ++j)
        for (uint32_t k = 0; k < K; ++k) {
            double* w = s.tw_host[b] + wv::spectrum_table_index((uint32_t)j, k, K);
            wv::spectrum_twiddle(s.freqs[k], s.st.steps[(size_t)j], w, w + 1);
        }
    WV_HIP(hipMemcpyAsync(s.tw_dev[b], s.tw_host[b], (size_t)t * K * 2 * sizeof(double), hipMemcpyHostToDevice, stream_));
    const int rc = staged_fold_begins(s, b);
    if (rc) return rc;
    if (s.fold_wide)
        hipLaunchKernelGGL((wv::spectrum_fold_kernel<true>), dim3(blocks), dim3(256), 0, stream_, s.stage, s.acc(), s.tw_dev[b], s.nodes, (int32_t)t, (int32_t)K);
    else
        hipLaunchKernelGGL((wv::spectrum_fold_kernel<false>), dim3(blocks), dim3(256), 0, stream_, s.stage, s.acc(), s.tw_dev[b], s.nodes, (int32_t)t, (int32_t)K);
    return WV_OK;
}

template <typename Real>
int Engine<Real>::spectrum_count(uint64_t* captures, uint64_t* last_step) {
    return staged_count(spec_, captures, last_step);
}

// Folds what is staged, then the planar sums -> the host, interleaved to [K][nz][ny][nx][2] there (not on the hot path).  The plan
// keeps running.
template <typename Real>
int Engine<Real>::fetch_spectrum(double* dst, uint64_t* captures) {
    DeviceGuard guard(device_);
    Spectrum& s = spec_;
    if (!s.active) return fail(WV_E_STATE, "wv_fetch_spectrum: no spectrum plan is set");
    if (!dst) return fail(WV_E_INVALID_ARGUMENT, "null argument");
    const int rc = staged_settle(s);
    if (rc) return rc;
    std::vector<double> planes((size_t)s.nodes * 2);
    for (uint32_t k = 0; k < s.plan.n_freqs; ++k) {
        WV_HIP(hipMemcpy(planes.data(), s.acc() + (uint64_t)k * 2 * s.nodes, planes.size() * sizeof(double), hipMemcpyDeviceToHost));
        double* out = dst + (uint64_t)k * 2 * s.nodes;
        const double *re = planes.data(), *im = planes.data() + s.nodes;
        for (uint64_t i = 0; i < s.nodes; ++i) {
            out[2 * i] = re[i];
            out[2 * i + 1] = im[i];
        }
    }
    if (captures) *captures = s.st.folded;
    return WV_OK;
}

}  // namespace wv

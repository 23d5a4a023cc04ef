// engine_intensity.hip.h -- wv_set_intensity / wv_intensity_count / wv_fetch_intensity / wv_fetch_intensity_velocity: a box of the
// field, decimated, captured every `period` steps while wv_run keeps going, the reference's directional_receiver integrator
// (src/waveguide/src/postprocessor/directional_receiver.cpp:29-69) run at every node taken and the intensity I = p v, with the
// squared pressure beside it, summed per node into time bins ON THE DEVICE.  What crosses the link is 4 n_bins doubles per node when
// the caller asks for them, however long the run (wayverb_amd/intensity.py turns them into directions and diffuseness).
//
// Part of the engine behind the C ABI of include/wayverb_amd.h (engine.hip is the translation unit; see engine.hip.h for the class).
//
// The life cycle -- capture, commit, fold, checkpoint, rollback, release -- is engine_staged.hip.h's.  What is the intensity plan's own:
//   capture   intensity_gather_kernel (intensity_kernels.hip.h) -> the device-only stage float[T][4][B] (pressure and the three float
//             gradient differences of every node taken)
//   fold      intensity_fold_kernel folds all staged captures, in order, into the velocities double[3][B] and the bins
//             double[4][n_bins][B].  The bins of the t staged captures, int32[t], are written by the host (decay_plan.h: decay_bin)
//             into one of two page-locked tables and copied ahead of the launch, as the decay plan's are (BinTable).
// The velocities are only ever touched by a fold, and a fold only ever sees committed captures: after a stop on a flag they have seen
// exactly the captures the bins hold.
#pragma once
#include "engine.hip.h"

namespace wv {

template <typename Real>
void Engine<Real>::Intensity::free_own() {
    host_table_free(table);
}

template <typename Real>
int Engine<Real>::set_intensity(const wv_intensity_plan* plan) {
    DeviceGuard guard(device_);
    if (!plan) return staged_stop(inten_);
    if (const int rc = plan_refused("wv_set_intensity", kIntensityRow)) return rc;
    const char* why = nullptr;
    if (wv::intensity_plan_check(*plan, nx_, ny_, nz_, &why)) return fail(WV_E_INVALID_ARGUMENT, why);
    Intensity d;
    d.plan = *plan;
    d.box = wv::plan_box(*plan);
    d.spacing = plan->spacing;
    d.nodes = wv::decay_nodes(d.box.nx, d.box.ny, d.box.nz);
    d.k = plan->ambient_density * plan->sample_rate;
    hipError_t rc = staged_allocate(d, wv::intensity_stage_bytes(d.nodes), wv::intensity_bins_bytes(d.nodes, plan->n_bins), wv::intensity_velocity_bytes(d.nodes));
    if (rc == hipSuccess) rc = host_table_allocate(d.table, (size_t)wv::decay_table_bytes());
    if (rc == hipSuccess) rc = hipMemsetAsync(d.bins(), 0, d.block_bytes[0], stream_);  // (+0.0 everywhere)
    if (rc == hipSuccess) rc = hipMemsetAsync(d.velocity(), 0, d.block_bytes[1], stream_);
    return staged_install(inten_, d, rc, "wv_set_intensity: no room for the stage, the velocities and the bins", plan->first_step, plan->period);
}

// The intensity plan's part of a fold (staged_fold): the bins of the t staged captures into turn b's table, its copy, the launch.
template <typename Real>
int Engine<Real>::intensity_enqueue(Intensity& d, int b, int t, unsigned blocks) {
    int rc = bin_table_write(d.table, d, b, t, d.plan.bin_captures, d.plan.n_bins);
    if (rc || (rc = staged_fold_begins(d, b))) return rc;
    hipLaunchKernelGGL(wv::intensity_fold_kernel, dim3(blocks), dim3(256), 0, stream_, d.stage, d.velocity(), d.bins(), d.table.dev[b], d.nodes,
                       d.plan.n_bins, d.k, (int32_t)t);
    return WV_OK;
}

// Folds what is staged, then the bins -> the host as they lie: [4][n_bins][nz][ny][nx].  The plan keeps running.
template <typename Real>
int Engine<Real>::fetch_intensity(double* dst, uint64_t* captures) {
    DeviceGuard guard(device_);
    Intensity& d = inten_;
    if (!d.active) return fail(WV_E_STATE, "wv_fetch_intensity: no intensity plan is set");
    if (!dst) return fail(WV_E_INVALID_ARGUMENT, "null argument");
    const int rc = staged_settle(d);
    if (rc) return rc;
    WV_HIP(hipMemcpy(dst, d.bins(), d.block_bytes[0], hipMemcpyDeviceToHost));
    if (captures) *captures = d.st.folded;
    return WV_OK;
}

// ... and the velocities the integrator carries, [3][nz][ny][nx], behind the same fold.
template <typename Real>
int Engine<Real>::fetch_intensity_velocity(double* dst) {
    DeviceGuard guard(device_);
    Intensity& d = inten_;
    if (!d.active) return fail(WV_E_STATE, "wv_fetch_intensity_velocity: no intensity plan is set");
    if (!dst) return fail(WV_E_INVALID_ARGUMENT, "null argument");
    const int rc = staged_fold(d);
    if (rc) return rc;
    WV_HIP(hipStreamSynchronize(stream_));
    WV_HIP(hipMemcpy(dst, d.velocity(), d.block_bytes[1], hipMemcpyDeviceToHost));
    return WV_OK;
}

}  // namespace wv

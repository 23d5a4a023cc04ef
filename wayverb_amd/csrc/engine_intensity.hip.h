// engine_intensity.hip.h -- wv_set_intensity / wv_intensity_count / wv_fetch_intensity / wv_fetch_intensity_velocity: a box of the
// field, decimated, captured every `period` steps while wv_run keeps going, the reference's directional_receiver integrator
// (src/waveguide/src/postprocessor/directional_receiver.cpp:29-69) run at every node taken and the intensity I = p v, with the
// squared pressure beside it, summed per node into time bins ON THE DEVICE.  What crosses the link is 4 n_bins doubles per node when
// the caller asks for them, however long the run (wayverb_amd/intensity.py turns them into directions and diffuseness).
//
// Part of the engine behind the C ABI of include/wayverb_amd.h (engine.hip is the translation unit; see engine.hip.h for the class).
//
// The life cycle is engine_decay.hip.h's, on the same stage bookkeeping (capture_stage.h); everything runs on the compute stream:
//   capture   intensity_gather_kernel (intensity_kernels.hip.h) -> the next free slot of the device-only stage float[T][4][B]
//             (pressure and the three float gradient differences of every node taken), directly behind the pass that produced the
//             step (engine_batch.hip.h cuts batches and segments at whichever plan is active: they exclude each other)
//   commit    a batch's captures stay staged until commit_batch has said how many of its steps were good (CaptureStage::commit)
//   fold      intensity_fold_kernel folds all staged captures, in order, into the velocities double[3][B] and the bins
//             double[4][n_bins][B] in ONE launch, and only when the stage has no slot left for the next batch -- or on fetch and
//             checkpoint.  The bins of the t staged captures, int32[t], are written by the host (decay_plan.h: decay_bin) into one of
//             two page-locked tables and copied ahead of the launch, as the decay plan's are.
// The velocities are only ever touched by a fold, and a fold only ever sees committed captures: after a stop on a flag they have seen
// exactly the captures the bins hold.
#pragma once
#include "engine.hip.h"

namespace wv {

static_assert(kIntensityStage == kSpectrumStage, "the intensity plan stages its captures by spectrum_plan.h's rules");

template <typename Real>
void Engine<Real>::intensity_release(Intensity& d) {
    if (d.stage) (void)hipFree(d.stage);
    if (d.bins) (void)hipFree(d.bins);
    if (d.velocity) (void)hipFree(d.velocity);
    for (int i = 0; i < 2; ++i) {
        if (d.table_dev[i]) (void)hipFree(d.table_dev[i]);
        if (d.table_host[i]) (void)hipHostFree(d.table_host[i]);
        if (d.begun[i]) (void)hipEventDestroy(d.begun[i]);
        if (d.folded_ev[i]) (void)hipEventDestroy(d.folded_ev[i]);
    }
    for (int i = 0; i < kIntensityStage; ++i) {
        if (d.gather_begun[i]) (void)hipEventDestroy(d.gather_begun[i]);
        if (d.gather_done[i]) (void)hipEventDestroy(d.gather_done[i]);
    }
    const uint64_t generation = d.generation;
    d = Intensity{};
    d.generation = generation;
}

template <typename Real>
int Engine<Real>::set_intensity(const wv_intensity_plan* plan) {
    DeviceGuard guard(device_);
    if (!plan) {
        WV_HIP(hipStreamSynchronize(stream_));
        intensity_release(inten_);
        ++inten_.generation;
        return WV_OK;
    }
    // (the snapshot plan's reason: a slab would have to cut its batches where its neighbours do, and holds only its part of a box)
    if (opt_.ghost_lo || opt_.ghost_hi || (comm_ && comm_->nranks() > 1))
        return fail(WV_E_STATE, "wv_set_intensity: not on a slab of a chain (one domain only)");
    // every plan wants to decide where passes end: one consumer of capture steps at a time
    if (snap_.active) return fail(WV_E_STATE, "wv_set_intensity: a snapshot plan is active (wv_set_snapshots(e, NULL) stops it); the plans exclude each other");
    if (spec_.active) return fail(WV_E_STATE, "wv_set_intensity: a spectrum plan is active (wv_set_spectrum(e, NULL, NULL) stops it); the plans exclude each other");
    if (decay_.active && decay_.n_bands)
        return fail(WV_E_STATE, "wv_set_intensity: a banded decay plan is active (wv_set_decay_bands(e, NULL, NULL, 0, 0) stops it); the plans exclude each other");
    if (decay_.active) return fail(WV_E_STATE, "wv_set_intensity: a decay plan is active (wv_set_decay(e, NULL) stops it); the plans exclude each other");
    if (arr_.active) return fail(WV_E_STATE, "wv_set_intensity: an arrival plan is active (wv_set_arrival(e, NULL, NULL) stops it); the plans exclude each other");
    if (lat_.active) return fail(WV_E_STATE, "wv_set_intensity: a lateral plan is active (wv_set_lateral(e, NULL, NULL) stops it); the plans exclude each other");
    const char* why = nullptr;
    if (wv::intensity_plan_check(*plan, nx_, ny_, nz_, &why)) return fail(WV_E_INVALID_ARGUMENT, why);
    // everything is allocated here, aside, and only a complete set takes the old plan's place: no room -> WV_E_HIP, engine untouched
    Intensity d;
    d.generation = inten_.generation + 1;
    d.plan = *plan;
    d.box = wv::intensity_box(*plan);
    d.nodes = wv::decay_nodes(d.box.nx, d.box.ny, d.box.nz);
    d.k = plan->ambient_density * plan->sample_rate;
    const uint64_t stage_bytes = wv::intensity_stage_bytes(d.nodes);
    const uint64_t bins_bytes = wv::intensity_bins_bytes(d.nodes, plan->n_bins);
    const uint64_t velocity_bytes = wv::intensity_velocity_bytes(d.nodes);
    const size_t table_bytes = (size_t)wv::decay_table_bytes();
    const uint64_t most = std::numeric_limits<size_t>::max() / 2;
    hipError_t rc = hipSuccess;
    if (stage_bytes == wv::kDecayNoSize || bins_bytes == wv::kDecayNoSize || velocity_bytes == wv::kDecayNoSize || stage_bytes > most || bins_bytes > most)
        rc = hipErrorOutOfMemory;
    if (rc == hipSuccess && (rc = hipMalloc((void**)&d.stage, (size_t)stage_bytes)) != hipSuccess) d.stage = nullptr;
    if (rc == hipSuccess && (rc = hipMalloc((void**)&d.bins, (size_t)bins_bytes)) != hipSuccess) d.bins = nullptr;
    if (rc == hipSuccess && (rc = hipMalloc((void**)&d.velocity, (size_t)velocity_bytes)) != hipSuccess) d.velocity = nullptr;
    for (int i = 0; i < 2 && rc == hipSuccess; ++i) {
        if ((rc = hipMalloc((void**)&d.table_dev[i], table_bytes)) != hipSuccess) {
            d.table_dev[i] = nullptr;
            break;
        }
        if ((rc = hipHostMalloc((void**)&d.table_host[i], table_bytes, hipHostMallocDefault)) != hipSuccess) {
            d.table_host[i] = nullptr;
            break;
        }
        if ((rc = hipEventCreate(&d.begun[i])) != hipSuccess) break;
        if ((rc = hipEventCreate(&d.folded_ev[i])) != hipSuccess) break;
    }
    for (int i = 0; i < kIntensityStage && rc == hipSuccess; ++i) {
        if ((rc = hipEventCreate(&d.gather_begun[i])) != hipSuccess) break;
        if ((rc = hipEventCreate(&d.gather_done[i])) != hipSuccess) break;
    }
    if (rc == hipSuccess) rc = hipMemsetAsync(d.bins, 0, (size_t)bins_bytes, stream_);  // (+0.0 everywhere)
    if (rc == hipSuccess) rc = hipMemsetAsync(d.velocity, 0, (size_t)velocity_bytes, stream_);
    if (rc == hipSuccess) rc = hipStreamSynchronize(stream_);
    if (rc != hipSuccess) {
        (void)hipGetLastError();  // nothing sticky
        intensity_release(d);
        wv::note_hip_error(rc);
        return fail(WV_E_HIP, std::string("wv_set_intensity: no room for the stage, the velocities and the bins: ") + hipGetErrorString(rc));
    }
    intensity_release(inten_);
    inten_ = std::move(d);
    inten_.st.start(plan->first_step, plan->period, steps_done);
    inten_.active = true;
    return WV_OK;
}

// The capture of `step`, which the field `current` holds once everything enqueued on the compute stream so far has run: into the
// slot behind the ones staged.
template <typename Real>
int Engine<Real>::intensity_capture(uint64_t step) {
    Intensity& d = inten_;
    // (intensity_plan_batch gives a batch no more captures than the stage has free slots)
    if (d.st.full()) return fail(WV_E_STATE, "wv_run: the intensity stage is full");
    const int slot = d.st.slot();
    if (timing) WV_HIP(hipEventRecord(d.gather_begun[slot], stream_));
    const int rc = launch_intensity_gather(d.box, d.plan.spacing, d.stage + (uint64_t)slot * wv::kIntensityPlanes * d.nodes);
    if (rc) return rc;
    if (timing) {
        WV_HIP(hipEventRecord(d.gather_done[slot], stream_));
        d.gather_timed[slot] = true;
    }
    d.st.staged(step);
    return WV_OK;
}

// The times of the folds that used table `table` (-1: either) and of the captures, where they ran with kernel timing on, once they
// have run.
template <typename Real>
int Engine<Real>::intensity_drain_timing(int table) {
    Intensity& d = inten_;
    for (int b = 0; b < 2; ++b) {
        if (!d.timed[b] || (table >= 0 && b != table)) continue;
        WV_HIP(hipEventSynchronize(d.folded_ev[b]));
        float ms = 0;
        WV_HIP(hipEventElapsedTime(&ms, d.begun[b], d.folded_ev[b]));
        d.kernel_ms += ms;
        d.timed[b] = false;
    }
    for (int i = 0; i < kIntensityStage; ++i) {
        if (!d.gather_timed[i]) continue;
        WV_HIP(hipEventSynchronize(d.gather_done[i]));
        float ms = 0;
        WV_HIP(hipEventElapsedTime(&ms, d.gather_begun[i], d.gather_done[i]));
        d.gather_ms += ms;
        ++d.gathers_timed;
        d.gather_timed[i] = false;
    }
    return WV_OK;
}

// All committed captures -> velocities and bins, one launch.  Only between batches, where nothing uncommitted is staged -- but for
// what a failed run left, which goes first: the stage is filled from slot 0 again behind a fold.
template <typename Real>
int Engine<Real>::intensity_fold() {
    Intensity& d = inten_;
    d.st.drop_uncommitted();
    const int t = d.st.committed;
    if (t == 0) return WV_OK;
    const int b = d.table;
    // the fold before last used this table: its copy has long left the host's (a wait only if the device is two folds behind)
    if (d.table_used[b]) WV_HIP(hipEventSynchronize(d.folded_ev[b]));
    // (the slots' event pairs are recorded again by the captures behind this fold)
    int rc = intensity_drain_timing(b);
    if (rc) return rc;
    // staged capture j is capture number folded + j since the plan was set
    for (int j = 0; j < t; ++j) d.table_host[b][j] = (int32_t)wv::decay_bin(d.st.folded + (uint64_t)j, d.plan.bin_captures, d.plan.n_bins);
    WV_HIP(hipMemcpyAsync(d.table_dev[b], d.table_host[b], (size_t)t * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
    const uint64_t blocks = (d.nodes + 255) / 256;
    if (blocks > 0x7fffffffull) return fail(WV_E_STATE, "wv_set_intensity: the box has more nodes than one launch covers");
    if (timing) {
        WV_HIP(hipEventRecord(d.begun[b], stream_));
        d.timed[b] = true;
    }
    hipLaunchKernelGGL(wv::intensity_fold_kernel, dim3((unsigned)blocks), dim3(256), 0, stream_, d.stage, d.velocity, d.bins, d.table_dev[b], d.nodes,
                       d.plan.n_bins, d.k, (int32_t)t);
    WV_HIP(hipGetLastError());
    WV_HIP(hipEventRecord(d.folded_ev[b], stream_));
    d.table_used[b] = true;
    d.table = 1 - b;
    ++d.folds;
    d.st.all_folded();
    return WV_OK;
}

// Before a batch is planned: the fold when the stage has no slot left, and where the batch ends at the latest.
template <typename Real>
int Engine<Real>::intensity_plan_batch() {
    Intensity& d = inten_;
    if (d.st.fold_due()) {
        const int rc = intensity_fold();
        if (rc) return rc;
    }
    d.st.plan_batch_end(opt_.tuning.graph != 0);
    return WV_OK;
}

// On entering wv_run: steps taken by wv_step / wv_swap capture nothing, so plan steps they passed are passed; a capture of the step
// the engine stands at is due now (and is of a completed step: committed at once).
template <typename Real>
int Engine<Real>::intensity_begin_run() {
    Intensity& d = inten_;
    if (d.st.begin_run(steps_done)) {
        int rc = d.st.fold_due() ? intensity_fold() : WV_OK;
        if (rc) return rc;
        if ((rc = intensity_capture(steps_done))) return rc;
        d.st.commit(steps_done);
    }
    return WV_OK;
}

// wv_checkpoint under a plan: bins and velocities (everything staged folded in first), the count and the next plan step aside; the
// copies are allocated by the first checkpoint taken under the plan.  Called before the checkpoint touches anything: no room ->
// WV_E_HIP, engine untouched.
template <typename Real>
int Engine<Real>::intensity_checkpoint() {
    Intensity& d = inten_;
    const size_t bytes = (size_t)wv::intensity_bins_bytes(d.nodes, d.plan.n_bins);
    const size_t velocity_bytes = (size_t)wv::intensity_velocity_bytes(d.nodes);
    if (!ckpt_.inten_velocity || ckpt_.inten_velocity_bytes != velocity_bytes) {
        if (ckpt_.inten_velocity) (void)hipFree(ckpt_.inten_velocity);
        ckpt_.inten_velocity = nullptr;
        ckpt_.inten_velocity_bytes = 0;
        const hipError_t rc = hipMalloc((void**)&ckpt_.inten_velocity, velocity_bytes);
        if (rc != hipSuccess) {
            ckpt_.inten_velocity = nullptr;
            (void)hipGetLastError();
            return fail(WV_E_HIP, std::string("wv_checkpoint: no room for a copy of the intensity plan's velocities: ") + hipGetErrorString(rc));
        }
        ckpt_.inten_velocity_bytes = velocity_bytes;
    }
    if (!ckpt_.inten_bins || ckpt_.inten_bytes != bytes) {
        if (ckpt_.inten_bins) (void)hipFree(ckpt_.inten_bins);
        ckpt_.inten_bins = nullptr;
        ckpt_.inten_bytes = 0;
        const hipError_t rc = hipMalloc((void**)&ckpt_.inten_bins, bytes);
        if (rc != hipSuccess) {
            ckpt_.inten_bins = nullptr;
            (void)hipGetLastError();
            return fail(WV_E_HIP, std::string("wv_checkpoint: no room for a copy of the intensity plan's bins: ") + hipGetErrorString(rc));
        }
        ckpt_.inten_bytes = bytes;
    }
    const int rc = intensity_fold();
    if (rc) return rc;
    WV_HIP(hipMemcpyAsync(ckpt_.inten_bins, d.bins, bytes, hipMemcpyDeviceToDevice, stream_));
    WV_HIP(hipMemcpyAsync(ckpt_.inten_velocity, d.velocity, velocity_bytes, hipMemcpyDeviceToDevice, stream_));
    ckpt_.inten_captures = d.st.folded;
    ckpt_.inten_last_step = d.st.last_step;
    ckpt_.inten_next = d.st.next;
    return WV_OK;
}

// wv_rollback (the plan is the one the checkpoint saw): bins, velocities and count back, what is staged forgotten; the re-run takes
// it again.
template <typename Real>
int Engine<Real>::intensity_rollback() {
    Intensity& d = inten_;
    WV_HIP(hipMemcpyAsync(d.bins, ckpt_.inten_bins, ckpt_.inten_bytes, hipMemcpyDeviceToDevice, stream_));
    WV_HIP(hipMemcpyAsync(d.velocity, ckpt_.inten_velocity, ckpt_.inten_velocity_bytes, hipMemcpyDeviceToDevice, stream_));
    d.st.rollback(ckpt_.inten_captures, ckpt_.inten_last_step, ckpt_.inten_next);
    return WV_OK;
}

template <typename Real>
int Engine<Real>::intensity_count(uint64_t* captures, uint64_t* last_step) {
    if (!inten_.active) return fail(WV_E_STATE, "wv_intensity_count: no intensity plan is set");
    if (captures) *captures = inten_.st.captures();
    if (last_step) *last_step = inten_.st.last_step;
    return WV_OK;
}

// Folds what is staged, then the bins -> the host as they lie: [4][n_bins][nz][ny][nx].  The plan keeps running.
template <typename Real>
int Engine<Real>::fetch_intensity(double* dst, uint64_t* captures) {
    DeviceGuard guard(device_);
    Intensity& d = inten_;
    if (!d.active) return fail(WV_E_STATE, "wv_fetch_intensity: no intensity plan is set");
    if (!dst) return fail(WV_E_INVALID_ARGUMENT, "null argument");
    int rc = intensity_fold();
    if (rc) return rc;
    WV_HIP(hipStreamSynchronize(stream_));
    if ((rc = intensity_drain_timing())) return rc;
    WV_HIP(hipMemcpy(dst, d.bins, (size_t)wv::intensity_bins_bytes(d.nodes, d.plan.n_bins), hipMemcpyDeviceToHost));
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
    const int rc = intensity_fold();
    if (rc) return rc;
    WV_HIP(hipStreamSynchronize(stream_));
    WV_HIP(hipMemcpy(dst, d.velocity, (size_t)wv::intensity_velocity_bytes(d.nodes), hipMemcpyDeviceToHost));
    return WV_OK;
}

}  // namespace wv

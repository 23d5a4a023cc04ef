// engine_lateral.hip.h -- wv_set_lateral / wv_lateral_count / wv_fetch_lateral: a box of the field, decimated, captured every `period`
// steps while wv_run keeps going -- as an intensity plan captures it -- the reference's directional_receiver integrator
// (src/waveguide/src/postprocessor/directional_receiver.cpp:29-69) run at every node taken and, per node and ON THE DEVICE, the
// capture at which the direct sound arrived and p^2, p v and the second-moment tensor v v^T summed into bins counted from the node's
// OWN arrival.  What crosses the link is 36 + 80 n_bins bytes per node when the caller asks for them, however long the run
// (wayverb_amd/lateral.py turns them into the early lateral energy fraction, the direct direction and the diffuseness).
//
// Part of the engine behind the C ABI of include/wayverb_amd.h (engine.hip is the translation unit; see engine.hip.h for the class).
//
// The life cycle is engine_arrival.hip.h's, on the same stage bookkeeping (capture_stage.h); everything runs on the compute stream:
//   capture   intensity_gather_kernel (intensity_kernels.hip.h, unchanged) -> the next free slot of the device-only stage
//             float[T][4][B], directly behind the pass that produced the step (engine_batch.hip.h cuts batches and segments at
//             whichever plan is active: they exclude each other)
//   commit    a batch's captures stay staged until commit_batch has said how many of its steps were good (CaptureStage::commit)
//   fold      lateral_fold_kernel (lateral_kernels.hip.h) folds all staged captures, in order, into the per-node state in ONE launch,
//             and only when the stage has no slot left for the next batch -- or on fetch and checkpoint.  Which bin a capture goes to
//             differs from node to node, so there is no table for the host to write: the edge table and the number of the first
//             staged capture are kernel arguments.
// The state is only ever touched by a fold, and a fold only ever sees committed captures: after a stop on a flag no onset, velocity
// or sum is of a step that was never completed.
#pragma once
#include "engine.hip.h"

namespace wv {

static_assert(kLateralStage == kSpectrumStage, "the lateral plan stages its captures by spectrum_plan.h's rules");

template <typename Real>
void Engine<Real>::lateral_release(Lateral& d) {
    if (d.stage) (void)hipFree(d.stage);
    if (d.state) (void)hipFree(d.state);
    if (d.threshold_map) (void)hipFree(d.threshold_map);
    for (int i = 0; i < 2; ++i) {
        if (d.begun[i]) (void)hipEventDestroy(d.begun[i]);
        if (d.folded_ev[i]) (void)hipEventDestroy(d.folded_ev[i]);
    }
    for (int i = 0; i < kLateralStage; ++i) {
        if (d.gather_begun[i]) (void)hipEventDestroy(d.gather_begun[i]);
        if (d.gather_done[i]) (void)hipEventDestroy(d.gather_done[i]);
    }
    const uint64_t generation = d.generation;
    d = Lateral{};
    d.generation = generation;
}

template <typename Real>
int Engine<Real>::set_lateral(const wv_lateral_plan* plan, const float* threshold_map) {
    DeviceGuard guard(device_);
    if (!plan) {
        WV_HIP(hipStreamSynchronize(stream_));
        lateral_release(lat_);
        ++lat_.generation;
        return WV_OK;
    }
    // (the snapshot plan's reason: a slab would have to cut its batches where its neighbours do, and holds only its part of a box)
    if (opt_.ghost_lo || opt_.ghost_hi || (comm_ && comm_->nranks() > 1))
        return fail(WV_E_STATE, "wv_set_lateral: not on a slab of a chain (one domain only)");
    // every plan wants to decide where passes end: one consumer of capture steps at a time
    if (snap_.active) return fail(WV_E_STATE, "wv_set_lateral: a snapshot plan is active (wv_set_snapshots(e, NULL) stops it); the plans exclude each other");
    if (spec_.active) return fail(WV_E_STATE, "wv_set_lateral: a spectrum plan is active (wv_set_spectrum(e, NULL, NULL) stops it); the plans exclude each other");
    if (decay_.active && decay_.n_bands)
        return fail(WV_E_STATE, "wv_set_lateral: a banded decay plan is active (wv_set_decay_bands(e, NULL, NULL, 0, 0) stops it); the plans exclude each other");
    if (decay_.active) return fail(WV_E_STATE, "wv_set_lateral: a decay plan is active (wv_set_decay(e, NULL) stops it); the plans exclude each other");
    if (inten_.active) return fail(WV_E_STATE, "wv_set_lateral: an intensity plan is active (wv_set_intensity(e, NULL) stops it); the plans exclude each other");
    if (arr_.active) return fail(WV_E_STATE, "wv_set_lateral: an arrival plan is active (wv_set_arrival(e, NULL, NULL) stops it); the plans exclude each other");
    const char* why = nullptr;
    if (wv::lateral_plan_check(*plan, nx_, ny_, nz_, &why)) return fail(WV_E_INVALID_ARGUMENT, why);
    const wv::SnapshotBox box = wv::lateral_box(*plan);
    const uint64_t nodes = wv::decay_nodes(box.nx, box.ny, box.nz);
    if (threshold_map)
        for (uint64_t i = 0; i < nodes; ++i)
            if (!wv::arrival_threshold_valid(threshold_map[i]))
                return fail(WV_E_INVALID_ARGUMENT, "wv_set_lateral: every entry of the threshold map must be >= 0 and finite");
    // everything is allocated here, aside, and only a complete set takes the old plan's place: no room -> WV_E_HIP, engine untouched
    Lateral d;
    d.generation = lat_.generation + 1;
    d.plan = *plan;
    d.box = box;
    d.nodes = nodes;
    d.k = plan->ambient_density * plan->sample_rate;
    const uint64_t stage_bytes = wv::lateral_stage_bytes(nodes);
    const uint64_t state_bytes = wv::lateral_state_bytes(nodes, plan->n_bins);
    const uint64_t map_bytes = wv::lateral_map_bytes(nodes);
    const uint64_t most = std::numeric_limits<size_t>::max() / 2;
    hipError_t rc = hipSuccess;
    if (stage_bytes == wv::kDecayNoSize || state_bytes == wv::kDecayNoSize || stage_bytes > most || state_bytes > most) rc = hipErrorOutOfMemory;
    if (rc == hipSuccess && (rc = hipMalloc((void**)&d.stage, (size_t)stage_bytes)) != hipSuccess) d.stage = nullptr;
    if (rc == hipSuccess && (rc = hipMalloc((void**)&d.state, (size_t)state_bytes)) != hipSuccess) d.state = nullptr;
    if (threshold_map && rc == hipSuccess && (rc = hipMalloc((void**)&d.threshold_map, (size_t)map_bytes)) != hipSuccess) d.threshold_map = nullptr;
    for (int i = 0; i < 2 && rc == hipSuccess; ++i) {
        if ((rc = hipEventCreate(&d.begun[i])) != hipSuccess) break;
        if ((rc = hipEventCreate(&d.folded_ev[i])) != hipSuccess) break;
    }
    for (int i = 0; i < kLateralStage && rc == hipSuccess; ++i) {
        if ((rc = hipEventCreate(&d.gather_begun[i])) != hipSuccess) break;
        if ((rc = hipEventCreate(&d.gather_done[i])) != hipSuccess) break;
    }
    d.state_bytes = (size_t)state_bytes;
    // +0.0 everywhere, then NONE (all bits set) into the onsets
    if (rc == hipSuccess) rc = hipMemsetAsync(d.state, 0, (size_t)state_bytes, stream_);
    if (rc == hipSuccess) rc = hipMemsetAsync(d.state + wv::lateral_onset_offset(nodes, plan->n_bins), 0xFF, (size_t)nodes * 4, stream_);
    // (pageable memory: the copy has left the caller's array when the call returns)
    if (threshold_map && rc == hipSuccess) rc = hipMemcpyAsync(d.threshold_map, threshold_map, (size_t)map_bytes, hipMemcpyHostToDevice, stream_);
    if (rc == hipSuccess) rc = hipStreamSynchronize(stream_);
    if (rc != hipSuccess) {
        (void)hipGetLastError();  // nothing sticky
        lateral_release(d);
        wv::note_hip_error(rc);
        return fail(WV_E_HIP, std::string("wv_set_lateral: no room for the stage and the state: ") + hipGetErrorString(rc));
    }
    lateral_release(lat_);
    lat_ = std::move(d);
    lat_.st.start(plan->first_step, plan->period, steps_done);
    lat_.active = true;
    return WV_OK;
}

// The capture of `step`, which the field `current` holds once everything enqueued on the compute stream so far has run: into the
// slot behind the ones staged.
template <typename Real>
int Engine<Real>::lateral_capture(uint64_t step) {
    Lateral& d = lat_;
    // (lateral_plan_batch gives a batch no more captures than the stage has free slots)
    if (d.st.full()) return fail(WV_E_STATE, "wv_run: the lateral stage is full");
    // (onsets are 32 bits wide, and all bits set means "none")
    if (d.st.folded + (uint64_t)d.st.slot() >= wv::kLateralMaxCaptures) return fail(WV_E_STATE, "wv_run: the lateral plan has counted 2^32 - 1 captures");
    const int slot = d.st.slot();
    if (timing) WV_HIP(hipEventRecord(d.gather_begun[slot], stream_));
    const int rc = launch_intensity_gather(d.box, d.plan.spacing, d.stage + (uint64_t)slot * wv::kIntensityPlanes * d.nodes);  // (engine_snapshot.hip.h)
    if (rc) return rc;
    if (timing) {
        WV_HIP(hipEventRecord(d.gather_done[slot], stream_));
        d.gather_timed[slot] = true;
    }
    d.st.staged(step);
    return WV_OK;
}

// The times of the folds that recorded event pair `pair` (-1: either) and of the captures, where they ran with kernel timing on,
// once they have run.
template <typename Real>
int Engine<Real>::lateral_drain_timing(int pair) {
    Lateral& d = lat_;
    for (int b = 0; b < 2; ++b) {
        if (!d.timed[b] || (pair >= 0 && b != pair)) continue;
        WV_HIP(hipEventSynchronize(d.folded_ev[b]));
        float ms = 0;
        WV_HIP(hipEventElapsedTime(&ms, d.begun[b], d.folded_ev[b]));
        d.kernel_ms += ms;
        d.timed[b] = false;
    }
    for (int i = 0; i < kLateralStage; ++i) {
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

// All committed captures -> the state, one launch.  Only between batches, where nothing uncommitted is staged -- but for what a
// failed run left, which goes first: the stage is filled from slot 0 again behind a fold.
template <typename Real>
int Engine<Real>::lateral_fold() {
    Lateral& d = lat_;
    d.st.drop_uncommitted();
    const int t = d.st.committed;
    if (t == 0) return WV_OK;
    const uint64_t blocks = (d.nodes + 255) / 256;
    if (blocks > 0x7fffffffull) return fail(WV_E_STATE, "wv_set_lateral: the box has more nodes than one launch covers");
    const int b = d.pair;
    // (the slots' event pairs are recorded again by the captures behind this fold; the fold before last recorded this pair)
    const int rc = lateral_drain_timing(b);
    if (rc) return rc;
    if (timing) WV_HIP(hipEventRecord(d.begun[b], stream_));
    const uint32_t n_bins = d.plan.n_bins;
    // the plan's entries first; what lies behind them is not looked at (arrival_bin stops at n_bins)
    wv::ArrivalEdges edges;
    for (uint32_t m = 0; m < wv::kArrivalMaxBins; ++m) edges.e[m] = m < wv::kLateralMaxBins ? d.plan.edges[m] : wv::kLateralNone;
    // staged capture j is capture number folded + j since the plan was set (lateral_capture keeps it inside 32 bits)
    hipLaunchKernelGGL(wv::lateral_fold_kernel, dim3((unsigned)blocks), dim3(256), 0, stream_, d.stage,
                       reinterpret_cast<double*>(d.state + wv::lateral_pre_offset()), reinterpret_cast<double*>(d.state + wv::lateral_velocity_offset(d.nodes)),
                       reinterpret_cast<double*>(d.state + wv::lateral_bins_offset(d.nodes)),
                       reinterpret_cast<uint32_t*>(d.state + wv::lateral_onset_offset(d.nodes, n_bins)), (const float*)d.threshold_map, d.plan.threshold,
                       edges, n_bins, (uint32_t)d.st.folded, d.nodes, d.k, (int32_t)t);
    WV_HIP(hipGetLastError());
    if (timing) {
        WV_HIP(hipEventRecord(d.folded_ev[b], stream_));
        d.timed[b] = true;
        d.pair = 1 - b;
    }
    ++d.folds;
    d.st.all_folded();
    return WV_OK;
}

// Before a batch is planned: the fold when the stage has no slot left, and where the batch ends at the latest.
template <typename Real>
int Engine<Real>::lateral_plan_batch() {
    Lateral& d = lat_;
    if (d.st.fold_due()) {
        const int rc = lateral_fold();
        if (rc) return rc;
    }
    d.st.plan_batch_end(opt_.tuning.graph != 0);
    return WV_OK;
}

// On entering wv_run: steps taken by wv_step / wv_swap capture nothing, so plan steps they passed are passed; a capture of the step
// the engine stands at is due now (and is of a completed step: committed at once).
template <typename Real>
int Engine<Real>::lateral_begin_run() {
    Lateral& d = lat_;
    if (d.st.begin_run(steps_done)) {
        int rc = d.st.fold_due() ? lateral_fold() : WV_OK;
        if (rc) return rc;
        if ((rc = lateral_capture(steps_done))) return rc;
        d.st.commit(steps_done);
    }
    return WV_OK;
}

// wv_checkpoint under a plan: the state block (everything staged folded in first), the count and the next plan step aside; the copy
// is allocated by the first checkpoint taken under the plan.  Called before the checkpoint touches anything: no room -> WV_E_HIP,
// engine untouched.
template <typename Real>
int Engine<Real>::lateral_checkpoint() {
    Lateral& d = lat_;
    if (!ckpt_.lat_state || ckpt_.lat_bytes != d.state_bytes) {
        if (ckpt_.lat_state) (void)hipFree(ckpt_.lat_state);
        ckpt_.lat_state = nullptr;
        ckpt_.lat_bytes = 0;
        const hipError_t rc = hipMalloc((void**)&ckpt_.lat_state, d.state_bytes);
        if (rc != hipSuccess) {
            ckpt_.lat_state = nullptr;
            (void)hipGetLastError();
            return fail(WV_E_HIP, std::string("wv_checkpoint: no room for a copy of the lateral plan's state: ") + hipGetErrorString(rc));
        }
        ckpt_.lat_bytes = d.state_bytes;
    }
    const int rc = lateral_fold();
    if (rc) return rc;
    WV_HIP(hipMemcpyAsync(ckpt_.lat_state, d.state, d.state_bytes, hipMemcpyDeviceToDevice, stream_));
    ckpt_.lat_captures = d.st.folded;
    ckpt_.lat_last_step = d.st.last_step;
    ckpt_.lat_next = d.st.next;
    return WV_OK;
}

// wv_rollback (the plan is the one the checkpoint saw): state and count back, what is staged forgotten; the re-run takes it again.
template <typename Real>
int Engine<Real>::lateral_rollback() {
    Lateral& d = lat_;
    WV_HIP(hipMemcpyAsync(d.state, ckpt_.lat_state, ckpt_.lat_bytes, hipMemcpyDeviceToDevice, stream_));
    d.st.rollback(ckpt_.lat_captures, ckpt_.lat_last_step, ckpt_.lat_next);
    return WV_OK;
}

template <typename Real>
int Engine<Real>::lateral_count(uint64_t* captures, uint64_t* last_step) {
    if (!lat_.active) return fail(WV_E_STATE, "wv_lateral_count: no lateral plan is set");
    if (captures) *captures = lat_.st.captures();
    if (last_step) *last_step = lat_.st.last_step;
    return WV_OK;
}

// Folds what is staged, then every part the caller gave a destination for -> the host as it lies.  The plan keeps running.
template <typename Real>
int Engine<Real>::fetch_lateral(uint32_t* onset, double* pre, double* velocity, double* bins, uint64_t* captures) {
    DeviceGuard guard(device_);
    Lateral& d = lat_;
    if (!d.active) return fail(WV_E_STATE, "wv_fetch_lateral: no lateral plan is set");
    int rc = lateral_fold();
    if (rc) return rc;
    WV_HIP(hipStreamSynchronize(stream_));
    if ((rc = lateral_drain_timing())) return rc;
    const uint64_t B = d.nodes;
    const uint32_t n_bins = d.plan.n_bins;
    if (onset) WV_HIP(hipMemcpy(onset, d.state + wv::lateral_onset_offset(B, n_bins), (size_t)B * 4, hipMemcpyDeviceToHost));
    if (pre) WV_HIP(hipMemcpy(pre, d.state + wv::lateral_pre_offset(), (size_t)B * 8, hipMemcpyDeviceToHost));
    if (velocity) WV_HIP(hipMemcpy(velocity, d.state + wv::lateral_velocity_offset(B), (size_t)wv::lateral_velocity_bytes(B), hipMemcpyDeviceToHost));
    if (bins) WV_HIP(hipMemcpy(bins, d.state + wv::lateral_bins_offset(B), (size_t)wv::lateral_bins_bytes(B, n_bins), hipMemcpyDeviceToHost));
    if (captures) *captures = d.st.folded;
    return WV_OK;
}

}  // namespace wv

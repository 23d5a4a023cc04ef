// engine_arrival.hip.h -- wv_set_arrival / wv_arrival_count / wv_fetch_arrival: a box of the field, decimated, captured every `period`
// steps while wv_run keeps going -- as a decay plan captures it -- and per node, ON THE DEVICE, the capture at which the direct sound
// arrived, the peak, the squares summed into bins counted from the node's OWN arrival, the energy ahead of it and the first time
// moment of the energy behind it.  What crosses the link is 28 + 8 n_bins bytes per node when the caller asks for them, however long
// the run (wayverb_amd/arrival.py turns them into arrival time, clarity, definition and centre time).
//
// Part of the engine behind the C ABI of include/wayverb_amd.h (engine.hip is the translation unit; see engine.hip.h for the class).
//
// The life cycle is engine_decay.hip.h's, on the same stage bookkeeping (capture_stage.h); everything runs on the compute stream:
//   capture   snapshot_gather_kernel (snapshot_kernels.hip.h, unchanged) -> the next free slot of the device-only stage float[T][B],
//             directly behind the pass that produced the step (engine_batch.hip.h cuts batches and segments at whichever plan is
//             active: they exclude each other)
//   commit    a batch's captures stay staged until commit_batch has said how many of its steps were good (CaptureStage::commit)
//   fold      arrival_fold_kernel (arrival_kernels.hip.h) folds all staged captures, in order, into the per-node state in ONE launch,
//             and only when the stage has no slot left for the next batch -- or on fetch and checkpoint.  Which bin a capture goes to
//             differs from node to node, so there is no table for the host to write: the edge table and the number of the first
//             staged capture are kernel arguments.
// The state is only ever touched by a fold, and a fold only ever sees committed captures: after a stop on a flag no onset, peak or
// sum is of a step that was never completed.
#pragma once
#include "engine.hip.h"

namespace wv {

static_assert(kArrivalStage == kSpectrumStage, "the arrival plan stages its captures by spectrum_plan.h's rules");
static_assert(sizeof(((wv_arrival_plan*)nullptr)->edges) == sizeof(ArrivalEdges), "the edge table goes to the kernel as it lies in the plan");

template <typename Real>
void Engine<Real>::arrival_release(Arrival& d) {
    if (d.stage) (void)hipFree(d.stage);
    if (d.state) (void)hipFree(d.state);
    if (d.threshold_map) (void)hipFree(d.threshold_map);
    for (int i = 0; i < 2; ++i) {
        if (d.begun[i]) (void)hipEventDestroy(d.begun[i]);
        if (d.folded_ev[i]) (void)hipEventDestroy(d.folded_ev[i]);
    }
    const uint64_t generation = d.generation;
    d = Arrival{};
    d.generation = generation;
}

template <typename Real>
int Engine<Real>::set_arrival(const wv_arrival_plan* plan, const float* threshold_map) {
    DeviceGuard guard(device_);
    if (!plan) {
        WV_HIP(hipStreamSynchronize(stream_));
        arrival_release(arr_);
        ++arr_.generation;
        return WV_OK;
    }
    // (the snapshot plan's reason: a slab would have to cut its batches where its neighbours do, and holds only its part of a box)
    if (opt_.ghost_lo || opt_.ghost_hi || (comm_ && comm_->nranks() > 1))
        return fail(WV_E_STATE, "wv_set_arrival: not on a slab of a chain (one domain only)");
    // every plan wants to decide where passes end: one consumer of capture steps at a time
    if (snap_.active) return fail(WV_E_STATE, "wv_set_arrival: a snapshot plan is active (wv_set_snapshots(e, NULL) stops it); the plans exclude each other");
    if (spec_.active) return fail(WV_E_STATE, "wv_set_arrival: a spectrum plan is active (wv_set_spectrum(e, NULL, NULL) stops it); the plans exclude each other");
    if (decay_.active && decay_.n_bands)
        return fail(WV_E_STATE, "wv_set_arrival: a banded decay plan is active (wv_set_decay_bands(e, NULL, NULL, 0, 0) stops it); the plans exclude each other");
    if (decay_.active) return fail(WV_E_STATE, "wv_set_arrival: a decay plan is active (wv_set_decay(e, NULL) stops it); the plans exclude each other");
    if (inten_.active) return fail(WV_E_STATE, "wv_set_arrival: an intensity plan is active (wv_set_intensity(e, NULL) stops it); the plans exclude each other");
    if (lat_.active) return fail(WV_E_STATE, "wv_set_arrival: a lateral plan is active (wv_set_lateral(e, NULL, NULL) stops it); the plans exclude each other");
    if (plan->n_bins < 1 || plan->n_bins > wv::kArrivalMaxBins) return fail(WV_E_INVALID_ARGUMENT, "wv_set_arrival: n_bins must be 1 .. 16");
    if (!wv::arrival_edges_valid(plan->edges, plan->n_bins))
        return fail(WV_E_INVALID_ARGUMENT, "wv_set_arrival: edges[0] must be 0 and the edges strictly increasing");
    if (!wv::arrival_threshold_valid(plan->threshold)) return fail(WV_E_INVALID_ARGUMENT, "wv_set_arrival: the threshold must be >= 0 and finite");
    wv::SnapshotBox box;
    box.x0 = plan->x0, box.y0 = plan->y0, box.z0 = plan->z0;
    box.nx = plan->nx, box.ny = plan->ny, box.nz = plan->nz;
    box.sx = plan->sx, box.sy = plan->sy, box.sz = plan->sz;
    if (plan->sx < 1 || plan->sy < 1 || plan->sz < 1) return fail(WV_E_INVALID_ARGUMENT, "wv_set_arrival: strides must be >= 1");
    if (plan->period < 1) return fail(WV_E_INVALID_ARGUMENT, "wv_set_arrival: period must be >= 1");
    if (!wv::snapshot_box_valid(box, nx_, ny_, nz_)) return fail(WV_E_INVALID_ARGUMENT, "wv_set_arrival: the box leaves the mesh");
    // (the capture kernel indexes a dense plane with 32 bits)
    if ((uint64_t)box.nx * (uint64_t)box.ny >= (1ull << 31)) return fail(WV_E_INVALID_ARGUMENT, "wv_set_arrival: more than 2^31 nodes per plane of the box");
    const uint64_t nodes = wv::decay_nodes(box.nx, box.ny, box.nz);
    if (threshold_map)
        for (uint64_t i = 0; i < nodes; ++i)
            if (!wv::arrival_threshold_valid(threshold_map[i]))
                return fail(WV_E_INVALID_ARGUMENT, "wv_set_arrival: every entry of the threshold map must be >= 0 and finite");
    // everything is allocated here, aside, and only a complete set takes the old plan's place: no room -> WV_E_HIP, engine untouched
    Arrival d;
    d.generation = arr_.generation + 1;
    d.plan = *plan;
    d.box = box;
    d.nodes = nodes;
    d.gather_wide = box.sx == 1 && box.x0 % 4 == 0 && box.nx % 4 == 0;  // (as engine_snapshot.hip.h decides it)
    const uint64_t stage_bytes = wv::arrival_stage_bytes(nodes);
    const uint64_t state_bytes = wv::arrival_state_bytes(nodes, plan->n_bins);
    const uint64_t map_bytes = wv::arrival_map_bytes(nodes);
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
    d.state_bytes = (size_t)state_bytes;
    // +0.0 / +0.0f everywhere, then NONE (all bits set) into the onsets and the peak captures
    if (rc == hipSuccess) rc = hipMemsetAsync(d.state, 0, (size_t)state_bytes, stream_);
    if (rc == hipSuccess) rc = hipMemsetAsync(d.state + wv::arrival_onset_offset(nodes, plan->n_bins), 0xFF, (size_t)nodes * 4, stream_);
    if (rc == hipSuccess) rc = hipMemsetAsync(d.state + wv::arrival_peak_capture_offset(nodes, plan->n_bins), 0xFF, (size_t)nodes * 4, stream_);
    // (pageable memory: the copy has left the caller's array when the call returns)
    if (threshold_map && rc == hipSuccess) rc = hipMemcpyAsync(d.threshold_map, threshold_map, (size_t)map_bytes, hipMemcpyHostToDevice, stream_);
    if (rc == hipSuccess) rc = hipStreamSynchronize(stream_);
    if (rc != hipSuccess) {
        (void)hipGetLastError();  // nothing sticky
        arrival_release(d);
        wv::note_hip_error(rc);
        return fail(WV_E_HIP, std::string("wv_set_arrival: no room for the stage and the state: ") + hipGetErrorString(rc));
    }
    arrival_release(arr_);
    arr_ = std::move(d);
    arr_.st.start(plan->first_step, plan->period, steps_done);
    arr_.active = true;
    return WV_OK;
}

// The capture of `step`, which the field `current` holds once everything enqueued on the compute stream so far has run: into the
// slot behind the ones staged.
template <typename Real>
int Engine<Real>::arrival_capture(uint64_t step) {
    Arrival& d = arr_;
    // (arrival_plan_batch gives a batch no more captures than the stage has free slots)
    if (d.st.full()) return fail(WV_E_STATE, "wv_run: the arrival stage is full");
    // (onsets and peak captures are 32 bits wide, and all bits set means "none")
    if (d.st.folded + (uint64_t)d.st.slot() >= wv::kArrivalMaxCaptures) return fail(WV_E_STATE, "wv_run: the arrival plan has counted 2^32 - 1 captures");
    const int rc = launch_snapshot_gather(d.box, d.gather_wide, d.stage + (uint64_t)d.st.slot() * d.nodes);  // (engine_snapshot.hip.h)
    if (rc) return rc;
    d.st.staged(step);
    return WV_OK;
}

// The times of the folds that recorded event pair `pair` (-1: either), once they have run (kernel timing on).
template <typename Real>
int Engine<Real>::arrival_drain_timing(int pair) {
    Arrival& d = arr_;
    for (int b = 0; b < 2; ++b) {
        if (!d.timed[b] || (pair >= 0 && b != pair)) continue;
        WV_HIP(hipEventSynchronize(d.folded_ev[b]));
        float ms = 0;
        WV_HIP(hipEventElapsedTime(&ms, d.begun[b], d.folded_ev[b]));
        d.kernel_ms += ms;
        d.timed[b] = false;
    }
    return WV_OK;
}

// All committed captures -> the state, one launch.  Only between batches, where nothing uncommitted is staged -- but for what a
// failed run left, which goes first: the stage is filled from slot 0 again behind a fold.
template <typename Real>
int Engine<Real>::arrival_fold() {
    Arrival& d = arr_;
    d.st.drop_uncommitted();
    const int t = d.st.committed;
    if (t == 0) return WV_OK;
    const uint64_t blocks = (d.nodes + 255) / 256;
    if (blocks > 0x7fffffffull) return fail(WV_E_STATE, "wv_set_arrival: the box has more nodes than one launch covers");
    const int b = d.pair;
    if (timing) {
        const int rc = arrival_drain_timing(b);  // (the fold before last recorded this pair)
        if (rc) return rc;
        WV_HIP(hipEventRecord(d.begun[b], stream_));
    }
    const uint32_t n_bins = d.plan.n_bins;
    wv::ArrivalEdges edges;
    for (uint32_t k = 0; k < wv::kArrivalMaxBins; ++k) edges.e[k] = d.plan.edges[k];
    // staged capture j is capture number folded + j since the plan was set (arrival_capture keeps it inside 32 bits)
    hipLaunchKernelGGL(wv::arrival_fold_kernel, dim3((unsigned)blocks), dim3(256), 0, stream_, d.stage,
                       reinterpret_cast<double*>(d.state + wv::arrival_pre_offset()), reinterpret_cast<double*>(d.state + wv::arrival_moment_offset(d.nodes)),
                       reinterpret_cast<double*>(d.state + wv::arrival_bins_offset(d.nodes)),
                       reinterpret_cast<uint32_t*>(d.state + wv::arrival_onset_offset(d.nodes, n_bins)),
                       reinterpret_cast<float*>(d.state + wv::arrival_peak_offset(d.nodes, n_bins)),
                       reinterpret_cast<uint32_t*>(d.state + wv::arrival_peak_capture_offset(d.nodes, n_bins)),
                       (const float*)d.threshold_map, d.plan.threshold, edges, n_bins, (uint32_t)d.st.folded, d.nodes, (int32_t)t);
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
int Engine<Real>::arrival_plan_batch() {
    Arrival& d = arr_;
    if (d.st.fold_due()) {
        const int rc = arrival_fold();
        if (rc) return rc;
    }
    d.st.plan_batch_end(opt_.tuning.graph != 0);
    return WV_OK;
}

// On entering wv_run: steps taken by wv_step / wv_swap capture nothing, so plan steps they passed are passed; a capture of the step
// the engine stands at is due now (and is of a completed step: committed at once).
template <typename Real>
int Engine<Real>::arrival_begin_run() {
    Arrival& d = arr_;
    if (d.st.begin_run(steps_done)) {
        int rc = d.st.fold_due() ? arrival_fold() : WV_OK;
        if (rc) return rc;
        if ((rc = arrival_capture(steps_done))) return rc;
        d.st.commit(steps_done);
    }
    return WV_OK;
}

// wv_checkpoint under a plan: the state block (everything staged folded in first), the count and the next plan step aside; the copy
// is allocated by the first checkpoint taken under the plan.  Called before the checkpoint touches anything: no room -> WV_E_HIP,
// engine untouched.
template <typename Real>
int Engine<Real>::arrival_checkpoint() {
    Arrival& d = arr_;
    if (!ckpt_.arr_state || ckpt_.arr_bytes != d.state_bytes) {
        if (ckpt_.arr_state) (void)hipFree(ckpt_.arr_state);
        ckpt_.arr_state = nullptr;
        ckpt_.arr_bytes = 0;
        const hipError_t rc = hipMalloc((void**)&ckpt_.arr_state, d.state_bytes);
        if (rc != hipSuccess) {
            ckpt_.arr_state = nullptr;
            (void)hipGetLastError();
            return fail(WV_E_HIP, std::string("wv_checkpoint: no room for a copy of the arrival plan's state: ") + hipGetErrorString(rc));
        }
        ckpt_.arr_bytes = d.state_bytes;
    }
    const int rc = arrival_fold();
    if (rc) return rc;
    WV_HIP(hipMemcpyAsync(ckpt_.arr_state, d.state, d.state_bytes, hipMemcpyDeviceToDevice, stream_));
    ckpt_.arr_captures = d.st.folded;
    ckpt_.arr_last_step = d.st.last_step;
    ckpt_.arr_next = d.st.next;
    return WV_OK;
}

// wv_rollback (the plan is the one the checkpoint saw): state and count back, what is staged forgotten; the re-run takes it again.
template <typename Real>
int Engine<Real>::arrival_rollback() {
    Arrival& d = arr_;
    WV_HIP(hipMemcpyAsync(d.state, ckpt_.arr_state, ckpt_.arr_bytes, hipMemcpyDeviceToDevice, stream_));
    d.st.rollback(ckpt_.arr_captures, ckpt_.arr_last_step, ckpt_.arr_next);
    return WV_OK;
}

template <typename Real>
int Engine<Real>::arrival_count(uint64_t* captures, uint64_t* last_step) {
    if (!arr_.active) return fail(WV_E_STATE, "wv_arrival_count: no arrival plan is set");
    if (captures) *captures = arr_.st.captures();
    if (last_step) *last_step = arr_.st.last_step;
    return WV_OK;
}

// Folds what is staged, then every part the caller gave a destination for -> the host as it lies.  The plan keeps running.
template <typename Real>
int Engine<Real>::fetch_arrival(uint32_t* onset, float* peak, uint32_t* peak_capture, double* pre, double* moment, double* bins, uint64_t* captures) {
    DeviceGuard guard(device_);
    Arrival& d = arr_;
    if (!d.active) return fail(WV_E_STATE, "wv_fetch_arrival: no arrival plan is set");
    int rc = arrival_fold();
    if (rc) return rc;
    WV_HIP(hipStreamSynchronize(stream_));
    if ((rc = arrival_drain_timing())) return rc;
    const uint64_t B = d.nodes;
    const uint32_t n_bins = d.plan.n_bins;
    if (onset) WV_HIP(hipMemcpy(onset, d.state + wv::arrival_onset_offset(B, n_bins), (size_t)B * 4, hipMemcpyDeviceToHost));
    if (peak) WV_HIP(hipMemcpy(peak, d.state + wv::arrival_peak_offset(B, n_bins), (size_t)B * 4, hipMemcpyDeviceToHost));
    if (peak_capture) WV_HIP(hipMemcpy(peak_capture, d.state + wv::arrival_peak_capture_offset(B, n_bins), (size_t)B * 4, hipMemcpyDeviceToHost));
    if (pre) WV_HIP(hipMemcpy(pre, d.state + wv::arrival_pre_offset(), (size_t)B * 8, hipMemcpyDeviceToHost));
    if (moment) WV_HIP(hipMemcpy(moment, d.state + wv::arrival_moment_offset(B), (size_t)B * 8, hipMemcpyDeviceToHost));
    if (bins) WV_HIP(hipMemcpy(bins, d.state + wv::arrival_bins_offset(B), (size_t)wv::arrival_bins_bytes(B, n_bins), hipMemcpyDeviceToHost));
    if (captures) *captures = d.st.folded;
    return WV_OK;
}

}  // namespace wv

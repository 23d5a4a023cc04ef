// engine_decay.hip.h -- wv_set_decay / wv_decay_count / wv_fetch_decay: a box of the field, decimated, captured every `period` steps
// while wv_run keeps going -- as a snapshot plan captures it -- and its squares summed per node into time bins ON THE DEVICE.  What
// crosses the link is n_bins doubles per node when the caller asks for them, however long the run; the backward sums of the bins are
// the Schroeder integral at the bin edges (wayverb_amd/decay.py).
//
// Part of the engine behind the C ABI of include/wayverb_amd.h (engine.hip is the translation unit; see engine.hip.h for the class).
//
// The life cycle is engine_spectrum.hip.h's, on the same stage bookkeeping (capture_stage.h); everything runs on the compute stream:
//   capture   snapshot_gather_kernel (snapshot_kernels.hip.h, unchanged) -> the next free slot of the device-only stage float[T][B],
//             directly behind the pass that produced the step (engine_batch.hip.h cuts batches and segments at whichever of the
//             three plans is active: they exclude each other)
//   commit    a batch's captures stay staged until commit_batch has said how many of its steps were good (CaptureStage::commit)
//   fold      decay_fold_kernel (decay_kernels.hip.h) folds all staged captures into the bins double[n_bins][B] in ONE launch, and
//             only when the stage has no slot left for the next batch -- or on fetch and checkpoint.  The bins of the t staged
//             captures, int32[t], are written by the host (decay_plan.h: decay_bin of the capture's number since the plan was set)
//             into one of two page-locked tables and copied ahead of the launch; two, so that the host never rewrites a table a
//             queued copy still reads.
//
// wv_set_decay_bands / wv_fetch_decay_bands are the same plan with a filter bank ahead of the square: n_bands cascades of n_sections
// biquad sections per node, their state double[n_bands][n_sections][2][B] and the coefficient table beside the bins, which grow to
// double[n_bands][n_bins][B]; decay_bands_fold_kernel (decay_bands_kernels.hip.h) takes decay_fold_kernel's place, one grid row per
// band.  Capture, commit, the fold's timing, the cut of batches, the exclusions and the queries are the plain plan's code, unchanged:
// the state is only ever touched by a fold, and a fold only ever sees committed captures.
#pragma once
#include "engine.hip.h"

namespace wv {

static_assert(kDecayStage == kSpectrumStage, "the decay plan stages its captures by spectrum_plan.h's rules");

template <typename Real>
void Engine<Real>::decay_release(Decay& d) {
    if (d.stage) (void)hipFree(d.stage);
    if (d.bins) (void)hipFree(d.bins);
    if (d.state) (void)hipFree(d.state);
    if (d.coef) (void)hipFree(d.coef);
    for (int i = 0; i < 2; ++i) {
        if (d.table_dev[i]) (void)hipFree(d.table_dev[i]);
        if (d.table_host[i]) (void)hipHostFree(d.table_host[i]);
        if (d.begun[i]) (void)hipEventDestroy(d.begun[i]);
        if (d.folded_ev[i]) (void)hipEventDestroy(d.folded_ev[i]);
    }
    const uint64_t generation = d.generation;
    d = Decay{};
    d.generation = generation;
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
    if (!plan) {
        WV_HIP(hipStreamSynchronize(stream_));
        decay_release(decay_);
        ++decay_.generation;
        return WV_OK;
    }
    // (the snapshot plan's reason: a slab would have to cut its batches where its neighbours do, and holds only its part of a box)
    if (opt_.ghost_lo || opt_.ghost_hi || (comm_ && comm_->nranks() > 1))
        return fail(WV_E_STATE, who + ": not on a slab of a chain (one domain only)");
    // all three plans want to decide where passes end: one consumer of capture steps at a time
    if (snap_.active) return fail(WV_E_STATE, who + ": a snapshot plan is active (wv_set_snapshots(e, NULL) stops it); the plans exclude each other");
    if (spec_.active) return fail(WV_E_STATE, who + ": a spectrum plan is active (wv_set_spectrum(e, NULL, NULL) stops it); the plans exclude each other");
    if (inten_.active) return fail(WV_E_STATE, who + ": an intensity plan is active (wv_set_intensity(e, NULL) stops it); the plans exclude each other");
    if (arr_.active) return fail(WV_E_STATE, who + ": an arrival plan is active (wv_set_arrival(e, NULL, NULL) stops it); the plans exclude each other");
    if (lat_.active) return fail(WV_E_STATE, who + ": a lateral plan is active (wv_set_lateral(e, NULL, NULL) stops it); the plans exclude each other");
    // the two kinds of decay plan answer to different fetches: neither setter turns one into the other behind the caller's back
    if (decay_.active && banded && !decay_.n_bands)
        return fail(WV_E_STATE, "wv_set_decay_bands: a plain decay plan is active (wv_set_decay(e, NULL) stops it); the plans exclude each other");
    if (decay_.active && !banded && decay_.n_bands)
        return fail(WV_E_STATE, "wv_set_decay: a banded decay plan is active (wv_set_decay_bands(e, NULL, NULL, 0, 0) stops it); the plans exclude each other");
    if (banded) {
        if (!wv::decay_bands_valid(n_bands, n_sections)) return fail(WV_E_INVALID_ARGUMENT, "wv_set_decay_bands: n_bands must be 1 .. 8 and n_sections 1 .. 4");
        if (!sections) return fail(WV_E_INVALID_ARGUMENT, "null argument");
        for (uint32_t i = 0; i < n_bands * n_sections; ++i) {
            const wv_biquad& c = sections[i];
            if (!std::isfinite(c.b0) || !std::isfinite(c.b1) || !std::isfinite(c.b2) || !std::isfinite(c.a1) || !std::isfinite(c.a2))
                return fail(WV_E_INVALID_ARGUMENT, "wv_set_decay_bands: every coefficient must be finite");
        }
    }
    if (plan->n_bins < 1 || plan->n_bins > wv::kDecayMaxBins) return fail(WV_E_INVALID_ARGUMENT, who + ": n_bins must be 1 .. 4096");
    if (plan->bin_captures < 1) return fail(WV_E_INVALID_ARGUMENT, who + ": bin_captures must be >= 1");
    wv::SnapshotBox box;
    box.x0 = plan->x0, box.y0 = plan->y0, box.z0 = plan->z0;
    box.nx = plan->nx, box.ny = plan->ny, box.nz = plan->nz;
    box.sx = plan->sx, box.sy = plan->sy, box.sz = plan->sz;
    if (plan->sx < 1 || plan->sy < 1 || plan->sz < 1) return fail(WV_E_INVALID_ARGUMENT, who + ": strides must be >= 1");
    if (plan->period < 1) return fail(WV_E_INVALID_ARGUMENT, who + ": period must be >= 1");
    if (!wv::snapshot_box_valid(box, nx_, ny_, nz_)) return fail(WV_E_INVALID_ARGUMENT, who + ": the box leaves the mesh");
    // (the capture kernel indexes a dense plane with 32 bits)
    if ((uint64_t)box.nx * (uint64_t)box.ny >= (1ull << 31)) return fail(WV_E_INVALID_ARGUMENT, who + ": more than 2^31 nodes per plane of the box");
    // everything is allocated here, aside, and only a complete set takes the old plan's place: no room -> WV_E_HIP, engine untouched
    Decay d;
    d.generation = decay_.generation + 1;
    d.plan = *plan;
    d.box = box;
    d.nodes = wv::decay_nodes(box.nx, box.ny, box.nz);
    d.gather_wide = box.sx == 1 && box.x0 % 4 == 0 && box.nx % 4 == 0;  // (as engine_snapshot.hip.h decides it)
    d.fold_wide = !banded && d.nodes % 2 == 0;                           // two nodes per lane, 16-byte accesses on the bins
    d.n_bands = banded ? n_bands : 0;
    d.n_sections = banded ? n_sections : 0;
    const uint64_t stage_bytes = wv::decay_stage_bytes(d.nodes);
    const uint64_t bins_bytes = banded ? wv::decay_band_bins_bytes(d.nodes, plan->n_bins, n_bands) : wv::decay_bins_bytes(d.nodes, plan->n_bins);
    const uint64_t state_bytes = banded ? wv::decay_band_state_bytes(d.nodes, n_bands, n_sections) : 0;
    const size_t coef_bytes = banded ? (size_t)wv::decay_band_coef_bytes(n_bands, n_sections) : 0;
    static_assert(sizeof(wv_biquad) == wv::kBiquadDoubles * sizeof(double), "wv_biquad is five doubles: the coefficient table is the caller's array as it lies");
    const size_t table_bytes = (size_t)wv::decay_table_bytes();
    hipError_t rc = hipSuccess;
    if (stage_bytes == wv::kDecayNoSize || bins_bytes == wv::kDecayNoSize || stage_bytes > std::numeric_limits<size_t>::max() / 2 ||
        bins_bytes > std::numeric_limits<size_t>::max() / 2 || state_bytes == wv::kDecayNoSize || state_bytes > std::numeric_limits<size_t>::max() / 2)
        rc = hipErrorOutOfMemory;
    if (rc == hipSuccess && (rc = hipMalloc((void**)&d.stage, (size_t)stage_bytes)) != hipSuccess) d.stage = nullptr;
    if (rc == hipSuccess && (rc = hipMalloc((void**)&d.bins, (size_t)bins_bytes)) != hipSuccess) d.bins = nullptr;
    if (banded && rc == hipSuccess && (rc = hipMalloc((void**)&d.state, (size_t)state_bytes)) != hipSuccess) d.state = nullptr;
    if (banded && rc == hipSuccess && (rc = hipMalloc((void**)&d.coef, coef_bytes)) != hipSuccess) d.coef = nullptr;
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
    if (rc == hipSuccess) rc = hipMemsetAsync(d.bins, 0, (size_t)bins_bytes, stream_);  // (+0.0 everywhere)
    if (banded && rc == hipSuccess) rc = hipMemsetAsync(d.state, 0, (size_t)state_bytes, stream_);
    // (pageable memory: the copy has left the caller's array when the call returns)
    if (banded && rc == hipSuccess) rc = hipMemcpyAsync(d.coef, sections, coef_bytes, hipMemcpyHostToDevice, stream_);
    if (rc == hipSuccess) rc = hipStreamSynchronize(stream_);
    if (rc != hipSuccess) {
        (void)hipGetLastError();  // nothing sticky
        decay_release(d);
        wv::note_hip_error(rc);
        return fail(WV_E_HIP, std::string(who + ": no room for the stage and the bins: ") + hipGetErrorString(rc));
    }
    decay_release(decay_);
    decay_ = std::move(d);
    decay_.st.start(plan->first_step, plan->period, steps_done);
    decay_.active = true;
    return WV_OK;
}

// The capture of `step`, which the field `current` holds once everything enqueued on the compute stream so far has run: into the
// slot behind the ones staged.
template <typename Real>
int Engine<Real>::decay_capture(uint64_t step) {
    Decay& d = decay_;
    // (decay_plan_batch gives a batch no more captures than the stage has free slots)
    if (d.st.full()) return fail(WV_E_STATE, "wv_run: the decay stage is full");
    const int rc = launch_snapshot_gather(d.box, d.gather_wide, d.stage + (uint64_t)d.st.slot() * d.nodes);  // (engine_snapshot.hip.h)
    if (rc) return rc;
    d.st.staged(step);
    return WV_OK;
}

// The time of the fold that last used table `b`, once it has run (kernel timing on).
template <typename Real>
int Engine<Real>::decay_drain_timing(int b) {
    Decay& d = decay_;
    if (!d.timed[b]) return WV_OK;
    WV_HIP(hipEventSynchronize(d.folded_ev[b]));
    float ms = 0;
    WV_HIP(hipEventElapsedTime(&ms, d.begun[b], d.folded_ev[b]));
    d.kernel_ms += ms;
    d.timed[b] = false;
    return WV_OK;
}

// All committed captures -> the bins, one launch.  Only between batches, where nothing uncommitted is staged -- but for what a
// failed run left, which goes first: the stage is filled from slot 0 again behind a fold.
template <typename Real>
int Engine<Real>::decay_fold() {
    Decay& d = decay_;
    d.st.drop_uncommitted();
    const int t = d.st.committed;
    if (t == 0) return WV_OK;
    const int b = d.table;
    // the fold before last used this table: its copy has long left the host's (a wait only if the device is two folds behind)
    if (d.table_used[b]) WV_HIP(hipEventSynchronize(d.folded_ev[b]));
    int rc = decay_drain_timing(b);
    if (rc) return rc;
    // staged capture j is capture number folded + j since the plan was set
    for (int j = 0; j < t; ++j) d.table_host[b][j] = (int32_t)wv::decay_bin(d.st.folded + (uint64_t)j, d.plan.bin_captures, d.plan.n_bins);
    WV_HIP(hipMemcpyAsync(d.table_dev[b], d.table_host[b], (size_t)t * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
    const uint64_t items = d.fold_wide ? d.nodes / 2 : d.nodes;  // (a banded plan: one node per lane)
    const uint64_t blocks = (items + 255) / 256;
    if (blocks > 0x7fffffffull) return fail(WV_E_STATE, "wv_set_decay: the box has more nodes than one launch covers");
    if (timing) {
        WV_HIP(hipEventRecord(d.begun[b], stream_));
        d.timed[b] = true;
    }
    if (d.n_bands) {
        const dim3 grid((unsigned)blocks, d.n_bands);  // (blockIdx.y = the band)
#define WV_BANDS_FOLD(S)                                                                                                                  \
    hipLaunchKernelGGL((wv::decay_bands_fold_kernel<S>), grid, dim3(256), 0, stream_, d.stage, d.state, d.bins, d.coef, d.table_dev[b], d.nodes, \
                       d.plan.n_bins, (int32_t)t)
        switch (d.n_sections) {
            case 1: WV_BANDS_FOLD(1); break;
            case 2: WV_BANDS_FOLD(2); break;
            case 3: WV_BANDS_FOLD(3); break;
            default: WV_BANDS_FOLD(4); break;
        }
#undef WV_BANDS_FOLD
    } else if (d.fold_wide)
        hipLaunchKernelGGL((wv::decay_fold_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, stream_, d.stage, d.bins, d.table_dev[b], d.nodes, (int32_t)t);
    else
        hipLaunchKernelGGL((wv::decay_fold_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, stream_, d.stage, d.bins, d.table_dev[b], d.nodes, (int32_t)t);
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
int Engine<Real>::decay_plan_batch() {
    Decay& d = decay_;
    if (d.st.fold_due()) {
        const int rc = decay_fold();
        if (rc) return rc;
    }
    d.st.plan_batch_end(opt_.tuning.graph != 0);
    return WV_OK;
}

// On entering wv_run: steps taken by wv_step / wv_swap capture nothing, so plan steps they passed are passed; a capture of the step
// the engine stands at is due now (and is of a completed step: committed at once).
template <typename Real>
int Engine<Real>::decay_begin_run() {
    Decay& d = decay_;
    if (d.st.begin_run(steps_done)) {
        int rc = d.st.fold_due() ? decay_fold() : WV_OK;
        if (rc) return rc;
        if ((rc = decay_capture(steps_done))) return rc;
        d.st.commit(steps_done);
    }
    return WV_OK;
}

// wv_checkpoint under a plan: the bins (everything staged folded in first), the count and the next plan step aside; the copy is
// allocated by the first checkpoint taken under the plan.  Called before the checkpoint touches anything: no room -> WV_E_HIP,
// engine untouched.
template <typename Real>
int Engine<Real>::decay_checkpoint() {
    Decay& d = decay_;
    const size_t bytes = (size_t)(d.n_bands ? wv::decay_band_bins_bytes(d.nodes, d.plan.n_bins, d.n_bands) : wv::decay_bins_bytes(d.nodes, d.plan.n_bins));
    const size_t state_bytes = (size_t)(d.n_bands ? wv::decay_band_state_bytes(d.nodes, d.n_bands, d.n_sections) : 0);
    if (state_bytes && (!ckpt_.decay_state || ckpt_.decay_state_bytes != state_bytes)) {  // a banded plan's filter states go aside with its bins
        if (ckpt_.decay_state) (void)hipFree(ckpt_.decay_state);
        ckpt_.decay_state = nullptr;
        ckpt_.decay_state_bytes = 0;
        const hipError_t rc = hipMalloc((void**)&ckpt_.decay_state, state_bytes);
        if (rc != hipSuccess) {
            ckpt_.decay_state = nullptr;
            (void)hipGetLastError();
            return fail(WV_E_HIP, std::string("wv_checkpoint: no room for a copy of the decay plan's filter states: ") + hipGetErrorString(rc));
        }
        ckpt_.decay_state_bytes = state_bytes;
    }
    if (!ckpt_.decay_bins || ckpt_.decay_bytes != bytes) {
        if (ckpt_.decay_bins) (void)hipFree(ckpt_.decay_bins);
        ckpt_.decay_bins = nullptr;
        ckpt_.decay_bytes = 0;
        const hipError_t rc = hipMalloc((void**)&ckpt_.decay_bins, bytes);
        if (rc != hipSuccess) {
            ckpt_.decay_bins = nullptr;
            (void)hipGetLastError();
            return fail(WV_E_HIP, std::string("wv_checkpoint: no room for a copy of the decay plan's bins: ") + hipGetErrorString(rc));
        }
        ckpt_.decay_bytes = bytes;
    }
    const int rc = decay_fold();
    if (rc) return rc;
    WV_HIP(hipMemcpyAsync(ckpt_.decay_bins, d.bins, bytes, hipMemcpyDeviceToDevice, stream_));
    if (state_bytes) WV_HIP(hipMemcpyAsync(ckpt_.decay_state, d.state, state_bytes, hipMemcpyDeviceToDevice, stream_));
    ckpt_.decay_captures = d.st.folded;
    ckpt_.decay_last_step = d.st.last_step;
    ckpt_.decay_next = d.st.next;
    return WV_OK;
}

// wv_rollback (the plan is the one the checkpoint saw): bins and count back, what is staged forgotten; the re-run takes it again.
template <typename Real>
int Engine<Real>::decay_rollback() {
    Decay& d = decay_;
    WV_HIP(hipMemcpyAsync(d.bins, ckpt_.decay_bins, ckpt_.decay_bytes, hipMemcpyDeviceToDevice, stream_));
    if (d.n_bands) WV_HIP(hipMemcpyAsync(d.state, ckpt_.decay_state, ckpt_.decay_state_bytes, hipMemcpyDeviceToDevice, stream_));
    d.st.rollback(ckpt_.decay_captures, ckpt_.decay_last_step, ckpt_.decay_next);
    return WV_OK;
}

template <typename Real>
int Engine<Real>::decay_count(uint64_t* captures, uint64_t* last_step) {
    if (!decay_.active) return fail(WV_E_STATE, "wv_decay_count: no decay plan is set");
    if (captures) *captures = decay_.st.captures();
    if (last_step) *last_step = decay_.st.last_step;
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
    int rc = decay_fold();
    if (rc) return rc;
    WV_HIP(hipStreamSynchronize(stream_));
    for (int b = 0; b < 2; ++b)
        if ((rc = decay_drain_timing(b))) return rc;
    const uint64_t bytes = d.n_bands ? wv::decay_band_bins_bytes(d.nodes, d.plan.n_bins, d.n_bands) : wv::decay_bins_bytes(d.nodes, d.plan.n_bins);
    WV_HIP(hipMemcpy(dst, d.bins, (size_t)bytes, hipMemcpyDeviceToHost));
    if (captures) *captures = d.st.folded;
    return WV_OK;
}

}  // namespace wv

// engine_spectrum.hip.h -- wv_set_spectrum / wv_spectrum_count / wv_fetch_spectrum: a box of the field, decimated, captured every
// `period` steps while wv_run keeps going -- as a snapshot plan captures it -- and Fourier-transformed ON THE DEVICE at K given
// frequencies.  What crosses the link is K complex numbers per node when the caller asks for them, however long the run.
//
// Part of the engine behind the C ABI of include/wayverb_amd.h (engine.hip is the translation unit; see engine.hip.h for the class).
//
// Everything runs on the compute stream, in order:
//   capture   snapshot_gather_kernel (snapshot_kernels.hip.h, unchanged) -> the next free slot of the device-only stage float[T][B],
//             directly behind the pass that produced the step.  A plan step is the end of a pass exactly as a snapshot step is:
//             engine_batch.hip.h cuts its batches and segments at whichever plan is active (the two plans exclude each other).
//   commit    a batch's captures stay staged until commit_batch has said how many of its steps were good; those of later steps are
//             dropped (CaptureStage::commit, capture_stage.h: the stage's bookkeeping, shared with engine_decay.hip.h).  A capture of a step that was never completed is never folded in.
//   fold      spectrum_fold_kernel (spectrum_kernels.hip.h) folds all staged captures into the sums double[K][2][B] in ONE launch,
//             and only when the stage has no slot left for the next batch -- or on fetch and checkpoint.  (A new plan, a NULL plan
//             and wv_destroy fold nothing: the sums are forgotten with the stage.)
//             Never because a batch ended: folding moves 32 K bytes per node whatever the number of captures.
//             Its twiddle table double[t][K][2] is written by the host (wv_spectrum_twiddle) into one of two page-locked buffers
//             and copied ahead of the launch; two, so that the host never rewrites a table a queued copy still reads.
// In-order execution is what keeps a slot from being overwritten before the fold has read it: captures of the next batch are
// enqueued behind the fold.
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
void Engine<Real>::spectrum_release(Spectrum& s) {
    if (s.stage) (void)hipFree(s.stage);
    if (s.acc) (void)hipFree(s.acc);
    for (int i = 0; i < 2; ++i) {
        if (s.tw_dev[i]) (void)hipFree(s.tw_dev[i]);
        if (s.tw_host[i]) (void)hipHostFree(s.tw_host[i]);
        if (s.begun[i]) (void)hipEventDestroy(s.begun[i]);
        if (s.folded_ev[i]) (void)hipEventDestroy(s.folded_ev[i]);
    }
    const uint64_t generation = s.generation;
    s = Spectrum{};
    s.generation = generation;
}

template <typename Real>
int Engine<Real>::set_spectrum(const wv_spectrum_plan* plan, const double* cycles_per_step) {
    DeviceGuard guard(device_);
    if (!plan) {
        WV_HIP(hipStreamSynchronize(stream_));
        spectrum_release(spec_);
        ++spec_.generation;
        return WV_OK;
    }
    // (the snapshot plan's reason: a slab would have to cut its batches where its neighbours do, and holds only its part of a box)
    if (opt_.ghost_lo || opt_.ghost_hi || (comm_ && comm_->nranks() > 1))
        return fail(WV_E_STATE, "wv_set_spectrum: not on a slab of a chain (one domain only)");
    // both plans want to decide where passes end: one consumer of capture steps at a time
    if (snap_.active) return fail(WV_E_STATE, "wv_set_spectrum: a snapshot plan is active (wv_set_snapshots(e, NULL) stops it); the two plans exclude each other");
    if (decay_.active) return fail(WV_E_STATE, "wv_set_spectrum: a decay plan is active (wv_set_decay(e, NULL) stops it); the plans exclude each other");
    if (inten_.active) return fail(WV_E_STATE, "wv_set_spectrum: an intensity plan is active (wv_set_intensity(e, NULL) stops it); the plans exclude each other");
    if (arr_.active) return fail(WV_E_STATE, "wv_set_spectrum: an arrival plan is active (wv_set_arrival(e, NULL, NULL) stops it); the plans exclude each other");
    if (lat_.active) return fail(WV_E_STATE, "wv_set_spectrum: a lateral plan is active (wv_set_lateral(e, NULL, NULL) stops it); the plans exclude each other");
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
    // everything is allocated here, aside, and only a complete set takes the old plan's place: no room -> WV_E_HIP, engine untouched
    Spectrum s;
    s.generation = spec_.generation + 1;
    s.plan = *plan;
    s.box = box;
    s.freqs.assign(cycles_per_step, cycles_per_step + plan->n_freqs);
    s.nodes = wv::spectrum_nodes(box.nx, box.ny, box.nz);
    s.gather_wide = box.sx == 1 && box.x0 % 4 == 0 && box.nx % 4 == 0;  // (as engine_snapshot.hip.h decides it)
    s.fold_wide = s.nodes % 2 == 0;                                      // two nodes per lane, 16-byte accesses on the sums
    const uint64_t stage_bytes = wv::spectrum_stage_bytes(s.nodes), sum_bytes = wv::spectrum_sum_bytes(s.nodes, plan->n_freqs);
    const size_t table_bytes = (size_t)wv::spectrum_table_bytes(plan->n_freqs);
    hipError_t rc = hipSuccess;
    if (stage_bytes == wv::kSpectrumNoSize || sum_bytes == wv::kSpectrumNoSize || stage_bytes > std::numeric_limits<size_t>::max() / 2 ||
        sum_bytes > std::numeric_limits<size_t>::max() / 2)
        rc = hipErrorOutOfMemory;
    if (rc == hipSuccess && (rc = hipMalloc((void**)&s.stage, (size_t)stage_bytes)) != hipSuccess) s.stage = nullptr;
    if (rc == hipSuccess && (rc = hipMalloc((void**)&s.acc, (size_t)sum_bytes)) != hipSuccess) s.acc = nullptr;
    for (int i = 0; i < 2 && rc == hipSuccess; ++i) {
        if ((rc = hipMalloc((void**)&s.tw_dev[i], table_bytes)) != hipSuccess) {
            s.tw_dev[i] = nullptr;
            break;
        }
        if ((rc = hipHostMalloc((void**)&s.tw_host[i], table_bytes, hipHostMallocDefault)) != hipSuccess) {
            s.tw_host[i] = nullptr;
            break;
        }
        if ((rc = hipEventCreate(&s.begun[i])) != hipSuccess) break;
        if ((rc = hipEventCreate(&s.folded_ev[i])) != hipSuccess) break;
    }
    if (rc == hipSuccess) rc = hipMemsetAsync(s.acc, 0, (size_t)sum_bytes, stream_);  // (+0.0 everywhere)
    if (rc == hipSuccess) rc = hipStreamSynchronize(stream_);
    if (rc != hipSuccess) {
        (void)hipGetLastError();  // nothing sticky
        spectrum_release(s);
        wv::note_hip_error(rc);
        return fail(WV_E_HIP, std::string("wv_set_spectrum: no room for the stage and the sums: ") + hipGetErrorString(rc));
    }
    spectrum_release(spec_);
    spec_ = std::move(s);
    spec_.st.start(plan->first_step, plan->period, steps_done);
    spec_.active = true;
    return WV_OK;
}

// The capture of `step`, which the field `current` holds once everything enqueued on the compute stream so far has run: into the
// slot behind the ones staged.
template <typename Real>
int Engine<Real>::spectrum_capture(uint64_t step) {
    Spectrum& s = spec_;
    // (spectrum_plan_batch gives a batch no more captures than the stage has free slots)
    if (s.st.full()) return fail(WV_E_STATE, "wv_run: the spectrum stage is full");
    const int rc = launch_snapshot_gather(s.box, s.gather_wide, s.stage + (uint64_t)s.st.slot() * s.nodes);  // (engine_snapshot.hip.h)
    if (rc) return rc;
    s.st.staged(step);
    return WV_OK;
}

// The time of the fold that last used table buffer `b`, once it has run (kernel timing on).
template <typename Real>
int Engine<Real>::spectrum_drain_timing(int b) {
    Spectrum& s = spec_;
    if (!s.timed[b]) return WV_OK;
    WV_HIP(hipEventSynchronize(s.folded_ev[b]));
    float ms = 0;
    WV_HIP(hipEventElapsedTime(&ms, s.begun[b], s.folded_ev[b]));
    s.kernel_ms += ms;
    s.timed[b] = false;
    return WV_OK;
}

// All committed captures -> the sums, one launch.  Only between batches, where nothing uncommitted is staged -- but for what a
// failed run left, which goes first: the stage is filled from slot 0 again behind a fold.
template <typename Real>
int Engine<Real>::spectrum_fold() {
    Spectrum& s = spec_;
    s.st.drop_uncommitted();
    const int t = s.st.committed;
    if (t == 0) return WV_OK;
    const int b = s.table;
    // the fold before last used this buffer: its copy has long left the host's table (a wait only if the device is two folds behind)
    if (s.table_used[b]) WV_HIP(hipEventSynchronize(s.folded_ev[b]));
    int rc = spectrum_drain_timing(b);
    if (rc) return rc;
    const uint32_t K = s.plan.n_freqs;
    for (int j = 0; j < t; ++j)
        for (uint32_t k = 0; k < K; ++k) {
            double* w = s.tw_host[b] + wv::spectrum_table_index((uint32_t)j, k, K);
            wv::spectrum_twiddle(s.freqs[k], s.st.steps[(size_t)j], w, w + 1);
        }
    WV_HIP(hipMemcpyAsync(s.tw_dev[b], s.tw_host[b], (size_t)t * K * 2 * sizeof(double), hipMemcpyHostToDevice, stream_));
    const uint64_t items = s.fold_wide ? s.nodes / 2 : s.nodes;
    const uint64_t blocks = (items + 255) / 256;
    if (blocks > 0x7fffffffull) return fail(WV_E_STATE, "wv_set_spectrum: the box has more nodes than one launch covers");
    if (timing) {
        WV_HIP(hipEventRecord(s.begun[b], stream_));
        s.timed[b] = true;
    }
    if (s.fold_wide)
        hipLaunchKernelGGL((wv::spectrum_fold_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, stream_, s.stage, s.acc, s.tw_dev[b], s.nodes, (int32_t)t, (int32_t)K);
    else
        hipLaunchKernelGGL((wv::spectrum_fold_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, stream_, s.stage, s.acc, s.tw_dev[b], s.nodes, (int32_t)t, (int32_t)K);
    WV_HIP(hipGetLastError());
    WV_HIP(hipEventRecord(s.folded_ev[b], stream_));
    s.table_used[b] = true;
    s.table = 1 - b;
    ++s.folds;
    s.st.all_folded();
    return WV_OK;
}

// Before a batch is planned: the fold when the stage has no slot left, and where the batch ends at the latest -- on the last capture
// the stage has a slot for (one capture per batch under graph replay: a replayed graph covers the whole batch).
template <typename Real>
int Engine<Real>::spectrum_plan_batch() {
    Spectrum& s = spec_;
    if (s.st.fold_due()) {
        const int rc = spectrum_fold();
        if (rc) return rc;
    }
    s.st.plan_batch_end(opt_.tuning.graph != 0);
    return WV_OK;
}

// On entering wv_run: steps taken by wv_step / wv_swap capture nothing, so plan steps they passed are passed; a capture of the step
// the engine stands at is due now (and is of a completed step: committed at once).
template <typename Real>
int Engine<Real>::spectrum_begin_run() {
    Spectrum& s = spec_;
    if (s.st.begin_run(steps_done)) {
        int rc = s.st.fold_due() ? spectrum_fold() : WV_OK;
        if (rc) return rc;
        if ((rc = spectrum_capture(steps_done))) return rc;
        s.st.commit(steps_done);
    }
    return WV_OK;
}

// wv_checkpoint under a plan: the sums (everything staged folded in first) and the count aside; the copy is allocated by the first
// checkpoint taken under the plan.  Called before the checkpoint touches anything: no room -> WV_E_HIP, engine untouched.
template <typename Real>
int Engine<Real>::spectrum_checkpoint() {
    Spectrum& s = spec_;
    const size_t bytes = (size_t)wv::spectrum_sum_bytes(s.nodes, s.plan.n_freqs);
    if (!ckpt_.spec_acc || ckpt_.spec_bytes != bytes) {
        if (ckpt_.spec_acc) (void)hipFree(ckpt_.spec_acc);
        ckpt_.spec_acc = nullptr;
        ckpt_.spec_bytes = 0;
        const hipError_t rc = hipMalloc((void**)&ckpt_.spec_acc, bytes);
        if (rc != hipSuccess) {
            ckpt_.spec_acc = nullptr;
            (void)hipGetLastError();
            return fail(WV_E_HIP, std::string("wv_checkpoint: no room for a copy of the spectrum's sums: ") + hipGetErrorString(rc));
        }
        ckpt_.spec_bytes = bytes;
    }
    const int rc = spectrum_fold();
    if (rc) return rc;
    WV_HIP(hipMemcpyAsync(ckpt_.spec_acc, s.acc, bytes, hipMemcpyDeviceToDevice, stream_));
    ckpt_.spec_captures = s.st.folded;
    ckpt_.spec_last_step = s.st.last_step;
    ckpt_.spec_next = s.st.next;
    return WV_OK;
}

// wv_rollback (the plan is the one the checkpoint saw): sums and count back, what is staged forgotten; the re-run takes it again.
template <typename Real>
int Engine<Real>::spectrum_rollback() {
    Spectrum& s = spec_;
    WV_HIP(hipMemcpyAsync(s.acc, ckpt_.spec_acc, ckpt_.spec_bytes, hipMemcpyDeviceToDevice, stream_));
    s.st.rollback(ckpt_.spec_captures, ckpt_.spec_last_step, ckpt_.spec_next);
    return WV_OK;
}

template <typename Real>
int Engine<Real>::spectrum_count(uint64_t* captures, uint64_t* last_step) {
    if (!spec_.active) return fail(WV_E_STATE, "wv_spectrum_count: no spectrum plan is set");
    if (captures) *captures = spec_.st.captures();
    if (last_step) *last_step = spec_.st.last_step;
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
    int rc = spectrum_fold();
    if (rc) return rc;
    WV_HIP(hipStreamSynchronize(stream_));
    for (int b = 0; b < 2; ++b)
        if ((rc = spectrum_drain_timing(b))) return rc;
    std::vector<double> planes((size_t)s.nodes * 2);
    for (uint32_t k = 0; k < s.plan.n_freqs; ++k) {
        WV_HIP(hipMemcpy(planes.data(), s.acc + (uint64_t)k * 2 * s.nodes, planes.size() * sizeof(double), hipMemcpyDeviceToHost));
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

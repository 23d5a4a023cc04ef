// engine_staged.hip.h -- the life cycle of the nine plans that accumulate on the device while wv_run keeps going: field spectra
// (engine_spectrum.hip.h), energy decay maps plain and banded (engine_decay.hip.h), intensity maps (engine_intensity.hip.h),
// arrival-aligned energy maps (engine_arrival.hip.h), lateral maps (engine_lateral.hip.h), modulation maps (engine_modulation.hip.h), band-limited arrival maps (engine_arrival_bands.hip.h), waterfall maps (engine_waterfall.hip.h) and interaural maps (engine_interaural.hip.h).  One copy of each step; what a plan's own
// file keeps is its setter's validation, sizes and first contents, the enqueue step of its fold and its fetch -- and
// of those the pieces more than one plan has are here too: the host-written tables of a fold (HostTable: bins, twiddles), the threshold
// map of the plans that find an onset, the fetch of complex sums.
//
// Part of the engine behind the C ABI of include/wayverb_amd.h (engine.hip is the translation unit; see engine.hip.h for the class).
//
// Everything runs on the compute stream, in order:
//   capture   snapshot_gather_kernel, intensity_gather_kernel for a plan that integrates velocities, or ear_gather_kernel for the plan
//             that reads two nodes per node taken (all three launched in engine_snapshot.hip.h) -> the next free slot of the device-only stage, directly behind the pass that produced the step.
//             A plan step is the end of a pass exactly as a snapshot step is: engine_batch.hip.h cuts its batches and segments at
//             whichever plan is active (they all exclude each other: plan_refused).
//   commit    a batch's captures stay staged until commit_batch has said how many of its steps were good; those of later steps are
//             dropped (CaptureStage::commit, capture_stage.h: the stage's integer bookkeeping).  A capture of a step that was never
//             completed is never folded in.
//   fold      the plan's fold kernel takes all staged captures into the plan's state blocks in ONE launch, and only when the stage has
//             no slot left for the next batch -- or on fetch and checkpoint.  (A new plan, a NULL plan and wv_destroy fold nothing: the
//             state is forgotten with the stage.)  Never because a batch ended: a fold moves the whole state whatever the number of
//             captures.
// In-order execution is what keeps a slot from being overwritten before the fold has read it: captures of the next batch are
// enqueued behind the fold.  The state is only ever touched by a fold, and a fold only ever sees committed captures.
#pragma once
#include <cmath>

#include "engine.hip.h"

namespace wv {

static_assert(kDecayStage == kSpectrumStage && kIntensityStage == kSpectrumStage && kArrivalStage == kSpectrumStage && kLateralStage == kSpectrumStage &&
                      kModulationStage == kSpectrumStage && kArrivalBandsStage == kSpectrumStage && kWaterfallStage == kSpectrumStage &&
                      kInterauralStage == kSpectrumStage,
              "every plan stages its captures by spectrum_plan.h's rules (capture_stage.h)");

// What every plan's setter, wv_set_snapshots included, refuses a plan for before it looks at it: a slab of a chain (it would have to cut
// its batches where its neighbours do, and holds only its part of a box), and another plan being active -- every plan wants to decide
// where passes end: one consumer of capture steps at a time.  `self`: the caller's own row (setting a plan again replaces it).
template <typename Real>
int Engine<Real>::plan_refused(const std::string& setter, PlanRow self) {
    if (opt_.ghost_lo || opt_.ghost_hi || (comm_ && comm_->nranks() > 1)) return fail(WV_E_STATE, setter + ": not on a slab of a chain (one domain only)");
    const struct {
        PlanRow row;
        bool active;
        const char* sentence;
    } rows[] = {
        {kSnapshotRow, snap_.active, "a snapshot plan is active (wv_set_snapshots(e, NULL) stops it); the plans exclude each other"},
        {kSpectrumRow, spec_.active, "a spectrum plan is active (wv_set_spectrum(e, NULL, NULL) stops it); the plans exclude each other"},
        {kBandedDecayRow, decay_.active && decay_.n_bands != 0, "a banded decay plan is active (wv_set_decay_bands(e, NULL, NULL, 0, 0) stops it); the plans exclude each other"},
        {kPlainDecayRow, decay_.active && decay_.n_bands == 0, "a decay plan is active (wv_set_decay(e, NULL) stops it); the plans exclude each other"},
        {kIntensityRow, inten_.active, "an intensity plan is active (wv_set_intensity(e, NULL) stops it); the plans exclude each other"},
        {kArrivalRow, arr_.active, "an arrival plan is active (wv_set_arrival(e, NULL, NULL) stops it); the plans exclude each other"},
        {kLateralRow, lat_.active, "a lateral plan is active (wv_set_lateral(e, NULL, NULL) stops it); the plans exclude each other"},
        {kModulationRow, mod_.active, "a modulation plan is active (wv_set_modulation(e, NULL, NULL, NULL, 0, 0) stops it); the plans exclude each other"},
        {kArrivalBandsRow, arrb_.active, "a banded arrival plan is active (wv_set_arrival_bands(e, NULL, NULL, NULL, 0, 0) stops it); the plans exclude each other"},
        {kWaterfallRow, wf_.active, "a waterfall plan is active (wv_set_waterfall(e, NULL, NULL) stops it); the plans exclude each other"},
        {kInterauralRow, ia_.active, "an interaural plan is active (wv_set_interaural(e, NULL, NULL, NULL) stops it); the plans exclude each other"},
    };
    for (const auto& r : rows)
        if (r.active && r.row != self) return fail(WV_E_STATE, setter + ": " + r.sentence);
    return WV_OK;
}

// Stage, state blocks, events and what the plan's own struct holds beside them (free_own) freed; the generation stays.
template <typename Real>
template <typename Plan>
void Engine<Real>::plan_release(Plan& p) {
    p.free_own();
    if (p.stage) (void)hipFree(p.stage);
    for (unsigned char* block : p.block)
        if (block) (void)hipFree(block);
    for (int i = 0; i < 2; ++i) {
        if (p.begun[i]) (void)hipEventDestroy(p.begun[i]);
        if (p.folded_ev[i]) (void)hipEventDestroy(p.folded_ev[i]);
    }
    for (int i = 0; i < kSpectrumStage; ++i) {
        if (p.gather_begun[i]) (void)hipEventDestroy(p.gather_begun[i]);
        if (p.gather_done[i]) (void)hipEventDestroy(p.gather_done[i]);
    }
    const uint64_t generation = p.generation;
    p = Plan{};
    p.generation = generation;
}

template <typename Real>
void Engine<Real>::staged_release(StagedPlan& p) {
    switch (p.kind) {
        case kSpectrumPlan: plan_release(static_cast<Spectrum&>(p)); break;
        case kDecayPlan: plan_release(static_cast<Decay&>(p)); break;
        case kIntensityPlan: plan_release(static_cast<Intensity&>(p)); break;
        case kArrivalPlan: plan_release(static_cast<Arrival&>(p)); break;
        case kLateralPlan: plan_release(static_cast<Lateral&>(p)); break;
        case kModulationPlan: plan_release(static_cast<Modulation&>(p)); break;
        case kArrivalBandsPlan: plan_release(static_cast<ArrivalBands&>(p)); break;
        case kWaterfallPlan: plan_release(static_cast<Waterfall&>(p)); break;
        default: plan_release(static_cast<Interaural&>(p)); break;
    }
}

// A setter given a NULL plan: the plan stops and its state is forgotten.
template <typename Real>
template <typename Plan>
int Engine<Real>::staged_stop(Plan& p) {
    WV_HIP(hipStreamSynchronize(stream_));
    plan_release(p);
    ++p.generation;
    return WV_OK;
}

// A setter's candidate gets its stage, its state blocks (their sizes kept for checkpoints) and its events.  Everything is allocated
// aside, and only a complete set takes the old plan's place (staged_install): no room -> WV_E_HIP, engine untouched.
template <typename Real>
hipError_t Engine<Real>::staged_allocate(StagedPlan& c, uint64_t stage_bytes, uint64_t block0_bytes, uint64_t block1_bytes) {
    const uint64_t most = std::numeric_limits<size_t>::max() / 2;  // (a size that does not fit 64 bits is all bits set)
    if (stage_bytes > most || block0_bytes > most || block1_bytes > most) return hipErrorOutOfMemory;
    hipError_t rc = hipMalloc((void**)&c.stage, (size_t)stage_bytes);
    if (rc != hipSuccess) {
        c.stage = nullptr;
        return rc;
    }
    const uint64_t bytes[kPlanBlocks] = {block0_bytes, block1_bytes};
    for (int i = 0; i < kPlanBlocks && bytes[i]; ++i) {
        if ((rc = hipMalloc((void**)&c.block[i], (size_t)bytes[i])) != hipSuccess) {
            c.block[i] = nullptr;
            return rc;
        }
        c.block_bytes[i] = (size_t)bytes[i];
        c.n_blocks = i + 1;
    }
    for (int i = 0; i < 2; ++i) {
        if ((rc = hipEventCreate(&c.begun[i])) != hipSuccess) return rc;
        if ((rc = hipEventCreate(&c.folded_ev[i])) != hipSuccess) return rc;
    }
    for (int i = 0; i < kSpectrumStage && c.gradients; ++i) {
        if ((rc = hipEventCreate(&c.gather_begun[i])) != hipSuccess) return rc;
        if ((rc = hipEventCreate(&c.gather_done[i])) != hipSuccess) return rc;
    }
    return hipSuccess;
}

// Both buffers of a host-written table and their device copies (a candidate's: what is missing stays null and plan_release frees the rest).
template <typename Real>
template <typename T>
hipError_t Engine<Real>::host_table_allocate(HostTable<T>& table, size_t bytes) {
    for (int i = 0; i < 2; ++i) {
        hipError_t rc = hipMalloc((void**)&table.dev[i], bytes);
        if (rc != hipSuccess) {
            table.dev[i] = nullptr;
            return rc;
        }
        if ((rc = hipHostMalloc((void**)&table.host[i], bytes, hipHostMallocDefault)) != hipSuccess) {
            table.host[i] = nullptr;
            return rc;
        }
    }
    return hipSuccess;
}

template <typename Real>
template <typename T>
void Engine<Real>::host_table_free(HostTable<T>& table) {
    for (int i = 0; i < 2; ++i) {
        if (table.dev[i]) (void)hipFree(table.dev[i]);
        if (table.host[i]) (void)hipHostFree(table.host[i]);
    }
}

// x = f * step, its fractional part, cos and sin of 2 pi x: three rounded operations ahead of libm, so that NumPy evaluating the
// same three gives the same argument (include/wayverb_amd.h: wv_spectrum_twiddle)
inline void spectrum_twiddle(double cycles_per_step, uint64_t step, double* c, double* s) {
    double x = cycles_per_step * (double)step;
    x -= std::floor(x);
    const double angle = 6.283185307179586476925286766559 * x;
    *c = std::cos(angle);
    *s = std::sin(angle);
}

// Turn b's twiddles for a fold of plan p's t staged captures, double[t][K][2]: cos and sin of capture j's step at each of the K
// frequencies, and the copy.
template <typename Real>
int Engine<Real>::twiddle_table_write(TwiddleTable& table, const StagedPlan& p, int b, int t, const std::vector<double>& freqs) {
    const uint32_t K = (uint32_t)freqs.size();
    for (int j = 0; j < t; ++j)
        for (uint32_t k = 0; k < K; ++k) {
            double* w = table.host[b] + wv::spectrum_table_index((uint32_t)j, k, K);
            wv::spectrum_twiddle(freqs[k], p.st.steps[(size_t)j], w, w + 1);
        }
    WV_HIP(hipMemcpyAsync(table.dev[b], table.host[b], (size_t)t * K * 2 * sizeof(double), hipMemcpyHostToDevice, stream_));
    return WV_OK;
}

// A fetch of complex sums: the Re plane at `re_plane` on the device and the Im plane behind it -> out[B][2], by way of the caller's
// `planes` (2 B doubles, allocated once per fetch).
template <typename Real>
int Engine<Real>::fetch_interleaved(const double* re_plane, uint64_t nodes, double* out, std::vector<double>& planes) {
    WV_HIP(hipMemcpy(planes.data(), re_plane, planes.size() * sizeof(double), hipMemcpyDeviceToHost));
    const double *re = planes.data(), *im = planes.data() + nodes;
    for (uint64_t i = 0; i < nodes; ++i) {
        out[2 * i] = re[i];
        out[2 * i + 1] = im[i];
    }
    return WV_OK;
}

// A setter's threshold map (NULL: none): refused for an entry that the plan's scalar would be refused for ...
template <typename Real>
int Engine<Real>::threshold_map_refused(const char* setter, const float* map, uint64_t nodes) {
    for (uint64_t i = 0; map && i < nodes; ++i)
        if (!wv::arrival_threshold_valid(map[i])) return fail(WV_E_INVALID_ARGUMENT, std::string(setter) + ": every entry of the threshold map must be >= 0 and finite");
    return WV_OK;
}

// ... and allocated and copied to the device beside a candidate's state.
template <typename Real>
hipError_t Engine<Real>::threshold_map_upload(float*& dev, const float* map, uint64_t nodes) {
    if (!map) return hipSuccess;
    const size_t bytes = (size_t)wv::arrival_map_bytes(nodes);
    const hipError_t rc = hipMalloc((void**)&dev, bytes);
    if (rc != hipSuccess) {
        dev = nullptr;
        return rc;
    }
    return hipMemcpyAsync(dev, map, bytes, hipMemcpyHostToDevice, stream_);
}

// The end of a setter: `rc` is what allocating and filling the candidate came to.  The candidate's first contents are on the device
// (and the caller's arrays read: pageable memory, the copies have left them) when the call returns.
template <typename Real>
template <typename Plan>
int Engine<Real>::staged_install(Plan& current, Plan& candidate, hipError_t rc, const std::string& no_room, uint64_t first_step, uint64_t period) {
    if (rc == hipSuccess) rc = hipStreamSynchronize(stream_);
    if (rc != hipSuccess) {
        (void)hipGetLastError();  // nothing sticky
        plan_release(candidate);
        wv::note_hip_error(rc);
        return fail(WV_E_HIP, no_room + ": " + hipGetErrorString(rc));
    }
    const uint64_t generation = current.generation + 1;
    plan_release(current);
    current = std::move(candidate);
    current.generation = generation;
    current.st.start(first_step, period, steps_done);
    current.active = true;
    return WV_OK;
}

// The capture of `step`, which the field `current` holds once everything enqueued on the compute stream so far has run: into the
// slot behind the ones staged.
template <typename Real>
int Engine<Real>::staged_capture(StagedPlan& p, uint64_t step) {
    // (staged_plan_batch gives a batch no more captures than the stage has free slots)
    if (p.st.full()) return fail(WV_E_STATE, std::string("wv_run: the ") + p.name + " stage is full");
    const int slot = p.st.slot();
    if (p.st.folded + (uint64_t)slot >= p.max_captures) return fail(WV_E_STATE, std::string("wv_run: the ") + p.name + " plan has counted 2^32 - 1 captures");
    if (p.gradients) {
        if (timing) WV_HIP(hipEventRecord(p.gather_begun[slot], stream_));
        const int rc = launch_intensity_gather(p.box, p.spacing, p.stage + (uint64_t)slot * wv::kIntensityPlanes * p.nodes);
        if (rc) return rc;
        if (timing) {
            WV_HIP(hipEventRecord(p.gather_done[slot], stream_));
            p.gather_timed[slot] = true;
        }
    } else if (p.ears) {
        const int rc = launch_ear_gather(p.box, p.ear_a, p.ear_b, p.stage + (uint64_t)slot * 2 * p.nodes);
        if (rc) return rc;
    } else {
        const int rc = launch_snapshot_gather(p.box, p.gather_wide, p.stage + (uint64_t)slot * p.nodes);
        if (rc) return rc;
    }
    p.st.staged(step);
    return WV_OK;
}

// The times of the folds that took turn `turn` (-1: either) and of the captures, where they ran with kernel timing on, once they
// have run.
template <typename Real>
int Engine<Real>::staged_drain_timing(StagedPlan& p, int turn) {
    for (int b = 0; b < 2; ++b) {
        if (!p.timed[b] || (turn >= 0 && b != turn)) continue;
        WV_HIP(hipEventSynchronize(p.folded_ev[b]));
        float ms = 0;
        WV_HIP(hipEventElapsedTime(&ms, p.begun[b], p.folded_ev[b]));
        p.kernel_ms += ms;
        p.timed[b] = false;
    }
    for (int i = 0; i < kSpectrumStage; ++i) {
        if (!p.gather_timed[i]) continue;
        WV_HIP(hipEventSynchronize(p.gather_done[i]));
        float ms = 0;
        WV_HIP(hipEventElapsedTime(&ms, p.gather_begun[i], p.gather_done[i]));
        p.gather_ms += ms;
        ++p.gathers_timed;
        p.gather_timed[i] = false;
    }
    return WV_OK;
}

// A plan's enqueue step calls this between its table's copy, if it has one, and its kernel: the fold's time is the kernel's.
template <typename Real>
int Engine<Real>::staged_fold_begins(StagedPlan& p, int b) {
    if (timing) WV_HIP(hipEventRecord(p.begun[b], stream_));
    return WV_OK;
}

// The one thing of a fold that is a plan's own: its table written and copied, if it has one, staged_fold_begins, its kernel launched
// over `blocks` workgroups of 256 for the `t` staged captures, with turn `b`'s table.
template <typename Real>
int Engine<Real>::staged_enqueue(StagedPlan& p, int b, int t, unsigned blocks) {
    switch (p.kind) {
        case kSpectrumPlan: return spectrum_enqueue(static_cast<Spectrum&>(p), b, t, blocks);
        case kDecayPlan: return decay_enqueue(static_cast<Decay&>(p), b, t, blocks);
        case kIntensityPlan: return intensity_enqueue(static_cast<Intensity&>(p), b, t, blocks);
        case kArrivalPlan: return arrival_enqueue(static_cast<Arrival&>(p), b, t, blocks);
        case kLateralPlan: return lateral_enqueue(static_cast<Lateral&>(p), b, t, blocks);
        case kModulationPlan: return modulation_enqueue(static_cast<Modulation&>(p), b, t, blocks);
        case kArrivalBandsPlan: return arrival_bands_enqueue(static_cast<ArrivalBands&>(p), b, t, blocks);
        case kWaterfallPlan: return waterfall_enqueue(static_cast<Waterfall&>(p), b, t, blocks);
        default: return interaural_enqueue(static_cast<Interaural&>(p), b, t, blocks);
    }
}

// All committed captures -> the state, one launch.  Only between batches, where nothing uncommitted is staged -- but for what a
// failed run left, which goes first: the stage is filled from slot 0 again behind a fold.
template <typename Real>
int Engine<Real>::staged_fold(StagedPlan& p) {
    p.st.drop_uncommitted();
    const int t = p.st.committed;
    if (t == 0) return WV_OK;
    const uint64_t blocks = ((p.fold_wide ? p.nodes / 2 : p.nodes) + 255) / 256;
    if (blocks > 0x7fffffffull) return fail(WV_E_STATE, std::string(p.setter) + ": the box has more nodes than one launch covers");
    const int b = p.turn;
    // a host-written table: the fold before last used this one, and its copy has long left the host's (a wait only if the device is two
    // folds behind).  Without a table, and without kernel timing, a fold records no event and the host waits for nothing
    if (p.host_table && p.used[b]) WV_HIP(hipEventSynchronize(p.folded_ev[b]));
    // (the fold before last recorded this pair; the slots' event pairs are recorded again by the captures behind this fold)
    int rc = staged_drain_timing(p, b);
    if (rc) return rc;
    if ((rc = staged_enqueue(p, b, t, (unsigned)blocks))) return rc;
    WV_HIP(hipGetLastError());
    if (p.host_table || timing) {
        WV_HIP(hipEventRecord(p.folded_ev[b], stream_));
        p.timed[b] = timing;
        p.used[b] = true;
        p.turn = 1 - b;
    }
    ++p.folds;
    p.st.all_folded();
    return WV_OK;
}

// Ahead of a fetch: what is staged folded in, the state at rest, the timing drained.  The plan keeps running.
template <typename Real>
int Engine<Real>::staged_settle(StagedPlan& p) {
    const int rc = staged_fold(p);
    if (rc) return rc;
    WV_HIP(hipStreamSynchronize(stream_));
    return staged_drain_timing(p);
}

// WV_QUERY_*_NS, *_GATHER_NS, *_GATHERS: the kernel times summed so far, once the timed folds and captures have run.
template <typename Real>
int Engine<Real>::staged_time_query(StagedPlan& p, PlanTime what, uint64_t* value) {
    DeviceGuard guard(device_);
    const int rc = staged_drain_timing(p);
    if (rc) return rc;
    *value = what == PlanTime::gathers ? p.gathers_timed : (uint64_t)((what == PlanTime::folds_ns ? p.kernel_ms : p.gather_ms) * 1e6 + 0.5);
    return WV_OK;
}

// Before a batch is planned: the fold when the stage has no slot left, and where the batch ends at the latest -- on the last capture
// the stage has a slot for (one capture per batch under graph replay: a replayed graph covers the whole batch).
template <typename Real>
int Engine<Real>::staged_plan_batch(StagedPlan& p) {
    if (p.st.fold_due()) {
        const int rc = staged_fold(p);
        if (rc) return rc;
    }
    p.st.plan_batch_end(opt_.tuning.graph != 0);
    return WV_OK;
}

// On entering wv_run: steps taken by wv_step / wv_swap capture nothing, so plan steps they passed are passed; a capture of the step
// the engine stands at is due now (and is of a completed step: committed at once).
template <typename Real>
int Engine<Real>::staged_begin_run(StagedPlan& p) {
    if (p.st.begin_run(steps_done)) {
        int rc = p.st.fold_due() ? staged_fold(p) : WV_OK;
        if (rc) return rc;
        if ((rc = staged_capture(p, steps_done))) return rc;
        p.st.commit(steps_done);
    }
    return WV_OK;
}

template <typename Real>
int Engine<Real>::staged_count(const StagedPlan& p, uint64_t* captures, uint64_t* last_step) {
    if (!p.active) return fail(WV_E_STATE, std::string("wv_") + p.name + "_count: no " + p.name + " plan is set");
    if (captures) *captures = p.st.captures();
    if (last_step) *last_step = p.st.last_step;
    return WV_OK;
}

// wv_checkpoint under a plan: the state blocks (everything staged folded in first), the count and the next plan step aside; the
// copies are allocated by the first checkpoint taken under the plan.  Called before the checkpoint touches anything: no room ->
// WV_E_HIP, engine untouched.
template <typename Real>
int Engine<Real>::staged_checkpoint(StagedPlan& p) {
    typename Checkpoint::PlanSave& save = ckpt_.plan[p.kind];
    for (int i = p.n_blocks - 1; i >= 0; --i) {
        if (save.block[i] && save.bytes[i] == p.block_bytes[i]) continue;
        if (save.block[i]) (void)hipFree(save.block[i]);
        save.block[i] = nullptr;
        save.bytes[i] = 0;
        const hipError_t rc = hipMalloc((void**)&save.block[i], p.block_bytes[i]);
        if (rc != hipSuccess) {
            save.block[i] = nullptr;
            (void)hipGetLastError();
            return fail(WV_E_HIP, std::string("wv_checkpoint: no room for a copy of ") + p.block_name[i] + ": " + hipGetErrorString(rc));
        }
        save.bytes[i] = p.block_bytes[i];
    }
    const int rc = staged_fold(p);
    if (rc) return rc;
    for (int i = 0; i < p.n_blocks; ++i) WV_HIP(hipMemcpyAsync(save.block[i], p.block[i], p.block_bytes[i], hipMemcpyDeviceToDevice, stream_));
    save.captures = p.st.folded;
    save.last_step = p.st.last_step;
    save.next = p.st.next;
    return WV_OK;
}

// wv_rollback (the plan is the one the checkpoint saw): state and count back, what is staged forgotten; the re-run takes it again.
template <typename Real>
int Engine<Real>::staged_rollback(StagedPlan& p) {
    const typename Checkpoint::PlanSave& save = ckpt_.plan[p.kind];
    for (int i = 0; i < p.n_blocks; ++i) WV_HIP(hipMemcpyAsync(p.block[i], save.block[i], save.bytes[i], hipMemcpyDeviceToDevice, stream_));
    p.st.rollback(save.captures, save.last_step, save.next);
    return WV_OK;
}

}  // namespace wv

// engine_snapshot.hip.h -- wv_set_snapshots / wv_snapshot_count / wv_fetch_snapshots: a box of the field, decimated, captured by the
// engine itself every `period` steps while wv_run keeps going (the mesh-pressure visualiser of the reference's application hangs off
// the per-step callback, src/combined/src/engine.cpp:158-169; here the field does not have to stop for it).
//
// Part of the engine behind the C ABI of include/wayverb_amd.h (engine.hip is the translation unit; see engine.hip.h for the class).
//
// The pipeline, per snapshot:
//   compute stream   [wait: the slot's previous copy, only when the ring has wrapped]  snapshot_gather_kernel -> device slot; event
//   copy stream      wait for that event; hipMemcpyAsync device slot -> page-locked host slot; event
//   host             before the next batch is planned and on leaving wv_run: host slots whose copy has landed -> the held log
// The capture cannot wait -- two steps (or two passes) later the field it reads is overwritten -- so it runs on the compute stream
// directly behind the pass that produced the step; everything after it is off that stream.  A snapshot step is always the end of a
// pass -- the only place where single steps, two- and three-step passes hold the step as a whole field -- and nothing of the step
// behind it rides in that pass's launches (engine_batch.hip.h: segments of a batch); under graph replay it is the end of the batch.
// A batch holds as many captures as the ring has free slots and ends on the last of them (snapshot_plan_batch).
#pragma once
#include "engine.hip.h"

namespace wv {

template <typename Real>
void Engine<Real>::snapshot_release(Snapshots& s) {
    if (s.copy_stream) (void)hipStreamSynchronize(s.copy_stream);
    for (int i = 0; i < kSnapSlots; ++i) {
        if (s.dev[i]) (void)hipFree(s.dev[i]);
        if (s.host[i]) (void)hipHostFree(s.host[i]);
        if (s.begun[i]) (void)hipEventDestroy(s.begun[i]);
        if (s.captured[i]) (void)hipEventDestroy(s.captured[i]);
        if (s.copied[i]) (void)hipEventDestroy(s.copied[i]);
    }
    if (s.copy_stream) (void)hipStreamDestroy(s.copy_stream);
    const uint64_t generation = s.generation;
    s = Snapshots{};
    s.generation = generation;
}

template <typename Real>
int Engine<Real>::set_snapshots(const wv_snapshot_plan* plan) {
    DeviceGuard guard(device_);
    if (!plan) {
        WV_HIP(hipStreamSynchronize(stream_));
        snapshot_release(snap_);
        ++snap_.generation;
        return WV_OK;
    }
    // (a slab of a chain would have to cut its batches where its neighbours do, and each rank holds only its part of a box: out of
    // scope, as for wv_checkpoint; an accumulating plan cuts the passes at its own steps: engine_staged.hip.h)
    if (const int rc = plan_refused("wv_set_snapshots", kSnapshotRow)) return rc;
    static const wv::PlanSentences says = WV_PLAN_SENTENCES("wv_set_snapshots");
    if (const char* why = wv::plan_refusal(*plan, nx_, ny_, nz_, says)) return fail(WV_E_INVALID_ARGUMENT, why);
    const wv::SnapshotBox box = wv::plan_box(*plan);
    // everything is allocated here, aside, and only a complete set takes the old plan's place: no room -> WV_E_HIP, engine untouched
    Snapshots s;
    s.generation = snap_.generation + 1;
    s.plan = *plan;
    s.box = box;
    s.elems = wv::snapshot_elements(box);
    const size_t bytes = (size_t)wv::snapshot_bytes(box);
    s.slots = bytes > (64ull << 20) ? 2 : kSnapSlots;
    s.wide = wv::gather_wide(box);
    hipError_t rc = hipStreamCreateWithFlags(&s.copy_stream, hipStreamNonBlocking);
    for (int i = 0; i < s.slots && rc == hipSuccess; ++i) {
        if ((rc = hipMalloc((void**)&s.dev[i], bytes)) != hipSuccess) {
            s.dev[i] = nullptr;
            break;
        }
        if ((rc = hipHostMalloc((void**)&s.host[i], bytes, hipHostMallocDefault)) != hipSuccess) {
            s.host[i] = nullptr;
            break;
        }
        if ((rc = hipEventCreate(&s.begun[i])) != hipSuccess) break;
        if ((rc = hipEventCreate(&s.captured[i])) != hipSuccess) break;
        if ((rc = hipEventCreateWithFlags(&s.copied[i], hipEventDisableTiming)) != hipSuccess) break;
    }
    if (rc != hipSuccess) {
        (void)hipGetLastError();  // nothing sticky
        snapshot_release(s);
        wv::note_hip_error(rc);
        return fail(WV_E_HIP, std::string("wv_set_snapshots: no room for the snapshot ring: ") + hipGetErrorString(rc));
    }
    WV_HIP(hipStreamSynchronize(stream_));
    snapshot_release(snap_);
    snap_ = std::move(s);
    snap_.set_at = steps_done;
    snap_.next = wv::snapshot_next_step(plan->first_step, plan->period, steps_done);
    snap_.active = true;
    return WV_OK;
}

// snapshot_gather_kernel on the compute stream: `box` of the field `current` -> the dense floats at `dst` (`wide`: four nodes per
// lane, snapshot_kernels.hip.h).  The one launch site of the kernel: a snapshot plan's captures and a spectrum, a decay and
// an arrival plan's (engine_staged.hip.h: staged_capture) are the same launch.
template <typename Real>
int Engine<Real>::launch_snapshot_gather(const wv::SnapshotBox& box, bool wide, float* dst) {
    wv::SnapshotArgs<Real> a{};
    a.field = field_[cur_];
    a.dst = dst;
    a.pitch = pitch_;
    a.mesh_ny = ny_;
    a.x0 = box.x0, a.y0 = box.y0, a.z0 = box.z0;
    a.nx = box.nx, a.ny = box.ny, a.nz = box.nz;
    a.sx = box.sx, a.sy = box.sy, a.sz = box.sz;
    // grid: x over the items of a dense plane, y over the planes (both with a stride loop behind them)
    const uint64_t items = (wide ? (uint64_t)box.nx / 4 : (uint64_t)box.nx) * (uint64_t)box.ny;
    const dim3 grid((unsigned)std::min<uint64_t>((items + 255) / 256, 1u << 14), (unsigned)std::min(box.nz, 1024));
    if (wide)
        hipLaunchKernelGGL((wv::snapshot_gather_kernel<Real, true>), grid, dim3(256), 0, stream_, a);
    else
        hipLaunchKernelGGL((wv::snapshot_gather_kernel<Real, false>), grid, dim3(256), 0, stream_, a);
    WV_HIP(hipGetLastError());
    return WV_OK;
}

// intensity_gather_kernel (intensity_kernels.hip.h) on the compute stream: per node of `box` the pressure and the three float
// differences of its neighbours' gradients, from the field `current` -> the four dense planes at `dst`.  The one launch site of that
// kernel (an intensity and a lateral plan's capture, engine_staged.hip.h: staged_capture); the box keeps clear of the mesh's faces (intensity_plan.h).
template <typename Real>
int Engine<Real>::launch_intensity_gather(const wv::SnapshotBox& box, double spacing, float* dst) {
    wv::IntensityGatherArgs<Real> a{};
    a.field = field_[cur_];
    a.dst = dst;
    a.pitch = pitch_;
    a.nodes = (int64_t)wv::snapshot_elements(box);
    a.mesh_ny = ny_;
    a.x0 = box.x0, a.y0 = box.y0, a.z0 = box.z0;
    a.nx = box.nx, a.ny = box.ny, a.nz = box.nz;
    a.sx = box.sx, a.sy = box.sy, a.sz = box.sz;
    a.spacing = spacing;
    const uint64_t items = (uint64_t)box.nx * (uint64_t)box.ny;
    const dim3 grid((unsigned)std::min<uint64_t>((items + 255) / 256, 1u << 14), (unsigned)std::min(box.nz, 1024));
    hipLaunchKernelGGL((wv::intensity_gather_kernel<Real>), grid, dim3(256), 0, stream_, a);
    WV_HIP(hipGetLastError());
    return WV_OK;
}

// ear_gather_kernel (interaural_kernels.hip.h) on the compute stream: per node of `box` the field at the node plus ear_a and at the node
// plus ear_b, from the field `current` -> the two dense planes at `dst`.  The one launch site of that kernel (an interaural plan's
// capture, engine_staged.hip.h: staged_capture); the setter has checked that both ears of every node lie on the mesh (interaural_plan.h).
template <typename Real>
int Engine<Real>::launch_ear_gather(const wv::SnapshotBox& box, const int32_t* ear_a, const int32_t* ear_b, float* dst) {
    wv::EarGatherArgs<Real> a{};
    a.field = field_[cur_];
    a.dst = dst;
    a.pitch = pitch_;
    a.nodes = (int64_t)wv::snapshot_elements(box);
    a.ear_a = ((int64_t)ear_a[2] * ny_ + ear_a[1]) * (int64_t)pitch_ + ear_a[0];
    a.ear_b = ((int64_t)ear_b[2] * ny_ + ear_b[1]) * (int64_t)pitch_ + ear_b[0];
    a.mesh_ny = ny_;
    a.x0 = box.x0, a.y0 = box.y0, a.z0 = box.z0;
    a.nx = box.nx, a.ny = box.ny, a.nz = box.nz;
    a.sx = box.sx, a.sy = box.sy, a.sz = box.sz;
    const uint64_t items = (uint64_t)box.nx * (uint64_t)box.ny;
    const dim3 grid((unsigned)std::min<uint64_t>((items + 255) / 256, 1u << 14), (unsigned)std::min(box.nz, 1024));
    hipLaunchKernelGGL((wv::ear_gather_kernel<Real>), grid, dim3(256), 0, stream_, a);
    WV_HIP(hipGetLastError());
    return WV_OK;
}

// The capture of `step`, which the field `current` holds once everything enqueued on the compute stream so far has run.
template <typename Real>
int Engine<Real>::snapshot_capture(uint64_t step) {
    Snapshots& s = snap_;
    const int slot = s.head;
    // (snapshot_plan_batch gives a batch no more captures than the ring has free slots)
    if ((int)s.pending.size() >= s.slots) return fail(WV_E_STATE, "wv_run: the snapshot ring is full");
    // the slot's previous copy must have left it: a stream wait, never a host wait
    if (s.used[slot]) WV_HIP(hipStreamWaitEvent(stream_, s.copied[slot], 0));
    s.timed[slot] = timing;
    if (timing) WV_HIP(hipEventRecord(s.begun[slot], stream_));
    const int rc = launch_snapshot_gather(s.box, s.wide, s.dev[slot]);
    if (rc) return rc;
    WV_HIP(hipEventRecord(s.captured[slot], stream_));
    WV_HIP(hipStreamWaitEvent(s.copy_stream, s.captured[slot], 0));
    WV_HIP(hipMemcpyAsync(s.host[slot], s.dev[slot], (size_t)s.elems * sizeof(float), hipMemcpyDeviceToHost, s.copy_stream));
    WV_HIP(hipEventRecord(s.copied[slot], s.copy_stream));
    s.used[slot] = true;
    s.head = (slot + 1) % s.slots;
    s.pending.push_back({slot, step});
    s.next = wv::snapshot_next_step(s.plan.first_step, s.plan.period, step + 1);
    return WV_OK;
}

// Captures whose copy has landed -> the held log, oldest first, `limit` at the most (`wait`: waiting for the copy stream).
template <typename Real>
int Engine<Real>::snapshot_harvest(bool wait, size_t limit) {
    Snapshots& s = snap_;
    for (size_t done = 0; done < limit && !s.pending.empty(); ++done) {
        const auto p = s.pending.front();
        if (wait) {
            WV_HIP(hipEventSynchronize(s.copied[p.slot]));
        } else {
            const hipError_t q = hipEventQuery(s.copied[p.slot]);
            if (q == hipErrorNotReady) {
                (void)hipGetLastError();  // (not a failure: nothing may be left for a later hipGetLastError to find)
                break;
            }
            WV_HIP(q);
        }
        if (s.timed[p.slot]) {
            float ms = 0;
            WV_HIP(hipEventElapsedTime(&ms, s.begun[p.slot], s.captured[p.slot]));
            s.kernel_ms += ms;
            s.timed[p.slot] = false;
        }
        // (the memory of a snapshot that was dropped serves the next one: with `keep` set nothing is allocated once the log is full)
        std::vector<float> v;
        if (!s.spare.empty()) {
            v = std::move(s.spare.back());
            s.spare.pop_back();
        }
        v.resize(s.elems);
        std::memcpy(v.data(), s.host[p.slot], (size_t)s.elems * sizeof(float));
        s.held.emplace_back(p.step, std::move(v));
        if (s.taken == 0) s.first_taken_step = p.step;
        ++s.taken;
        s.bytes += s.elems * sizeof(float);
        if (s.plan.keep)
            while (s.held.size() > s.plan.keep) {
                if (s.spare.size() < 2) s.spare.push_back(std::move(s.held.front().second));
                s.held.pop_front();
            }
        s.pending.pop_front();
    }
    return WV_OK;
}

// The batch stopped on a flag: its captures of steps behind the last completed one are of no completed step.  (Their copies may
// still be on their way; each slot's event guards the slot as for any other.)
template <typename Real>
void Engine<Real>::snapshot_discard_after(uint64_t last_good_step) {
    while (!snap_.pending.empty() && snap_.pending.back().step > last_good_step) {
        snap_.next = snap_.pending.back().step;
        snap_.pending.pop_back();
    }
}

// Before a batch is planned.  The batch is given its end: it may hold captures for half the ring (each between two passes, the last
// at its end), so that the other half can still hold the batch before's, whose copies are taken over by the host while this batch
// keeps the device busy (run: snapshot_harvest behind the enqueueing) -- and never a capture of this batch, which is of no
// committed step until the batch's flag words are in.  Only a ring without a free slot is waited for here.  With graph replay
// on, one capture per batch, at its end: a replayed graph covers the whole batch.
template <typename Real>
int Engine<Real>::snapshot_plan_batch() {
    Snapshots& s = snap_;
    while ((int)s.pending.size() >= s.slots) {  // (the copies have fallen a whole ring behind: the one host wait of the pipeline)
        const int rc = snapshot_harvest(true, 1);
        if (rc) return rc;
    }
    s.committed = s.pending.size();
    int room = opt_.tuning.graph != 0 ? 1 : std::max(1, std::min(s.slots / 2, s.slots - (int)s.pending.size()));
    uint64_t end = s.next;
    for (; room > 1 && end != wv::kNoSnapshotStep; --room) end = wv::snapshot_next_step(s.plan.first_step, s.plan.period, end + 1);
    s.batch_end = end == wv::kNoSnapshotStep ? s.next : end;
    return WV_OK;
}

// On entering wv_run: steps taken by wv_step / wv_swap record nothing, so snapshot steps they passed are passed; a snapshot of the
// step the engine stands at is due now.
template <typename Real>
int Engine<Real>::snapshot_begin_run() {
    Snapshots& s = snap_;
    if (!s.pending.empty()) {  // (a run that failed while enqueueing left captures of steps that were never committed)
        WV_HIP(hipStreamSynchronize(s.copy_stream));
        s.pending.clear();
    }
    if (s.next < steps_done) s.next = wv::snapshot_next_step(s.plan.first_step, s.plan.period, steps_done);
    s.batch_end = s.next;
    if (s.next == steps_done) return snapshot_capture(steps_done);
    return WV_OK;
}

// wv_rollback to a checkpoint taken at `to_step`: the snapshots of later steps are forgotten, the re-run takes them again.
template <typename Real>
void Engine<Real>::snapshot_rollback(uint64_t to_step) {
    Snapshots& s = snap_;
    uint64_t keep_taken, next;
    if (ckpt_.snap_generation == s.generation) {
        keep_taken = std::min(ckpt_.snap_taken, s.taken);
        next = ckpt_.snap_next;
    } else {
        // the plan was set after the checkpoint, at a step >= to_step: only a snapshot of to_step itself stays
        keep_taken = (s.taken > 0 && s.first_taken_step == to_step) ? 1 : 0;
        next = wv::snapshot_next_step(s.plan.first_step, s.plan.period, keep_taken ? to_step + 1 : s.set_at);
    }
    while (s.taken > keep_taken) {
        if (!s.held.empty()) s.held.pop_back();
        --s.taken;
    }
    s.next = next;
}

template <typename Real>
int Engine<Real>::snapshot_count(uint64_t* taken, uint64_t* first_held) {
    if (!snap_.active) return fail(WV_E_STATE, "wv_snapshot_count: no snapshot plan is set");
    if (taken) *taken = snap_.taken;
    if (first_held) *first_held = snap_.taken - snap_.held.size();
    return WV_OK;
}

template <typename Real>
int Engine<Real>::fetch_snapshots(uint64_t first, uint64_t n, float* dst, uint64_t* steps) {
    if (!snap_.active) return fail(WV_E_STATE, "wv_fetch_snapshots: no snapshot plan is set");
    const uint64_t first_held = snap_.taken - snap_.held.size();
    if (first < first_held) return fail(WV_E_INVALID_ARGUMENT, "wv_fetch_snapshots: snapshot already dropped (wv_snapshot_plan::keep)");
    if (first > snap_.taken || n > snap_.taken - first) return fail(WV_E_INVALID_ARGUMENT, "wv_fetch_snapshots: snapshot not taken yet");
    if (n && !dst) return fail(WV_E_INVALID_ARGUMENT, "null argument");
    for (uint64_t j = 0; j < n; ++j) {
        const auto& h = snap_.held[(size_t)(first - first_held + j)];
        std::memcpy(dst + j * snap_.elems, h.second.data(), (size_t)snap_.elems * sizeof(float));
        if (steps) steps[j] = h.first;
    }
    return WV_OK;
}

}  // namespace wv

// capture_stage.h -- (host only, no HIP) the bookkeeping of a stage of captures, shared by the five plans that accumulate on the device:
// field spectra, energy decay maps (plain and banded), intensity maps, arrival-aligned energy maps and lateral maps (engine_staged.hip.h
// has their life cycle, engine_<plan>.hip.h what is each plan's own).  All capture a box into the next free slot of a device-only
// stage, keep a batch's captures staged until commit_batch has said how many of the batch's steps were good, and fold everything staged
// in one launch when the stage has no slot left.  What differs between them is the fold itself; which steps were staged, how many of
// them are committed, which plan step comes next and where the batch being planned ends is the same, and lives here.  The integer rules
// (free slots, fold due, captures per batch, good captures after a stop) are spectrum_plan.h's, unchanged; which steps are plan steps is
// snapshot_plan.h's.
#pragma once
#include <cstdint>
#include <vector>

#include "snapshot_plan.h"
#include "spectrum_plan.h"

namespace wv {

struct CaptureStage {
    uint64_t first_step = 0, period = 1;    // captures at first_step + j * period
    uint64_t next = kNoSnapshotStep;        // the next plan step not yet captured
    uint64_t batch_end = kNoSnapshotStep;   // the plan step at which the batch being planned ends at the latest
    std::vector<uint64_t> steps;            // the steps of the staged captures, slot by slot
    int committed = 0;                      // how many of them are of committed steps (all of them between batches)
    uint64_t folded = 0;                    // captures already folded into the sums
    uint64_t last_step = 0;                 // the step of the last committed capture

    // a plan set when the engine has completed `steps_done` steps
    void start(uint64_t first, uint64_t every, uint64_t steps_done) {
        *this = CaptureStage{};
        first_step = first, period = every;
        next = snapshot_next_step(first_step, period, steps_done);
        batch_end = next;
    }
    bool full() const { return (int)steps.size() >= kSpectrumStage; }
    int slot() const { return (int)steps.size(); }                        // the slot the next capture takes
    uint64_t captures() const { return folded + (uint64_t)committed; }    // captures of completed steps since the plan was set
    bool fold_due() const { return spectrum_fold_due(committed); }

    // the capture of `step` has been enqueued into slot()
    void staged(uint64_t step) {
        steps.push_back(step);
        next = snapshot_next_step(first_step, period, step + 1);
    }
    // Captures of steps that were never committed (a run that failed while enqueueing left them staged) are dropped and are due again.
    void drop_uncommitted() {
        if ((int)steps.size() > committed) {
            next = steps[(size_t)committed];
            steps.resize((size_t)committed);
        }
    }
    // Behind commit_batch: the batch's captures of steps that were completed stay, the others are dropped (and are due again).
    void commit(uint64_t last_good_step) {
        const int n = (int)steps.size() - committed;
        const int good = spectrum_good_captures(steps.data() + committed, n, last_good_step);
        if (good < n) {
            next = steps[(size_t)(committed + good)];
            steps.resize((size_t)(committed + good));
        }
        committed += good;
        if (committed > 0) last_step = steps.back();
    }
    // Where the batch being planned ends at the latest: on the last capture the stage has a slot for (one capture per batch under
    // graph replay: a replayed graph covers the whole batch).  The fold, when due, has run.
    void plan_batch_end(bool graph) {
        int room = spectrum_batch_captures(committed, graph);
        uint64_t end = next;
        for (; room > 1 && end != kNoSnapshotStep; --room) end = snapshot_next_step(first_step, period, end + 1);
        batch_end = end == kNoSnapshotStep ? next : end;
    }
    // On entering wv_run at `steps_done`: plan steps that wv_step / wv_swap passed are passed.  True when a capture of the step the
    // engine stands at is due now.
    bool begin_run(uint64_t steps_done) {
        drop_uncommitted();
        if (next < steps_done) next = snapshot_next_step(first_step, period, steps_done);
        batch_end = next;
        return next == steps_done;
    }
    // the fold of everything committed has been enqueued: the stage is filled from slot 0 again
    void all_folded() {
        folded += (uint64_t)committed;
        committed = 0;
        steps.clear();
    }
    // wv_rollback: what is staged is of abandoned steps; count and position are the checkpoint's
    void rollback(uint64_t captures, uint64_t last, uint64_t next_step) {
        steps.clear();
        committed = 0;
        folded = captures;
        last_step = last;
        next = next_step;
        batch_end = next;
    }
};

}  // namespace wv

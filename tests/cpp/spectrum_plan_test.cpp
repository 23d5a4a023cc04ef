// spectrum_plan_test.cpp -- the stage planning of wayverb_amd/csrc/spectrum_plan.h on the CPU (tests/test_spectrum_plan.py builds and
// runs this).  Every expectation below is derived by hand from the contract in include/wayverb_amd.h and DESIGN.md 4.9, none recorded
// from the code.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "snapshot_plan.h"
#include "spectrum_plan.h"

static int g_failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++g_failures;                                                   \
        }                                                                   \
    } while (0)

using namespace wv;

// A stand-in for wv_run's loop with a spectrum plan: before each batch the fold when it is due, then a batch that ends on the last
// capture the stage has a slot for (never longer than `ring` steps); every capture goes into the stage.  Returns the number of folds
// (without the one a fetch adds) and checks that the stage never overflows and that no fold is launched on a stage with a free slot.
static int drive(uint64_t period, uint64_t run_steps, uint64_t ring, bool graph, uint64_t* captures_out) {
    int staged = 0, folds = 0;
    uint64_t captures = 0, done = 0, next = snapshot_next_step(0, period, 0);
    if (next == done) {  // the capture of step 0 at the start of the run
        ++staged, ++captures;
        next = snapshot_next_step(0, period, done + 1);
    }
    while (done < run_steps) {
        if (spectrum_fold_due(staged)) {
            CHECK(staged == kSpectrumStage);
            staged = 0;
            ++folds;
        }
        int room = spectrum_batch_captures(staged, graph);
        CHECK(room >= 1 && room <= kSpectrumStage - staged);
        uint64_t end = next;
        for (; room > 1; --room) end = snapshot_next_step(0, period, end + 1);
        const uint64_t want = ring < run_steps - done ? ring : run_steps - done;
        const uint64_t batch = snapshot_batch_limit(want, done, end);
        CHECK(batch >= 1);
        for (uint64_t s = done + 1; s <= done + batch; ++s)
            if (s == next) {
                ++staged, ++captures;
                CHECK(staged <= kSpectrumStage);
                next = snapshot_next_step(0, period, s + 1);
            }
        done += batch;
    }
    *captures_out = captures;
    return folds;
}

int main() {
    // ---- free slots -> captures of the next batch
    CHECK(kSpectrumStage == 16 && kSpectrumMaxFreqs == 64);
    CHECK(spectrum_free_slots(0) == 16 && spectrum_free_slots(1) == 15 && spectrum_free_slots(15) == 1 && spectrum_free_slots(16) == 0);
    CHECK(spectrum_free_slots(17) == 0 && spectrum_free_slots(-1) == 16);
    CHECK(spectrum_batch_captures(0, false) == 16 && spectrum_batch_captures(5, false) == 11 && spectrum_batch_captures(15, false) == 1);
    CHECK(spectrum_batch_captures(16, false) == 0);
    CHECK(spectrum_batch_captures(0, true) == 1 && spectrum_batch_captures(15, true) == 1 && spectrum_batch_captures(16, true) == 0);
    // ---- when a fold is due: only when the next batch could stage nothing
    CHECK(!spectrum_fold_due(0) && !spectrum_fold_due(1) && !spectrum_fold_due(15) && spectrum_fold_due(16));
    // ---- whole runs: period 1, 33 captures (steps 0 .. 32): the stage fills at 16 and at 32 -> two folds, the 33rd capture staged
    uint64_t captures = 0;
    CHECK(drive(1, 32, 64, false, &captures) == 2 && captures == 33);
    CHECK(drive(1, 15, 64, false, &captures) == 0 && captures == 16);   // exactly one stage: nothing folded before the fetch
    CHECK(drive(1, 16, 64, false, &captures) == 1 && captures == 17);
    CHECK(drive(1, 0, 64, false, &captures) == 0 && captures == 1);
    CHECK(drive(3, 480, 64, false, &captures) == 10 && captures == 161);  // 161 = 10 * 16 + 1
    CHECK(drive(3, 480, 7, false, &captures) == 10 && captures == 161);   // short batches change nothing
    CHECK(drive(16, 64, 64, true, &captures) == 0 && captures == 5);      // graph replay: one capture per batch
    CHECK(drive(1, 40, 64, true, &captures) == 2 && captures == 41);
    for (uint64_t period = 1; period <= 9; ++period)
        for (uint64_t steps = 0; steps <= 70; steps += 7) {
            const int folds = drive(period, steps, 64, false, &captures);
            CHECK(captures == steps / period + 1);
            // one per full stage that a further batch follows: a run that goes on behind its last capture (steps % period != 0) has
            // folded a stage that capture filled, a run that ends on it has not
            CHECK((uint64_t)folds == (steps % period != 0 ? captures / 16 : (captures - 1) / 16));
        }
    // ---- the good captures after a stop at step f
    {
        const uint64_t steps[] = {4, 8, 12, 16, 20};
        CHECK(spectrum_good_captures(steps, 5, 3) == 0);
        CHECK(spectrum_good_captures(steps, 5, 4) == 1);
        CHECK(spectrum_good_captures(steps, 5, 12) == 3);   // a capture of the very step the run stopped at stays
        CHECK(spectrum_good_captures(steps, 5, 13) == 3 && spectrum_good_captures(steps, 5, 15) == 3);
        CHECK(spectrum_good_captures(steps, 5, 20) == 5 && spectrum_good_captures(steps, 5, ~0ull) == 5);
        CHECK(spectrum_good_captures(steps, 0, 100) == 0 && spectrum_good_captures(nullptr, 0, 100) == 0);
    }
    // ---- the twiddle table [T][K][2]
    CHECK(spectrum_table_entries(1) == 32 && spectrum_table_bytes(1) == 256);
    CHECK(spectrum_table_entries(64) == 2048 && spectrum_table_bytes(64) == 16384);
    CHECK(spectrum_table_index(0, 0, 5) == 0 && spectrum_table_index(0, 4, 5) == 8 && spectrum_table_index(1, 0, 5) == 10);
    CHECK(spectrum_table_index(15, 63, 64) + 2 == spectrum_table_entries(64));
    // ---- B and byte counts, 64-bit and overflow-safe
    CHECK(spectrum_nodes(10, 9, 7) == 630 && spectrum_nodes(1, 1, 1) == 1);
    CHECK(spectrum_nodes(0, 9, 7) == 0 && spectrum_nodes(10, -1, 7) == 0 && spectrum_nodes(10, 9, 0) == 0);
    CHECK(spectrum_nodes(128, 128, 128) == 2097152ull);                       // 512^3 decimated by 4
    CHECK(spectrum_nodes(2147483647, 2147483647, 2) == 9223372028264841218ull);  // (2^31 - 1)^2 * 2: past 32 and 63 bits, inside 64
    CHECK(spectrum_nodes(2147483647, 2147483647, 5) == kSpectrumNoSize);      // past 64 bits
    CHECK(spectrum_stage_bytes(2097152ull) == 134217728ull);                  // 64 B per node: 128 MiB
    CHECK(spectrum_sum_bytes(2097152ull, 64) == 2147483648ull);               // 16 K B per node: 2 GiB
    CHECK(spectrum_sum_bytes(2097152ull, 16) == 536870912ull);
    CHECK(spectrum_sum_bytes(630, 5) == 50400 && spectrum_stage_bytes(630) == 40320);
    CHECK(spectrum_stage_bytes(1ull << 58) == kSpectrumNoSize && spectrum_stage_bytes((1ull << 58) - 1) == ((1ull << 58) - 1) * 64);
    CHECK(spectrum_sum_bytes(1ull << 54, 64) == kSpectrumNoSize && spectrum_sum_bytes(kSpectrumNoSize, 1) == kSpectrumNoSize);
    CHECK(spectrum_mul(0, kSpectrumNoSize - 1) == 0 && spectrum_mul(3, 5) == 15);
    CHECK(spectrum_mul(1ull << 32, 1ull << 31) == 1ull << 63 && spectrum_mul(1ull << 32, 1ull << 32) == kSpectrumNoSize);
    // ---- the bound: B (4 t + 32 K) bytes per fold; 36 B per node and capture at t = K = 16, 516 B when every capture is folded alone
    CHECK(spectrum_fold_traffic(1, 16, 16) == 576 && 576 / 16 == 36);
    CHECK(spectrum_fold_traffic(1, 1, 16) == 516);
    CHECK(spectrum_fold_traffic(2097152ull, 16, 16) / 16 == 75497472ull);     // 75 MB per capture ...
    CHECK(spectrum_fold_traffic(2097152ull, 1, 16) == 1082130432ull);         // ... against 1.08 GB
    if (g_failures) {
        std::printf("%d failures\n", g_failures);
        return 1;
    }
    std::printf("SPECTRUM PLAN OK\n");
    return 0;
}

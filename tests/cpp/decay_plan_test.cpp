// decay_plan_test.cpp -- wayverb_amd/csrc/decay_plan.h and the shared stage bookkeeping of capture_stage.h on the CPU
// (tests/test_decay_plan.py builds and runs this).  Every expectation below is derived by hand from the contract in
// include/wayverb_amd.h and DESIGN.md 4.10, none recorded from the code.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "capture_stage.h"
#include "decay_plan.h"

static int g_failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++g_failures;                                                   \
        }                                                                   \
    } while (0)

using namespace wv;

static void bins_of_captures() {
    // W = 1: every capture a bin of its own, until the last bin takes the rest
    for (uint64_t j = 0; j < 8; ++j) CHECK(decay_bin(j, 1, 100) == j);
    CHECK(decay_bin(99, 1, 100) == 99 && decay_bin(100, 1, 100) == 99 && decay_bin(1000000, 1, 100) == 99);
    // W = 5: 0..4 -> 0, 5..9 -> 1, 10..14 -> 2
    CHECK(decay_bin(0, 5, 10) == 0 && decay_bin(4, 5, 10) == 0 && decay_bin(5, 5, 10) == 1 && decay_bin(9, 5, 10) == 1 && decay_bin(14, 5, 10) == 2);
    // W = 16: a whole stage per bin; W = 17: the edge moves one slot per stage
    CHECK(decay_bin(15, 16, 4) == 0 && decay_bin(16, 16, 4) == 1 && decay_bin(31, 16, 4) == 1 && decay_bin(32, 16, 4) == 2);
    CHECK(decay_bin(16, 17, 4) == 0 && decay_bin(17, 17, 4) == 1 && decay_bin(33, 17, 4) == 1 && decay_bin(34, 17, 4) == 2);
    // the open-ended last bin: n_bins * W captures fill the bins, every later one goes to the last
    CHECK(decay_bin(49, 5, 10) == 9 && decay_bin(50, 5, 10) == 9 && decay_bin(51, 5, 10) == 9 && decay_bin(~0ull, 5, 10) == 9);
    CHECK(decay_bin(0, 7, 1) == 0 && decay_bin(6, 7, 1) == 0 && decay_bin(7, 7, 1) == 0 && decay_bin(12345, 7, 1) == 0);
    CHECK(decay_bin((1ull << 40) + 3, 1u << 20, 4096) == 4095);               // 2^20 bins' worth, past the last
    CHECK(decay_bin((1ull << 31) - 1, 1u << 20, 4096) == 2047);
    // bins never decrease with j and never leave 0 .. n_bins - 1
    uint32_t before = 0;
    for (uint64_t j = 0; j < 300; ++j) {
        const uint32_t b = decay_bin(j, 17, 9);
        CHECK(b >= before && b < 9);
        before = b;
    }
    // (what the engine refuses maps to bin 0, never out of bounds)
    CHECK(decay_bin(5, 0, 10) == 0 && decay_bin(5, 3, 0) == 0);
}

static void sizes_and_overflow() {
    CHECK(kDecayStage == 16 && kDecayMaxBins == 4096);
    CHECK(decay_nodes(24, 20, 28) == 13440 && decay_nodes(1, 1, 1) == 1 && decay_nodes(0, 5, 5) == 0 && decay_nodes(5, -1, 5) == 0);
    CHECK(decay_bins_bytes(630, 1) == 5040 && decay_bins_bytes(630, 4096) == 630ull * 4096 * 8);
    CHECK(decay_stage_bytes(630) == 630ull * 64 && decay_stage_bytes(0) == 0);
    CHECK(decay_table_bytes() == 64);
    // 512^3 decimated by 4, 300 bins: 128^3 * 2400 bytes
    CHECK(decay_bins_bytes(decay_nodes(128, 128, 128), 300) == 5033164800ull);
    // products that leave 64 bits say so, and the mark goes through every later product
    CHECK(decay_mul(1ull << 32, 1ull << 32) == kDecayNoSize);
    CHECK(decay_mul(1ull << 32, (1ull << 32) - 1) == 0xffffffff00000000ull);
    CHECK(decay_mul(0, kDecayNoSize - 1) == 0 && decay_mul(kDecayNoSize, 0) == kDecayNoSize && decay_mul(3, kDecayNoSize) == kDecayNoSize);
    CHECK(decay_nodes(1ll << 31, 1ll << 31, 4) == kDecayNoSize);
    CHECK(decay_nodes(1ll << 30, 1ll << 30, 8) != kDecayNoSize);
    CHECK(decay_bins_bytes(1ull << 50, 4096) == kDecayNoSize);                // 2^50 * 2^15
    CHECK(decay_bins_bytes(1ull << 48, 4096) == 1ull << 63);
    CHECK(decay_stage_bytes(1ull << 58) == kDecayNoSize && decay_stage_bytes(kDecayNoSize) == kDecayNoSize);
    CHECK(decay_bins_bytes(kDecayNoSize, 1) == kDecayNoSize);
}

static void traffic_model() {
    // r: distinct bins among t consecutive captures
    CHECK(decay_fold_bins(0, 16, 1, 4096) == 16);      // W = 1: r = t
    CHECK(decay_fold_bins(0, 16, 16, 100) == 1 && decay_fold_bins(16, 16, 16, 100) == 1);
    CHECK(decay_fold_bins(0, 16, 40, 100) == 1 && decay_fold_bins(32, 16, 40, 100) == 2);   // captures 32..47: bins 0 and 1
    CHECK(decay_fold_bins(0, 16, 5, 100) == 4);        // 0..15 -> bins 0, 1, 2, 3
    CHECK(decay_fold_bins(16, 16, 5, 100) == 4);       // 16..31 -> bins 3, 4, 5, 6
    CHECK(decay_fold_bins(0, 16, 17, 100) == 1 && decay_fold_bins(16, 16, 17, 100) == 2);
    CHECK(decay_fold_bins(0, 16, 1, 4) == 4);          // the open-ended last bin takes captures 3..15
    CHECK(decay_fold_bins(16, 16, 1, 4) == 1);
    CHECK(decay_fold_bins(7, 1, 3, 10) == 1 && decay_fold_bins(7, 0, 3, 10) == 0);
    // B * (4 t + 16 r)
    CHECK(decay_fold_traffic(1000, 16, 1) == 80000);
    CHECK(decay_fold_traffic(1000, 16, 16) == 320000);
    CHECK(decay_fold_traffic(262144, 16, 1) == 20971520ull);   // one 512^2 plane, W >= 16: 20 MiB per 16 captures
    CHECK(decay_fold_traffic(630, 5, 2) == 630ull * 52);
    CHECK(decay_fold_traffic(kDecayNoSize, 16, 1) == kDecayNoSize && decay_fold_traffic(1ull << 60, 16, 16) == kDecayNoSize);
}

// The stage bookkeeping both accumulating plans share: a plan of period 3 from step 0 on a ring of 8 steps per batch.
static void stage_bookkeeping() {
    CaptureStage st;
    st.start(0, 3, 0);
    CHECK(st.next == 0 && st.batch_end == 0 && st.captures() == 0 && st.slot() == 0 && !st.full() && !st.fold_due());
    CHECK(st.begin_run(0));            // a capture of step 0 is due at the start of the run
    st.staged(0);
    st.commit(0);
    CHECK(st.committed == 1 && st.next == 3 && st.last_step == 0 && st.captures() == 1);
    st.plan_batch_end(false);          // 15 free slots: 3, 6, ..., 45
    CHECK(st.batch_end == 45);
    st.plan_batch_end(true);           // graph replay: one capture per batch
    CHECK(st.batch_end == 3);
    // a batch stages 3, 6, 9 and stops on a flag at step 7: 3 and 6 stay, 9 is due again
    st.staged(3), st.staged(6), st.staged(9);
    CHECK(st.slot() == 4 && st.next == 12);
    st.commit(7);
    CHECK(st.committed == 3 && st.slot() == 3 && st.next == 9 && st.last_step == 6 && st.captures() == 3);
    // a run that failed while enqueueing left a capture staged: dropped, due again
    st.staged(9);
    st.drop_uncommitted();
    CHECK(st.slot() == 3 && st.next == 9);
    // wv_step took the engine to step 11: 9 is passed, 12 comes next
    CHECK(!st.begin_run(11));
    CHECK(st.next == 12 && st.batch_end == 12);
    // fill the stage: 13 more captures
    for (uint64_t s = 12; st.slot() < kSpectrumStage; s += 3) st.staged(s);
    CHECK(st.full());
    st.commit(1000);
    CHECK(st.committed == 16 && st.fold_due() && st.last_step == 12 + 12 * 3);
    st.all_folded();
    CHECK(st.folded == 16 && st.committed == 0 && st.slot() == 0 && st.captures() == 16 && !st.fold_due());
    // the first staged capture after a fold is capture number `folded`
    CHECK(decay_bin(st.folded + 0, 5, 100) == 3);
    st.rollback(3, 6, 9);
    CHECK(st.folded == 3 && st.last_step == 6 && st.next == 9 && st.batch_end == 9 && st.slot() == 0 && st.captures() == 3);
    // a plan set at step 10 with first_step 4, period 4: 12 is the first plan step
    st.start(4, 4, 10);
    CHECK(st.next == 12 && st.folded == 0 && st.captures() == 0);
}

int main() {
    bins_of_captures();
    sizes_and_overflow();
    traffic_model();
    stage_bookkeeping();
    if (g_failures) {
        std::printf("%d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("DECAY PLAN OK\n");
    return 0;
}

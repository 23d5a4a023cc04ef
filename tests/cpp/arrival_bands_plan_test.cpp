// arrival_bands_plan_test.cpp -- wayverb_amd/csrc/arrival_bands_plan.h on the CPU (tests/test_arrival_bands_plan.py builds and runs
// this).  Every expectation below is derived by hand from the contract in include/wayverb_amd.h and DESIGN.md 4.17, none recorded from
// the code.
#include <cstdio>

#include "arrival_bands_plan.h"

static int g_failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++g_failures;                                                   \
        }                                                                   \
    } while (0)

using namespace wv;

// edges (0, 1, 5, 16, 17), a tail of 4 bins of 3 captures from rel 19: bins 5 .. 8 begin at 19, 22, 25, 28; bin 8 is open-ended
static ArrivalBandsTable five_with_tail() {
    ArrivalBandsTable p = {};
    const uint32_t e[5] = {0, 1, 5, 16, 17};
    for (int k = 0; k < 5; ++k) p.edges[k] = e[k];
    for (int k = 5; k < 16; ++k) p.edges[k] = 0xDEADBEEFu;   // (not looked at)
    p.n_edges = 5, p.n_tail = 4, p.tail_first = 19, p.tail_captures = 3;
    return p;
}

static void validity() {
    const uint32_t e[16] = {0, 1, 5, 16, 17};
    CHECK(arrival_bands_tail_count_valid(5, 0) && arrival_bands_tail_count_valid(5, 4091) && !arrival_bands_tail_count_valid(5, 4092));
    CHECK(arrival_bands_tail_count_valid(16, 4080) && !arrival_bands_tail_count_valid(16, 4081) && arrival_bands_tail_count_valid(1, 4095));
    CHECK(!arrival_bands_tail_count_valid(1, 0xFFFFFFFFu));
    CHECK(arrival_bands_tail_first_valid(e, 5, 4, 18) && !arrival_bands_tail_first_valid(e, 5, 4, 17) && !arrival_bands_tail_first_valid(e, 5, 4, 0));
    CHECK(arrival_bands_tail_first_valid(e, 5, 0, 0));       // no tail: not looked at
    CHECK(arrival_bands_tail_first_valid(e, 1, 3, 1) && !arrival_bands_tail_first_valid(e, 1, 3, 0));
    CHECK(arrival_bands_tail_captures_valid(4, 1) && !arrival_bands_tail_captures_valid(4, 0) && arrival_bands_tail_captures_valid(0, 0));
    CHECK(kArrivalBandsStage == 16 && kArrivalBandsMaxBins == 4096 && kArrivalBandsMaxBands == 8);
    CHECK(sizeof(ArrivalBandsTable) == 28 * 4);
}

static void rel_and_bin() {
    // lag: d <= lag stays at 0, then counts from 1
    CHECK(arrival_bands_rel(0, 0) == 0 && arrival_bands_rel(7, 0) == 7);
    CHECK(arrival_bands_rel(0, 4) == 0 && arrival_bands_rel(4, 4) == 0 && arrival_bands_rel(5, 4) == 1 && arrival_bands_rel(3, 100) == 0);
    CHECK(arrival_bands_rel(0xFFFFFFFEu, 0xFFFFFFFFu) == 0 && arrival_bands_rel(0xFFFFFFFEu, 2) == 0xFFFFFFFCu);
    const ArrivalBandsTable p = five_with_tail();
    // every edge and one below it
    CHECK(arrival_bands_bin(0, p) == 0);
    CHECK(arrival_bands_bin(1, p) == 1 && arrival_bands_bin(4, p) == 1);
    CHECK(arrival_bands_bin(5, p) == 2 && arrival_bands_bin(15, p) == 2);
    CHECK(arrival_bands_bin(16, p) == 3);
    CHECK(arrival_bands_bin(17, p) == 4 && arrival_bands_bin(18, p) == 4);   // tail_first - 1: the last explicit bin, closed by the tail
    CHECK(arrival_bands_bin(19, p) == 5 && arrival_bands_bin(21, p) == 5);   // tail_first
    CHECK(arrival_bands_bin(22, p) == 6 && arrival_bands_bin(24, p) == 6 && arrival_bands_bin(25, p) == 7 && arrival_bands_bin(27, p) == 7);
    CHECK(arrival_bands_bin(28, p) == 8 && arrival_bands_bin(31, p) == 8);   // the tail's last boundary; open-ended behind it
    CHECK(arrival_bands_bin(0xFFFFFFFEu, p) == 8);
    ArrivalBandsTable q = p;
    q.n_tail = 0;                                                            // without a tail the last explicit bin is the open one
    CHECK(arrival_bands_bin(18, q) == 4 && arrival_bands_bin(19, q) == 4 && arrival_bands_bin(0xFFFFFFFEu, q) == 4);
    // the banded decay plan's shape: one edge, W = tail_first = 3, n = 4 bins: min(rel / 3, 3)
    ArrivalBandsTable d = {};
    d.n_edges = 1, d.n_tail = 3, d.tail_first = 3, d.tail_captures = 3;
    for (uint32_t rel = 0; rel < 20; ++rel) CHECK(arrival_bands_bin(rel, d) == (rel / 3 < 3 ? rel / 3 : 3));
    // the table a lane walks by: the first rel of every bin, NONE behind the last
    uint32_t first[10];
    for (uint32_t& v : first) v = 7;
    CHECK(arrival_bands_bin_first_entries(9) == 10);
    arrival_bands_bin_first(p, first);
    const uint32_t want[10] = {0, 1, 5, 16, 17, 19, 22, 25, 28, 0xFFFFFFFFu};
    for (int k = 0; k < 10; ++k) CHECK(first[k] == want[k]);
    uint32_t plain[6];
    arrival_bands_bin_first(q, plain);
    CHECK(plain[4] == 17 && plain[5] == 0xFFFFFFFFu);
    // a bin that begins beyond the last capture number is never reached: NONE, not a wrapped number
    ArrivalBandsTable w = {};
    w.n_edges = 1, w.n_tail = 4, w.tail_first = 1, w.tail_captures = 0x80000000u;
    CHECK(arrival_bands_first_rel(1, w) == 1 && arrival_bands_first_rel(2, w) == 0x80000001u && arrival_bands_first_rel(3, w) == 0xFFFFFFFFu &&
          arrival_bands_first_rel(4, w) == 0xFFFFFFFFu);
    CHECK(arrival_bands_bin(0x80000000u, w) == 1 && arrival_bands_bin(0x80000001u, w) == 2 && arrival_bands_bin(0xFFFFFFFEu, w) == 2);
    // walking by the table gives the definition's bin at every rel
    uint32_t k = 0;
    for (uint32_t rel = 0; rel < 64; ++rel) {
        if (rel >= first[k + 1]) ++k;
        CHECK(k == arrival_bands_bin(rel, p));
    }
}

static void sizes() {
    // B = 1000, K = 3, n_bins = 9, S = 4: doubles first -- pre 3 B, moment 3 B, bins 27 B -- then 3 B onsets, peak, peak_capture
    CHECK(arrival_bands_pre_offset() == 0 && arrival_bands_moment_offset(1000, 3) == 24000 && arrival_bands_bins_offset(1000, 3) == 48000);
    CHECK(arrival_bands_bins_bytes(1000, 3, 9) == 216000 && arrival_bands_onset_offset(1000, 3, 9) == 264000);
    CHECK(arrival_bands_peak_offset(1000, 3, 9) == 276000 && arrival_bands_peak_capture_offset(1000, 3, 9) == 280000);
    CHECK(arrival_bands_sums_bytes(1000, 3, 9) == 284000);
    CHECK(arrival_bands_state_bytes(1000, 3, 4) == 192000 && arrival_bands_stage_bytes(1000) == 64000);
    CHECK(arrival_bands_coef_bytes(3, 4) == 480 && arrival_bands_tables_bytes(3, 4, 9) == 520);
    // one band, one bin: the arrival plan's 28 + 8 bytes per node
    CHECK(arrival_bands_sums_bytes(7, 1, 1) == 7 * 36);
    // an odd B keeps every double aligned: all offsets of doubles are multiples of 8
    CHECK(arrival_bands_moment_offset(7, 3) % 8 == 0 && arrival_bands_bins_offset(7, 3) % 8 == 0 && arrival_bands_onset_offset(7, 3, 9) % 4 == 0);
    // overflow
    const uint64_t big = 1ull << 61;
    CHECK(arrival_bands_moment_offset(big, 8) == kDecayNoSize && arrival_bands_sums_bytes(big, 1, 1) == kDecayNoSize);
    CHECK(arrival_bands_bins_bytes(1ull << 48, 8, 4096) == kDecayNoSize && arrival_bands_state_bytes(big, 8, 4) == kDecayNoSize);
    CHECK(arrival_bands_peak_offset(kDecayNoSize, 1, 1) == kDecayNoSize);
    CHECK(arrival_bands_sums_bytes(1ull << 40, 8, 4096) == (1ull << 40) * (8ull * 8 * 4098 + 32 + 8));
}

static void traffic() {
    // 1024^2 nodes, K = 4, S = 4, t = 16, one bin touched, no map: 4 (64 + 128 + 20 + 16) + 8 = 920 bytes per node
    CHECK(arrival_bands_fold_traffic(1ull << 20, 4, 4, 16, 1, false) == (1ull << 20) * 920);
    // K = 1, S = 1, t = 16, two bins, a map: 64 + 32 + 20 + 32 + 4 + 8 = 160
    CHECK(arrival_bands_fold_traffic(1000, 1, 1, 16, 2, true) == 160000);
    CHECK(arrival_bands_fold_traffic(1ull << 62, 8, 4, 16, 1, false) == kDecayNoSize);
}

int main() {
    validity();
    rel_and_bin();
    sizes();
    traffic();
    if (g_failures) {
        std::printf("%d FAILED\n", g_failures);
        return 1;
    }
    std::printf("ARRIVAL BANDS PLAN OK\n");
    return 0;
}

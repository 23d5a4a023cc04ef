// arrival_plan_test.cpp -- wayverb_amd/csrc/arrival_plan.h on the CPU (tests/test_arrival_plan.py builds and runs this).  Every
// expectation below is derived by hand from the contract in include/wayverb_amd.h and DESIGN.md 4.13, none recorded from the code.
#include <cmath>
#include <cstdio>
#include <limits>

#include "arrival_plan.h"

static int g_failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++g_failures;                                                   \
        }                                                                   \
    } while (0)

using namespace wv;

static void edges() {
    const uint32_t one[16] = {0};
    CHECK(arrival_edges_valid(one, 1));
    CHECK(!arrival_edges_valid(one, 0));     // n_bins 1 .. 16
    CHECK(!arrival_edges_valid(one, 17));
    CHECK(!arrival_edges_valid(one, 2));     // 0, 0: not increasing
    CHECK(!arrival_edges_valid(nullptr, 1));
    const uint32_t clarity[16] = {0, 400, 640};   // 50 and 80 ms at 8 kHz; the entries behind n_bins are not looked at
    CHECK(arrival_edges_valid(clarity, 3));
    CHECK(!arrival_edges_valid(clarity, 4)); // the fourth entry is 0
    const uint32_t late_start[16] = {1, 2, 3};
    CHECK(!arrival_edges_valid(late_start, 3));   // edges[0] must be 0
    const uint32_t equal[16] = {0, 5, 5, 9};
    CHECK(!arrival_edges_valid(equal, 4));
    CHECK(arrival_edges_valid(equal, 2));
    const uint32_t falling[16] = {0, 5, 4};
    CHECK(!arrival_edges_valid(falling, 3));
    uint32_t full[16];
    for (uint32_t k = 0; k < 16; ++k) full[k] = k * k;   // 0, 1, 4, 9, ...
    CHECK(arrival_edges_valid(full, 16));
    full[15] = 0xFFFFFFFEu;                  // the largest rel there is
    CHECK(arrival_edges_valid(full, 16));
}

static void thresholds() {
    CHECK(arrival_threshold_valid(0.0f));
    CHECK(arrival_threshold_valid(-0.0f));
    CHECK(arrival_threshold_valid(1e-30f));
    CHECK(arrival_threshold_valid(std::numeric_limits<float>::max()));
    CHECK(arrival_threshold_valid(std::numeric_limits<float>::denorm_min()));
    CHECK(!arrival_threshold_valid(-1e-30f));
    CHECK(!arrival_threshold_valid(std::numeric_limits<float>::infinity()));
    CHECK(!arrival_threshold_valid(std::numeric_limits<float>::quiet_NaN()));
}

constexpr uint32_t kThree[3] = {0, 7, 9};

static void bins() {
    const uint32_t e[16] = {0, 1, 5, 16, 17};
    // rel equal to each edge opens that bin; one less is still the bin before
    CHECK(arrival_bin(0, e, 5) == 0);
    CHECK(arrival_bin(1, e, 5) == 1);
    CHECK(arrival_bin(4, e, 5) == 1);
    CHECK(arrival_bin(5, e, 5) == 2);
    CHECK(arrival_bin(15, e, 5) == 2);
    CHECK(arrival_bin(16, e, 5) == 3);
    CHECK(arrival_bin(17, e, 5) == 4);
    CHECK(arrival_bin(18, e, 5) == 4);
    CHECK(arrival_bin(0xFFFFFFFEu, e, 5) == 4);   // the last bin is open-ended: rel = 2^32 - 2, the largest there is
    // fewer bins of the same table: the entries behind n_bins are not looked at
    CHECK(arrival_bin(17, e, 3) == 2);
    CHECK(arrival_bin(0xFFFFFFFEu, e, 1) == 0);
    CHECK(arrival_bin(3, e, 0) == 0);
    // all 16, the last edge at the very top
    uint32_t full[16];
    for (uint32_t k = 0; k < 16; ++k) full[k] = 3 * k;
    for (uint32_t k = 0; k < 16; ++k) {
        CHECK(arrival_bin(3 * k, full, 16) == k);
        CHECK(arrival_bin(3 * k + 2, full, 16) == k);
        if (k) CHECK(arrival_bin(3 * k - 1, full, 16) == k - 1);
    }
    full[15] = 0xFFFFFFFEu;
    CHECK(arrival_bin(0xFFFFFFFDu, full, 16) == 14);
    CHECK(arrival_bin(0xFFFFFFFEu, full, 16) == 15);
    // constexpr: the device evaluates this very text
    static_assert(arrival_bin(7, kThree, 3) == 1 && arrival_bin(6, kThree, 3) == 0 && arrival_bin(9, kThree, 3) == 2, "");
    CHECK(kArrivalNone == 0xFFFFFFFFu && kArrivalMaxCaptures == 0xFFFFFFFFull && kArrivalMaxBins == 16 && kArrivalStage == 16);
}

static void sizes() {
    // B = 630, 3 bins: doubles first -- pre at 0, moment at 5040, bins at 10080 (15120 bytes), then onset at 25200, peak at 27720,
    // peak_capture at 30240; 32760 bytes = 630 * (28 + 24)
    CHECK(arrival_pre_offset() == 0);
    CHECK(arrival_moment_offset(630) == 5040);
    CHECK(arrival_bins_offset(630) == 10080);
    CHECK(arrival_bins_bytes(630, 3) == 15120);
    CHECK(arrival_onset_offset(630, 3) == 25200);
    CHECK(arrival_peak_offset(630, 3) == 27720);
    CHECK(arrival_peak_capture_offset(630, 3) == 30240);
    CHECK(arrival_state_bytes(630, 3) == 32760);
    // an odd B: every double part still starts on a multiple of 8, every 4-byte part on a multiple of 4
    CHECK(arrival_onset_offset(567, 16) % 8 == 0 && arrival_peak_offset(567, 16) % 4 == 0 && arrival_peak_capture_offset(567, 16) % 4 == 0);
    CHECK(arrival_state_bytes(1, 1) == 36 && arrival_state_bytes(1, 16) == 156 && arrival_state_bytes(0, 16) == 0);
    CHECK(arrival_stage_bytes(630) == 630 * 64 && arrival_map_bytes(630) == 2520);
    // past 64 bits: kDecayNoSize, never a wrapped number
    const uint64_t huge = 1ull << 60;
    CHECK(arrival_state_bytes(huge, 16) == kDecayNoSize);
    CHECK(arrival_state_bytes(huge, 1) == kDecayNoSize);       // 36 * 2^60
    CHECK(arrival_onset_offset(huge, 1) == kDecayNoSize);      // 24 * 2^60
    CHECK(arrival_bins_bytes(huge, 1) == 8 * huge);
    CHECK(arrival_stage_bytes(huge) == kDecayNoSize);
    CHECK(arrival_map_bytes(1ull << 62) == kDecayNoSize);
    CHECK(arrival_state_bytes(kDecayNoSize, 1) == kDecayNoSize);
    // the sum of two sizes that each fit: (2^63 - 1) * 2 + ... -> no size
    CHECK(arrival_add(1ull << 63, 1ull << 63) == kDecayNoSize);
    CHECK(arrival_add(kDecayNoSize - 1, 1) == kDecayNoSize);    // (the all-ones value itself means "no size")
    CHECK(arrival_add(kDecayNoSize - 2, 1) == kDecayNoSize - 1);
    CHECK(arrival_add(5, 7) == 12);
    // 2^59 nodes, one bin: 36 * 2^59 > 2^64 -> no size; 2^58: 36 * 2^58 = 9 * 2^60 fits
    CHECK(arrival_state_bytes(1ull << 59, 1) == kDecayNoSize);
    CHECK(arrival_state_bytes(1ull << 58, 1) == 9 * (1ull << 60));
    // the traffic model: t floats, 28 bytes of state, r bins read and written, 4 more with a map
    CHECK(arrival_fold_traffic(1000, 16, 1, false) == 1000 * (64 + 28 + 16));
    CHECK(arrival_fold_traffic(1000, 16, 2, true) == 1000 * (64 + 28 + 32 + 4));
    CHECK(arrival_fold_traffic(1, 1, 1, false) == 48);
}

int main() {
    edges();
    thresholds();
    bins();
    sizes();
    if (g_failures) {
        std::printf("%d FAILURES\n", g_failures);
        return 1;
    }
    std::printf("ARRIVAL PLAN OK\n");
    return 0;
}

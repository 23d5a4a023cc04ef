// waterfall_plan_test.cpp -- (CPU, stand-alone) wayverb_amd/csrc/waterfall_plan.h against hand-derived cases: the cap on sums per node,
// the bin of a capture (decay_plan.h's rule, reused), sizes and places of the one block with their overflow answers, the tables' sizes,
// the distinct bins of a fold and the traffic model.  tests/test_waterfall_plan.py builds and runs it.
#include "waterfall_plan.h"

#include <cstdio>

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

int main() {
    using namespace wv;
    // limits: the spectrum plan's K, the decay plan's bins, 4096 sums per node
    CHECK(kWaterfallStage == 16 && kWaterfallStage == kSpectrumStage && kWaterfallStage == kDecayStage);
    CHECK(kWaterfallMaxFreqs == 64 && kWaterfallMaxBins == 4096 && kWaterfallMaxSums == 4096);
    CHECK(waterfall_sums_valid(1, 1) && waterfall_sums_valid(1, 4096) && waterfall_sums_valid(64, 64) && waterfall_sums_valid(16, 256));
    CHECK(!waterfall_sums_valid(65, 64) && !waterfall_sums_valid(64, 65) && !waterfall_sums_valid(2, 2049) && !waterfall_sums_valid(64, 4096));
    CHECK(!waterfall_sums_valid(0xffffffffu, 0xffffffffu));                       // (the product is taken in 64 bits)
    CHECK(waterfall_sums_valid(4096, 1));                                         // (each factor's own range is the setter's check, ahead of this one)

    // the bin of a capture IS decay_bin: W per bin, the last open-ended
    for (uint64_t j = 0; j < 40; ++j)
        for (uint32_t w = 1; w < 6; ++w)
            for (uint32_t n = 1; n < 8; ++n) CHECK(waterfall_bin(j, w, n) == decay_bin(j, w, n));
    CHECK(waterfall_bin(0, 4, 3) == 0 && waterfall_bin(3, 4, 3) == 0 && waterfall_bin(4, 4, 3) == 1 && waterfall_bin(11, 4, 3) == 2);
    CHECK(waterfall_bin(12, 4, 3) == 2 && waterfall_bin(1000000, 4, 3) == 2 && waterfall_bin(~0ull, 1, 4096) == 4095);
    CHECK(waterfall_bin(7, 1, 1) == 0 && waterfall_bin(5, 0, 3) == 0 && waterfall_bin(5, 3, 0) == 0);

    // sizes: stage float[16][B], sums double[n_bins][K][2][B], the two tables
    CHECK(waterfall_nodes(10, 9, 7) == 630 && waterfall_nodes(0, 9, 7) == 0 && waterfall_nodes(1, 1, 1) == 1);
    CHECK(waterfall_stage_bytes(630) == 630ull * 16 * 4);
    CHECK(waterfall_sum_bytes(630, 7, 5) == 630ull * 7 * 5 * 16);
    CHECK(waterfall_sum_bytes(1, 64, 64) == 65536);                               // 64 KiB of sums per node at the cap
    CHECK(waterfall_sum_bytes(1, 1, 5) == spectrum_sum_bytes(1, 5));              // one bin: the spectrum plan's block
    CHECK(waterfall_fetch_bytes(567, 4, 9) == waterfall_sum_bytes(567, 4, 9));
    CHECK(waterfall_bin_table_bytes() == 64 && waterfall_bin_table_bytes() == decay_table_bytes());
    CHECK(waterfall_twiddle_table_bytes(5) == 16ull * 5 * 2 * 8 && waterfall_twiddle_table_bytes(64) == spectrum_table_bytes(64));
    CHECK(waterfall_stage_bytes(kWaterfallNoSize) == kWaterfallNoSize);
    CHECK(waterfall_sum_bytes(1ull << 60, 4096, 1) == kWaterfallNoSize);          // does not fit 64 bits: the engine answers "no room"
    CHECK(waterfall_sum_bytes((1ull << 63) / 65536, 64, 64) == (1ull << 63));

    // places: bin-major, then frequency, a re plane and an im plane each
    CHECK(waterfall_sum_offset(630, 0, 0, 5) == 0 && waterfall_sum_offset(630, 0, 1, 5) == 2 * 630);
    CHECK(waterfall_sum_offset(630, 1, 0, 5) == 10 * 630 && waterfall_sum_offset(630, 6, 4, 5) == (6 * 5 + 4) * 2 * 630ull);
    CHECK((waterfall_sum_offset(630, 6, 4, 5) + 2 * 630) * 8 == waterfall_sum_bytes(630, 7, 5));   // the last pair of planes ends the block
    CHECK(waterfall_sum_offset(567, 0, 3, 9) == spectrum_sum_bytes(567, 3) / 8);  // bin 0 lies as the spectrum plan's sums do

    // r': distinct bins among a fold's captures, and the model B * (4 t + 32 K r')
    CHECK(waterfall_fold_bins(0, 16, 16, 4) == 1 && waterfall_fold_bins(1, 16, 16, 4) == 2 && waterfall_fold_bins(0, 16, 1, 33) == 16);
    CHECK(waterfall_fold_bins(3, 16, 3, 7) == 6 && waterfall_fold_bins(0, 16, 8, 3) == 2 && waterfall_fold_bins(100, 16, 3, 4) == 1);
    CHECK(waterfall_fold_bins(5, 0, 3, 4) == 0 && waterfall_fold_bins(5, 1, 3, 4) == 1);
    CHECK(waterfall_fold_traffic(630, 16, 5, 1) == 630ull * (64 + 160));
    CHECK(waterfall_fold_traffic(630, 16, 5, 1) == spectrum_fold_traffic(630, 16, 5));            // one bin: the spectrum fold's bytes
    CHECK(waterfall_fold_traffic(262144, 16, 16, 2) == 262144ull * (64 + 1024));
    CHECK(waterfall_fold_traffic(kWaterfallNoSize, 16, 1, 1) == kWaterfallNoSize);

    if (failures == 0) std::printf("WATERFALL PLAN OK\n");
    return failures ? 1 : 0;
}

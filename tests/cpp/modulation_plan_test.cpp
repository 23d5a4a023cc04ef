// modulation_plan_test.cpp -- wayverb_amd/csrc/modulation_plan.h on the CPU (tests/test_modulation_plan.py builds and runs this).
// Every expectation below is derived by hand from the contract in include/wayverb_amd.h and DESIGN.md 4.16, none recorded from the
// code.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "modulation_plan.h"

static int g_failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++g_failures;                                                   \
        }                                                                   \
    } while (0)

using namespace wv;

static void limits() {
    CHECK(kModulationStage == 16 && kModulationStage == kDecayStage && kModulationMaxFreqs == 16);
    CHECK(kModulationMaxBands == 8 && kModulationMaxSections == 4);
    CHECK(modulation_valid(1, 1, 1) && modulation_valid(8, 4, 16) && modulation_valid(3, 4, 14));
    CHECK(!modulation_valid(0, 1, 1) && !modulation_valid(9, 1, 1) && !modulation_valid(1, 0, 1) && !modulation_valid(1, 5, 1));
    CHECK(!modulation_valid(1, 1, 0) && !modulation_valid(1, 1, 17) && !modulation_valid(0xffffffffu, 4, 16) && !modulation_valid(8, 4, 0xffffffffu));
    CHECK(modulation_frequency_valid(0.0) && modulation_frequency_valid(0.5) && modulation_frequency_valid(12.5 / 8000.0) && modulation_frequency_valid(-0.0));
    CHECK(!modulation_frequency_valid(-1e-300) && !modulation_frequency_valid(std::nextafter(0.5, 1.0)) && !modulation_frequency_valid(1.0));
    CHECK(!modulation_frequency_valid(std::numeric_limits<double>::quiet_NaN()) && !modulation_frequency_valid(std::numeric_limits<double>::infinity()));
    CHECK(!modulation_frequency_valid(-std::numeric_limits<double>::infinity()));
}

static void sizes_and_overflow() {
    CHECK(modulation_nodes(24, 20, 28) == 13440 && modulation_nodes(1, 1, 1) == 1 && modulation_nodes(0, 5, 5) == 0 && modulation_nodes(5, -1, 5) == 0);
    CHECK(modulation_band_planes(1) == 3 && modulation_band_planes(14) == 29 && modulation_band_planes(16) == 33);
    CHECK(modulation_stage_bytes(630) == 630ull * 64 && modulation_stage_bytes(0) == 0);
    // the issue's figure: 8 n_bands (1 + 2 n_freqs) bytes per node
    CHECK(modulation_sums_bytes(630, 1, 1) == 630ull * 24);
    CHECK(modulation_sums_bytes(630, 3, 14) == 630ull * 8 * 3 * 29);
    CHECK(modulation_sums_bytes(1, 8, 16) == 8ull * 8 * 33);
    CHECK(modulation_fetch_bytes(1024 * 1024, 7, 14) == 1048576ull * 8 * 7 * 29);
    // 16 n_sections n_bands bytes of filter state per node
    CHECK(modulation_state_bytes(630, 1, 1) == 630ull * 16 && modulation_state_bytes(630, 8, 4) == 630ull * 16 * 32);
    CHECK(modulation_coef_bytes(1, 1) == 40 && modulation_coef_bytes(8, 4) == 1280 && modulation_coef_bytes(3, 4) == 480);
    CHECK(modulation_table_entries(1) == 32 && modulation_table_entries(14) == 448 && modulation_table_bytes(16) == 16ull * 16 * 2 * 8);
    // products that leave 64 bits say so, and the mark goes through every later product
    const uint64_t huge = modulation_nodes(1ll << 31, 1ll << 31, 4);
    CHECK(huge == kModulationNoSize);
    CHECK(modulation_stage_bytes(huge) == kModulationNoSize && modulation_sums_bytes(huge, 1, 1) == kModulationNoSize && modulation_state_bytes(huge, 1, 1) == kModulationNoSize);
    CHECK(modulation_energy_offset(huge, 1, 1) == kModulationNoSize && modulation_sum_offset(huge, 0, 0, 1) == kModulationNoSize);
    CHECK(modulation_fold_traffic(huge, 1, 1, 1, 1) == kModulationNoSize);
    const uint64_t big = modulation_nodes(1ll << 30, 1ll << 30, 8);  // 2^63 nodes: a count that fits, bytes that do not
    CHECK(big == (1ull << 63) && modulation_stage_bytes(big) == kModulationNoSize && modulation_sums_bytes(big, 1, 1) == kModulationNoSize);
    CHECK(modulation_sums_bytes(1ull << 55, 8, 16) == kModulationNoSize);      // 2^55 * 2112
    CHECK(modulation_sums_bytes(1ull << 52, 8, 16) == (1ull << 52) * 2112);    // fits
    CHECK(modulation_state_bytes(1ull << 60, 1, 1) == kModulationNoSize && modulation_state_bytes(1ull << 59, 1, 1) == (1ull << 63));
}

static void places() {
    const uint64_t B = 630;
    // block 0, double[n_bands][1 + 2 M][B]: band k starts at k (1 + 2 M) B; E first, then Re, Im per frequency
    CHECK(modulation_energy_offset(B, 0, 14) == 0 && modulation_energy_offset(B, 1, 14) == 29 * B && modulation_energy_offset(B, 7, 16) == 7 * 33 * B);
    CHECK(modulation_sum_offset(B, 0, 0, 14) == B && modulation_sum_offset(B, 0, 1, 14) == 3 * B && modulation_sum_offset(B, 0, 13, 14) == 27 * B);
    CHECK(modulation_sum_offset(B, 2, 5, 14) == (2 * 29 + 11) * B);
    // the last Im plane of the last band ends the block
    for (uint32_t K = 1; K <= 8; ++K)
        for (uint32_t M = 1; M <= 16; ++M) {
            CHECK((modulation_sum_offset(B, K - 1, M - 1, M) + 2 * B) * 8 == modulation_sums_bytes(B, K, M));
            // planes never overlap: Re of m + 1 starts where Im of m ends, E of band k + 1 where Im of the last frequency ends
            for (uint32_t m = 0; m + 1 < M; ++m) CHECK(modulation_sum_offset(B, K - 1, m + 1, M) == modulation_sum_offset(B, K - 1, m, M) + 2 * B);
            CHECK(modulation_energy_offset(B, K, M) == modulation_sum_offset(B, K - 1, M - 1, M) + 2 * B);
            CHECK(modulation_sum_offset(B, K - 1, 0, M) == modulation_energy_offset(B, K - 1, M) + B);
        }
    // block 1, double[n_bands][S][2][B]
    CHECK(modulation_state_offset(B, 0, 0, 0, 4) == 0 && modulation_state_offset(B, 0, 0, 1, 4) == B && modulation_state_offset(B, 0, 1, 0, 4) == 2 * B);
    CHECK(modulation_state_offset(B, 1, 0, 0, 4) == 8 * B && modulation_state_offset(B, 2, 1, 1, 3) == (2 * 3 + 1) * 2 * B + B);
    for (uint32_t K = 1; K <= 8; ++K)
        for (uint32_t S = 1; S <= 4; ++S) CHECK((modulation_state_offset(B, K - 1, S - 1, 1, S) + B) * 8 == modulation_state_bytes(B, K, S));
    // the twiddle table double[T][M][2], the spectrum plan's index
    CHECK(modulation_table_index(0, 0, 14) == 0 && modulation_table_index(0, 13, 14) == 26 && modulation_table_index(1, 0, 14) == 28);
    CHECK(modulation_table_index(15, 15, 16) + 2 == modulation_table_entries(16) && modulation_table_index(15, 0, 1) + 2 == modulation_table_entries(1));
    for (uint32_t M = 1; M <= 16; ++M) CHECK((modulation_table_index(15, M - 1, M) + 2) * 8 == modulation_table_bytes(M));
}

static void traffic() {
    // B n_bands (4 t + 32 S + 16 + 32 M)
    CHECK(modulation_fold_traffic(1, 1, 1, 1, 1) == 4 + 32 + 16 + 32);
    CHECK(modulation_fold_traffic(1024 * 1024, 3, 4, 14, 16) == 1048576ull * 3 * (64 + 128 + 16 + 448));
    CHECK(modulation_fold_traffic(630, 8, 4, 16, 16) == 630ull * 8 * (64 + 128 + 16 + 512));
    CHECK(modulation_fold_traffic(0, 8, 4, 16, 16) == 0);
    // against the banded decay fold of the same plane with all captures in one bin: 32 M more bytes per node and band
    CHECK(modulation_fold_traffic(630, 3, 4, 14, 16) - decay_bands_fold_traffic(630, 3, 4, 16, 1) == 630ull * 3 * 32 * 14);
}

int main() {
    limits();
    sizes_and_overflow();
    places();
    traffic();
    if (g_failures) {
        std::printf("%d FAILED\n", g_failures);
        return 1;
    }
    std::printf("MODULATION PLAN OK\n");
    return 0;
}

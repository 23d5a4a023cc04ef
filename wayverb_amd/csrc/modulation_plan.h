// modulation_plan.h -- (host only, no HIP, nothing but the standard library) the integer logic of modulation maps (wv_set_modulation,
// include/wayverb_amd.h) that is the plan's own: what a plan is refused for, the sizes of everything that is allocated for it, where
// the energies, the Fourier sums and the filter states of a band lie inside the plan's two blocks, the twiddle table's size and index,
// and the traffic model of a fold.  The stage itself is spectrum_plan.h's, unchanged (capture_stage.h holds its bookkeeping); the band
// limits are decay_plan.h's; which steps are plan steps and whether a box lies inside the mesh is snapshot_plan.h's.
// tests/cpp/modulation_plan_test.cpp covers this file on the CPU.
#pragma once
#include <cstdint>
#include <limits>

#include "decay_plan.h"

namespace wv {

constexpr int kModulationStage = kDecayStage;       // T: captures the stage holds (engine_staged.hip.h asserts that all plans agree)
constexpr uint32_t kModulationMaxFreqs = 16;        // M at the most (IEC 60268-16 uses 14)
constexpr uint32_t kModulationMaxBands = kDecayMaxBands;
constexpr int kModulationMaxSections = kDecayMaxSections;
constexpr uint64_t kModulationNoSize = kDecayNoSize;  // "does not fit 64 bits"

// 1 .. 8 bands, 1 .. 4 sections, 1 .. 16 modulation frequencies
inline bool modulation_valid(uint32_t n_bands, uint32_t n_sections, uint32_t n_freqs) {
    return decay_bands_valid(n_bands, n_sections) && n_freqs >= 1 && n_freqs <= kModulationMaxFreqs;
}
// a frequency in cycles per step the plan takes: 0 .. 0.5 (a NaN fails both comparisons)
inline bool modulation_frequency_valid(double cycles_per_step) { return cycles_per_step >= 0.0 && cycles_per_step <= 0.5; }

// B: nodes taken by a box of nx * ny * nz nodes (0 for an empty box)
inline uint64_t modulation_nodes(int64_t nx, int64_t ny, int64_t nz) { return decay_nodes(nx, ny, nz); }

// planes of B doubles one band has in block 0: E, then Re and Im per frequency
inline uint64_t modulation_band_planes(uint32_t n_freqs) { return 1ull + 2ull * n_freqs; }

// bytes of the stage float[T][B], of block 0 double[n_bands][1 + 2 M][B], of block 1 double[n_bands][S][2][B], of the coefficient
// table double[n_bands][S][5], of one twiddle table double[T][M][2]
inline uint64_t modulation_stage_bytes(uint64_t nodes) { return decay_mul(nodes, (uint64_t)kModulationStage * sizeof(float)); }
inline uint64_t modulation_sums_bytes(uint64_t nodes, uint32_t n_bands, uint32_t n_freqs) {
    return decay_mul(nodes, (uint64_t)n_bands * modulation_band_planes(n_freqs) * sizeof(double));
}
inline uint64_t modulation_state_bytes(uint64_t nodes, uint32_t n_bands, uint32_t n_sections) { return decay_band_state_bytes(nodes, n_bands, n_sections); }
inline uint64_t modulation_coef_bytes(uint32_t n_bands, uint32_t n_sections) { return decay_band_coef_bytes(n_bands, n_sections); }
inline uint64_t modulation_table_entries(uint32_t n_freqs) { return (uint64_t)kModulationStage * n_freqs * 2; }
inline uint64_t modulation_table_bytes(uint32_t n_freqs) { return modulation_table_entries(n_freqs) * sizeof(double); }
// where the twiddle pair (cos, sin) of staged capture j and frequency m starts in a table
inline uint64_t modulation_table_index(uint32_t j, uint32_t m, uint32_t n_freqs) { return ((uint64_t)j * n_freqs + m) * 2; }

// offsets in DOUBLES inside block 0: the energy plane of band k, the Re plane of band k at frequency m (its Im plane follows it)
inline uint64_t modulation_energy_offset(uint64_t nodes, uint32_t band, uint32_t n_freqs) {
    return decay_mul(nodes, (uint64_t)band * modulation_band_planes(n_freqs));
}
inline uint64_t modulation_sum_offset(uint64_t nodes, uint32_t band, uint32_t m, uint32_t n_freqs) {
    return decay_mul(nodes, (uint64_t)band * modulation_band_planes(n_freqs) + 1 + 2ull * m);
}
// ... inside block 1: z1 (which = 0) or z2 (which = 1) of section s of band k
inline uint64_t modulation_state_offset(uint64_t nodes, uint32_t band, uint32_t s, uint32_t which, uint32_t n_sections) {
    return decay_mul(nodes, ((uint64_t)band * n_sections + s) * 2 + which);
}

// bytes that cross the link per fetch: n_bands * (1 + 2 M) doubles per node
inline uint64_t modulation_fetch_bytes(uint64_t nodes, uint32_t n_bands, uint32_t n_freqs) { return modulation_sums_bytes(nodes, n_bands, n_freqs); }

// bytes one fold of t staged captures moves: per band t floats read (the re-reads expected from L2), the state, E and the 2 M sums
// read and written
inline uint64_t modulation_fold_traffic(uint64_t nodes, uint32_t n_bands, uint32_t n_sections, uint32_t n_freqs, uint32_t t) {
    return decay_mul(decay_mul(nodes, n_bands), 4ull * t + 32ull * n_sections + 16ull + 32ull * n_freqs);
}

}  // namespace wv

// decay_plan.h -- (host only, no HIP, nothing but the standard library) the integer logic of energy decay maps (wv_set_decay,
// include/wayverb_amd.h) that is the plan's own: which bin a capture goes to, the sizes of everything that is allocated for a plan,
// and the traffic model of a fold.  The stage itself -- 16 slots, free slots, when a fold is due, captures per batch under graph
// replay, the good captures after a stop -- is spectrum_plan.h's, unchanged (capture_stage.h holds its bookkeeping for both plans);
// which steps are plan steps and whether a box lies inside the mesh is snapshot_plan.h's.
// tests/cpp/decay_plan_test.cpp covers this file on the CPU.
#pragma once
#include <cstdint>
#include <limits>

namespace wv {

constexpr int kDecayStage = 16;            // T: captures the stage holds (== kSpectrumStage: engine_staged.hip.h asserts it)
constexpr uint32_t kDecayMaxBins = 4096;   // n_bins at the most
constexpr uint64_t kDecayNoSize = std::numeric_limits<uint64_t>::max();  // "does not fit 64 bits"

// a * b, kDecayNoSize when the product leaves 64 bits (or an operand already has): spectrum_mul's rule
inline uint64_t decay_mul(uint64_t a, uint64_t b) {
    if (a == kDecayNoSize || b == kDecayNoSize) return kDecayNoSize;
    if (a != 0 && b > (kDecayNoSize - 1) / a) return kDecayNoSize;
    return a * b;
}

// The bin of capture j (captures are counted 0, 1, ... since the plan was set): W = bin_captures captures per bin, the last bin
// open-ended, so that the backward sums of the bins stay exact tail sums at every earlier edge.  (W = 0 or n_bins = 0: bin 0; the
// engine refuses both.)
inline uint32_t decay_bin(uint64_t j, uint32_t bin_captures, uint32_t n_bins) {
    if (bin_captures == 0 || n_bins == 0) return 0;
    const uint64_t b = j / bin_captures;
    return b >= n_bins ? n_bins - 1 : (uint32_t)b;
}

// B: nodes taken by a box of nx * ny * nz nodes (0 for an empty box)
inline uint64_t decay_nodes(int64_t nx, int64_t ny, int64_t nz) {
    if (nx < 1 || ny < 1 || nz < 1) return 0;
    return decay_mul(decay_mul((uint64_t)nx, (uint64_t)ny), (uint64_t)nz);
}

// bytes of the bins double[n_bins][B], of the stage float[T][B], of one per-fold bin table int32[T]
inline uint64_t decay_bins_bytes(uint64_t nodes, uint32_t n_bins) { return decay_mul(nodes, (uint64_t)n_bins * sizeof(double)); }
inline uint64_t decay_stage_bytes(uint64_t nodes) { return decay_mul(nodes, (uint64_t)kDecayStage * sizeof(float)); }
inline uint64_t decay_table_bytes() { return (uint64_t)kDecayStage * sizeof(int32_t); }

// r: distinct bins among the t captures first, first + 1, ..., first + t - 1 (bins never decrease: the last less the first, plus one)
inline uint32_t decay_fold_bins(uint64_t first, uint32_t t, uint32_t bin_captures, uint32_t n_bins) {
    if (t == 0) return 0;
    return decay_bin(first + t - 1, bin_captures, n_bins) - decay_bin(first, bin_captures, n_bins) + 1;
}

// bytes one fold of t staged captures moves: t floats read, r bins read and written, per node
inline uint64_t decay_fold_traffic(uint64_t nodes, uint32_t t, uint32_t r) { return decay_mul(nodes, 4ull * t + 16ull * r); }

// ---- band-limited decay maps (wv_set_decay_bands): n_bands cascades of n_sections biquad sections ahead of the square
constexpr uint32_t kDecayMaxBands = 8;     // n_bands at the most
constexpr int kDecayMaxSections = 4;       // n_sections at the most (the fold kernel has one instance per count)
constexpr uint32_t kBiquadDoubles = 5;     // b0 b1 b2 a1 a2 (wv_biquad)

inline bool decay_bands_valid(uint32_t n_bands, uint32_t n_sections) {
    return n_bands >= 1 && n_bands <= kDecayMaxBands && n_sections >= 1 && n_sections <= (uint32_t)kDecayMaxSections;
}
// bytes of the bins double[n_bands][n_bins][B], of the filter state double[n_bands][n_sections][2][B], of the coefficient table
inline uint64_t decay_band_bins_bytes(uint64_t nodes, uint32_t n_bins, uint32_t n_bands) { return decay_mul(decay_bins_bytes(nodes, n_bins), n_bands); }
inline uint64_t decay_band_state_bytes(uint64_t nodes, uint32_t n_bands, uint32_t n_sections) {
    return decay_mul(nodes, (uint64_t)n_bands * n_sections * 2 * sizeof(double));
}
inline uint64_t decay_band_coef_bytes(uint32_t n_bands, uint32_t n_sections) { return (uint64_t)n_bands * n_sections * kBiquadDoubles * sizeof(double); }
// bytes one banded fold moves: per band t floats read (the re-reads expected from L2), the state and r bins read and written
inline uint64_t decay_bands_fold_traffic(uint64_t nodes, uint32_t n_bands, uint32_t n_sections, uint32_t t, uint32_t r) {
    return decay_mul(decay_mul(nodes, n_bands), 4ull * t + 32ull * n_sections + 16ull * r);
}

}  // namespace wv

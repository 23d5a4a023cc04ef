// waterfall_plan.h -- (host only, no HIP, nothing but the standard library) the integer logic of waterfall maps (wv_set_waterfall,
// include/wayverb_amd.h) that is the plan's own: the cap on sums per node, the sizes of everything that is allocated for a plan, where
// the sums of a bin and a frequency lie inside the plan's one block, and the traffic model of a fold.  The stage itself and the twiddle
// table are spectrum_plan.h's, the bin of a capture and the bin table are decay_plan.h's, all unchanged (capture_stage.h holds the
// stage's bookkeeping); which steps are plan steps and whether a box lies inside the mesh is snapshot_plan.h's.
// tests/cpp/waterfall_plan_test.cpp covers this file on the CPU.
#pragma once
#include <cstdint>
#include <limits>

#include "decay_plan.h"
#include "spectrum_plan.h"

namespace wv {

constexpr int kWaterfallStage = kSpectrumStage;            // T: captures the stage holds (the engine asserts that all plans agree)
constexpr uint32_t kWaterfallMaxFreqs = kSpectrumMaxFreqs;  // K at the most
constexpr uint32_t kWaterfallMaxBins = kDecayMaxBins;       // n_bins at the most
constexpr uint32_t kWaterfallMaxSums = 4096;                // K * n_bins at the most: 64 KiB of complex sums per node
constexpr uint64_t kWaterfallNoSize = kDecayNoSize;         // "does not fit 64 bits"

// K * n_bins complex sums per node, 4096 at the most (each factor is checked on its own first: neither is 0 here)
inline bool waterfall_sums_valid(uint32_t n_freqs, uint32_t n_bins) { return (uint64_t)n_freqs * n_bins <= kWaterfallMaxSums; }

// The bin of capture j (counted 0, 1, ... since the plan was set): decay_plan.h's rule, W captures per bin, the last bin open-ended.
inline uint32_t waterfall_bin(uint64_t j, uint32_t bin_captures, uint32_t n_bins) { return decay_bin(j, bin_captures, n_bins); }

// B: nodes taken by a box of nx * ny * nz nodes (0 for an empty box)
inline uint64_t waterfall_nodes(int64_t nx, int64_t ny, int64_t nz) { return decay_nodes(nx, ny, nz); }

// bytes of the stage float[T][B], of the planar sums double[n_bins][K][2][B], of one bin table int32[T], of one twiddle table double[T][K][2]
inline uint64_t waterfall_stage_bytes(uint64_t nodes) { return decay_mul(nodes, (uint64_t)kWaterfallStage * sizeof(float)); }
inline uint64_t waterfall_sum_bytes(uint64_t nodes, uint32_t n_bins, uint32_t n_freqs) {
    return decay_mul(nodes, decay_mul((uint64_t)n_bins * n_freqs, 2 * sizeof(double)));
}
inline uint64_t waterfall_bin_table_bytes() { return decay_table_bytes(); }
inline uint64_t waterfall_twiddle_table_bytes(uint32_t n_freqs) { return spectrum_table_bytes(n_freqs); }

// offset in DOUBLES of the Re plane of bin b at frequency k inside the block (its Im plane follows it)
inline uint64_t waterfall_sum_offset(uint64_t nodes, uint32_t bin, uint32_t k, uint32_t n_freqs) {
    return decay_mul(nodes, ((uint64_t)bin * n_freqs + k) * 2);
}

// bytes that cross the link per fetch: n_bins * K complex sums per node
inline uint64_t waterfall_fetch_bytes(uint64_t nodes, uint32_t n_bins, uint32_t n_freqs) { return waterfall_sum_bytes(nodes, n_bins, n_freqs); }

// r': distinct bins among the t captures first, first + 1, ..., first + t - 1
inline uint32_t waterfall_fold_bins(uint64_t first, uint32_t t, uint32_t bin_captures, uint32_t n_bins) {
    return decay_fold_bins(first, t, bin_captures, n_bins);
}

// bytes one fold of t staged captures moves: t floats read, the K sums of each of the r' bins read and written, per node
inline uint64_t waterfall_fold_traffic(uint64_t nodes, uint32_t t, uint32_t n_freqs, uint32_t r) {
    return decay_mul(nodes, 4ull * t + 32ull * n_freqs * r);
}

}  // namespace wv

// spectrum_plan.h -- (host only, no HIP, nothing but the standard library) the integer logic of field spectra
// (wv_set_spectrum, include/wayverb_amd.h): how many captures the next batch of steps may stage, when the stage has to be
// folded into the sums, which staged captures survive a run that stopped on a flag, and the sizes of everything that is
// allocated for a plan.  Which steps are plan steps and whether a box lies inside the mesh is snapshot_plan.h's, unchanged:
// a spectrum plan captures exactly what a snapshot plan of the same box and cadence captures.
//
// The stage holds kSpectrumStage captures as dense float boxes.  A batch's captures go behind the ones already staged and
// stay there until commit_batch has said how many of the batch's steps were good; the fold takes all that are staged in one
// launch and is due only when the stage has no slot left for the next batch (engine_staged.hip.h).
// tests/cpp/spectrum_plan_test.cpp covers this file on the CPU.
#pragma once
#include <cstdint>
#include <limits>

namespace wv {

constexpr int kSpectrumStage = 16;        // T: captures the stage holds
constexpr uint32_t kSpectrumMaxFreqs = 64;  // K at the most
constexpr uint64_t kSpectrumNoSize = std::numeric_limits<uint64_t>::max();  // "does not fit 64 bits"

// a * b, kSpectrumNoSize when the product leaves 64 bits (or an operand already has)
inline uint64_t spectrum_mul(uint64_t a, uint64_t b) {
    if (a == kSpectrumNoSize || b == kSpectrumNoSize) return kSpectrumNoSize;
    if (a != 0 && b > (kSpectrumNoSize - 1) / a) return kSpectrumNoSize;
    return a * b;
}

// B: nodes taken by a box of nx * ny * nz nodes (0 for an empty box)
inline uint64_t spectrum_nodes(int64_t nx, int64_t ny, int64_t nz) {
    if (nx < 1 || ny < 1 || nz < 1) return 0;
    return spectrum_mul(spectrum_mul((uint64_t)nx, (uint64_t)ny), (uint64_t)nz);
}

// bytes of the stage float[T][B], of the planar sums double[K][2][B], of one twiddle table double[T][K][2]
inline uint64_t spectrum_stage_bytes(uint64_t nodes) { return spectrum_mul(nodes, (uint64_t)kSpectrumStage * sizeof(float)); }
inline uint64_t spectrum_sum_bytes(uint64_t nodes, uint32_t n_freqs) { return spectrum_mul(nodes, (uint64_t)n_freqs * 2 * sizeof(double)); }
inline uint64_t spectrum_table_entries(uint32_t n_freqs) { return (uint64_t)kSpectrumStage * n_freqs * 2; }
inline uint64_t spectrum_table_bytes(uint32_t n_freqs) { return spectrum_table_entries(n_freqs) * sizeof(double); }
// where the twiddle pair of staged capture j and frequency k starts in a table
inline uint64_t spectrum_table_index(uint32_t j, uint32_t k, uint32_t n_freqs) { return ((uint64_t)j * n_freqs + k) * 2; }

// bytes one fold of t staged captures moves: t floats read, K sums read and written, per node
inline uint64_t spectrum_fold_traffic(uint64_t nodes, uint32_t t, uint32_t n_freqs) {
    return spectrum_mul(nodes, 4ull * t + 32ull * n_freqs);
}

// slots the stage has left when `staged` captures wait in it
inline int spectrum_free_slots(int staged) { return staged < 0 ? kSpectrumStage : staged >= kSpectrumStage ? 0 : kSpectrumStage - staged; }

// the fold is due before the next batch is planned only when that batch could stage nothing
inline bool spectrum_fold_due(int staged) { return spectrum_free_slots(staged) == 0; }

// captures the next batch may stage: the free slots, one under graph replay (a replayed graph covers the whole batch, which
// then ends on its one capture); at least one is always possible because the fold has run when none was free
inline int spectrum_batch_captures(int staged, bool graph) {
    const int free_slots = spectrum_free_slots(staged);
    return graph ? (free_slots > 0 ? 1 : 0) : free_slots;
}

// Of the `n` capture steps a batch staged (ascending), how many are of steps <= last_good, the last step that was completed:
// those stay, the others are dropped.
inline int spectrum_good_captures(const uint64_t* steps, int n, uint64_t last_good) {
    int good = 0;
    while (good < n && steps[good] <= last_good) ++good;
    return good;
}

}  // namespace wv

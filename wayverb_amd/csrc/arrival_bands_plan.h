// arrival_bands_plan.h -- (host only, nothing but the standard library) the integer logic of band-limited arrival maps
// (wv_set_arrival_bands, include/wayverb_amd.h) that is the plan's own: which tail is refused, the bin of a capture counted from a
// node's onset less the band's lag, and the sizes and places of everything that is allocated for a plan.  Edge tables and thresholds
// are arrival_plan.h's, band and section counts decay_plan.h's; the stage is spectrum_plan.h's (capture_stage.h holds its bookkeeping).
// arrival_bands_bin is the DEFINITION of the bin.  The fold kernel evaluates it once per lane and fold and from there walks: a lane
// keeps its bin and the rel at which it moves on, read from a table the host writes (arrival_bands_bin_first), and
// tests/cpp/arrival_bands_kernel_host.cpp holds the walk to the definition.  What the kernel evaluates is constexpr: the rule exists once.
// tests/cpp/arrival_bands_plan_test.cpp covers this file on the CPU.
#pragma once
#include <cstdint>

#include "arrival_plan.h"

namespace wv {

constexpr int kArrivalBandsStage = kArrivalStage;                 // T: captures the stage holds
constexpr uint32_t kArrivalBandsMaxBins = kDecayMaxBins;          // n_edges + n_tail at the most
constexpr uint32_t kArrivalBandsMaxBands = kDecayMaxBands;        // wv_arrival_bands_plan::lag has that many entries

// What the fold needs of a wv_arrival_bands_plan, as the kernel takes it by value: every index into it is a loop counter.
struct ArrivalBandsTable {
    uint32_t edges[kArrivalMaxBins];
    uint32_t n_edges, n_tail, tail_first, tail_captures;
    uint32_t lag[kArrivalBandsMaxBands];
};

// 0 <= n_tail <= 4096 - n_edges; with a tail: tail_first > edges[n_edges - 1] and tail_captures >= 1 (without: neither is looked at)
inline bool arrival_bands_tail_count_valid(uint32_t n_edges, uint32_t n_tail) { return n_edges <= kArrivalBandsMaxBins && n_tail <= kArrivalBandsMaxBins - n_edges; }
inline bool arrival_bands_tail_first_valid(const uint32_t* edges, uint32_t n_edges, uint32_t n_tail, uint32_t tail_first) {
    return n_tail == 0 || (n_edges >= 1 && tail_first > edges[n_edges - 1]);
}
inline bool arrival_bands_tail_captures_valid(uint32_t n_tail, uint32_t tail_captures) { return n_tail == 0 || tail_captures >= 1; }

// rel of a capture d = c - onset captures behind the node's onset in a band whose clock starts `lag` captures late: the lagged stretch
// stays at 0, in bin 0
constexpr uint32_t arrival_bands_rel(uint32_t d, uint32_t lag) { return d > lag ? d - lag : 0u; }

// The bin of rel: behind tail_first the uniform tail, W captures per bin, the plan's LAST bin open-ended; ahead of it the explicit
// edges as arrival_bin counts them (whose last bin is then closed by tail_first).
constexpr uint32_t arrival_bands_bin(uint32_t rel, const ArrivalBandsTable& p) {
    if (p.n_tail > 0 && rel >= p.tail_first) {
        const uint32_t q = (rel - p.tail_first) / p.tail_captures;
        return p.n_edges + (q < p.n_tail - 1 ? q : p.n_tail - 1);
    }
    return arrival_bin(rel, p.edges, p.n_edges);
}

// The first rel of bin b, b = 0 .. n_bins - 1: an edge, or tail_first + (b - n_edges) W; kArrivalNone where that leaves 32 bits (no
// capture has that number: the bin is never reached).
inline uint32_t arrival_bands_first_rel(uint32_t b, const ArrivalBandsTable& p) {
    if (b < p.n_edges) return p.edges[b];
    const uint64_t at = (uint64_t)p.tail_first + (uint64_t)(b - p.n_edges) * p.tail_captures;
    return at >= kArrivalNone ? kArrivalNone : (uint32_t)at;
}

// The table in memory from which a lane in bin k reads the rel at which it moves on, bin_first[k + 1]: n_bins + 1 entries, the first
// rel of every bin and kArrivalNone behind the last, which is open-ended.
inline uint32_t arrival_bands_bin_first_entries(uint32_t n_bins) { return n_bins + 1; }
inline void arrival_bands_bin_first(const ArrivalBandsTable& p, uint32_t* out) {
    const uint32_t n_bins = p.n_edges + p.n_tail;
    for (uint32_t b = 0; b < n_bins; ++b) out[b] = arrival_bands_first_rel(b, p);
    out[n_bins] = kArrivalNone;
}

// Block 0, everything a fold accumulates, the doubles first so that every part is aligned whatever B is:
//   double pre[K][B], moment[K][B], bins[K][n_bins][B]; uint32 onset[K][B]; float peak[B]; uint32 peak_capture[B]
// (one onset word per band: each band's lanes carry their own copy, all equal; a fetch takes plane 0).  Block 1, the filter state:
//   double z[K][S][2][B]
// Offsets in bytes from a block's start; kDecayNoSize where a size leaves 64 bits.
inline uint64_t arrival_bands_pre_offset() { return 0; }
inline uint64_t arrival_bands_moment_offset(uint64_t nodes, uint32_t K) { return decay_mul(nodes, (uint64_t)K * sizeof(double)); }
inline uint64_t arrival_bands_bins_offset(uint64_t nodes, uint32_t K) { return decay_mul(nodes, 2ull * K * sizeof(double)); }
inline uint64_t arrival_bands_bins_bytes(uint64_t nodes, uint32_t K, uint32_t n_bins) { return decay_mul(nodes, (uint64_t)K * n_bins * sizeof(double)); }
inline uint64_t arrival_bands_onset_offset(uint64_t nodes, uint32_t K, uint32_t n_bins) { return decay_mul(nodes, (uint64_t)K * (2ull + n_bins) * sizeof(double)); }
inline uint64_t arrival_bands_peak_offset(uint64_t nodes, uint32_t K, uint32_t n_bins) {
    return arrival_add(arrival_bands_onset_offset(nodes, K, n_bins), decay_mul(nodes, 4ull * K));
}
inline uint64_t arrival_bands_peak_capture_offset(uint64_t nodes, uint32_t K, uint32_t n_bins) {
    return arrival_add(arrival_bands_onset_offset(nodes, K, n_bins), decay_mul(nodes, 4ull * K + 4));
}
inline uint64_t arrival_bands_sums_bytes(uint64_t nodes, uint32_t K, uint32_t n_bins) {
    return arrival_add(arrival_bands_onset_offset(nodes, K, n_bins), decay_mul(nodes, 4ull * K + 8));
}
inline uint64_t arrival_bands_state_bytes(uint64_t nodes, uint32_t K, uint32_t S) { return decay_band_state_bytes(nodes, K, S); }
inline uint64_t arrival_bands_stage_bytes(uint64_t nodes) { return decay_stage_bytes(nodes); }
// the coefficient table double[K][S][5] with the table uint32[n_bins + 1] of the bins' first rels behind it, one allocation
inline uint64_t arrival_bands_coef_bytes(uint32_t K, uint32_t S) { return decay_band_coef_bytes(K, S); }
inline uint64_t arrival_bands_tables_bytes(uint32_t K, uint32_t S, uint32_t n_bins) {
    return arrival_bands_coef_bytes(K, S) + (uint64_t)arrival_bands_bin_first_entries(n_bins) * sizeof(uint32_t);
}

// Bytes one fold of t staged captures moves, in the steady state where every node has its onset behind it: per band
// t floats read (the K - 1 re-reads expected from L2), the filter state read and written (32 S), the band's onset word and the moment
// read (12 B), the moment written (8 B), r bins read and written; band 0 also reads peak and peak_capture (8 B per node, once); the
// threshold where a map gives it (4 B per band).
inline uint64_t arrival_bands_fold_traffic(uint64_t nodes, uint32_t K, uint32_t S, uint32_t t, uint32_t r, bool map) {
    return arrival_add(decay_mul(decay_mul(nodes, K), 4ull * t + 32ull * S + 20ull + 16ull * r + (map ? 4ull : 0ull)), decay_mul(nodes, 8));
}

}  // namespace wv

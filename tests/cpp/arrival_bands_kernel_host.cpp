// arrival_bands_kernel_host.cpp -- (CPU, stand-alone) the text of arrival_bands_fold_kernel (wayverb_amd/csrc/arrival_bands_kernels.hip.h)
// compiled for the host over tests/cpp/hip_stub and called once per lane, band after band and fold after fold as
// engine_arrival_bands.hip.h launches it: indices, the tail of B, the onset copies of the bands, the lane's walk through explicit and
// tail bins, the state carried from fold to fold (and what is NOT stored because it cannot have changed) and the order of every
// operation are then the kernel's own, and tests/test_arrival_bands_host.py compares every output and the filter states with
// arrival.banded_arrival_fold byte for byte.  Both blocks and the table of the bins' first rels are allocated at arrival_bands_plan.h's
// sizes, as the engine allocates them, so a wrong offset or size shows under -fsanitize=address.  The bands run in DESCENDING order
// within a fold: a lane that read another band's onset copy, or band 0's after band 0 had stored it, would differ.  (What only the
// device can show -- the code the compiler makes of it for gfx950 -- is tests/test_gpu_arrival_bands.py's.)
//
// usage: arrival_bands_kernel_host IN OUT
//   IN:  uint64 nodes, K, S, T, first_fold, has_map; ArrivalBandsTable as it lies (uint32 edges[16], n_edges, n_tail, tail_first,
//        tail_captures, lag[8]); float threshold; double coef[K][S][5]; float map[nodes] (if has_map); float snaps[T][nodes]
//   OUT: block 0 as it lies (double pre[K][B], moment[K][B], bins[K][n_bins][B]; uint32 onset[K][B]; float peak[B]; uint32
//        peak_capture[B]), then block 1 (double z[K][S][2][B])
#include "arrival_bands_kernels.hip.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

template <int S>
static void fold(const float* stage, double* state, unsigned char* sums, const float* map, float threshold, const double* coef, const uint32_t* bin_first,
                 const wv::ArrivalBandsTable& table, uint32_t first, uint64_t nodes, int t, uint32_t K) {
    const uint32_t n_bins = table.n_edges + table.n_tail;
    for (unsigned by = K; by-- > 0;)
        for (unsigned bx = 0; bx < (nodes + 255) / 256; ++bx)
            for (unsigned tx = 0; tx < 256; ++tx) {
                blockIdx = {bx, by, 0};
                threadIdx = {tx, 0, 0};
                wv::arrival_bands_fold_kernel<S>(stage, state, reinterpret_cast<double*>(sums + wv::arrival_bands_pre_offset()),
                                                 reinterpret_cast<double*>(sums + wv::arrival_bands_moment_offset(nodes, K)),
                                                 reinterpret_cast<double*>(sums + wv::arrival_bands_bins_offset(nodes, K)),
                                                 reinterpret_cast<uint32_t*>(sums + wv::arrival_bands_onset_offset(nodes, K, n_bins)),
                                                 reinterpret_cast<float*>(sums + wv::arrival_bands_peak_offset(nodes, K, n_bins)),
                                                 reinterpret_cast<uint32_t*>(sums + wv::arrival_bands_peak_capture_offset(nodes, K, n_bins)), map, threshold,
                                                 coef, bin_first, table, first, nodes, t);
            }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t h[6];
    wv::ArrivalBandsTable table;
    float threshold;
    static_assert(sizeof(table) == 28 * 4, "the table as the tests write it");
    if (std::fread(h, 8, 6, f) != 6 || std::fread(&table, sizeof(table), 1, f) != 1 || std::fread(&threshold, 4, 1, f) != 1) return 2;
    const uint64_t nodes = h[0], T = h[3], first_fold = h[4], has_map = h[5];
    const uint32_t K = (uint32_t)h[1], S = (uint32_t)h[2];
    if (!wv::decay_bands_valid(K, S) || !wv::arrival_edges_valid(table.edges, table.n_edges) || !wv::arrival_bands_tail_count_valid(table.n_edges, table.n_tail) ||
        !wv::arrival_bands_tail_first_valid(table.edges, table.n_edges, table.n_tail, table.tail_first) ||
        !wv::arrival_bands_tail_captures_valid(table.n_tail, table.tail_captures) || first_fold < 1 || first_fold > (uint64_t)wv::kArrivalBandsStage)
        return 2;
    const uint32_t n_bins = table.n_edges + table.n_tail;
    std::vector<double> coef((size_t)K * S * 5);
    std::vector<float> map(has_map ? nodes : 0), snaps(T * nodes);
    if (std::fread(coef.data(), 8, coef.size(), f) != coef.size() || std::fread(map.data(), 4, map.size(), f) != map.size() ||
        std::fread(snaps.data(), 4, snaps.size(), f) != snaps.size())
        return 2;
    std::fclose(f);
    // the engine's allocation and initialisation: zeros, then all bits set in every band's onsets and in the peak captures
    const uint64_t bytes = wv::arrival_bands_sums_bytes(nodes, K, n_bins), state_bytes = wv::arrival_bands_state_bytes(nodes, K, S);
    if (bytes == wv::kDecayNoSize || state_bytes == wv::kDecayNoSize) return 2;
    unsigned char* sums = new unsigned char[bytes];   // (exactly the size: the sanitizer sees a byte past it)
    double* state = new double[state_bytes / 8];
    uint32_t* bin_first = new uint32_t[wv::arrival_bands_bin_first_entries(n_bins)];
    std::memset(sums, 0, bytes);
    std::memset(sums + wv::arrival_bands_onset_offset(nodes, K, n_bins), 0xFF, nodes * 4 * K);
    std::memset(sums + wv::arrival_bands_peak_capture_offset(nodes, K, n_bins), 0xFF, nodes * 4);
    std::memset(state, 0, state_bytes);
    wv::arrival_bands_bin_first(table, bin_first);
    for (uint64_t folded = 0; folded < T;) {
        // (the first fold may be short, as one cut by a fetch mid-run is)
        const int t = (int)std::min<uint64_t>(folded == 0 ? first_fold : (uint64_t)wv::kArrivalBandsStage, T - folded);
        // slot j of the stage = capture folded + j; a stage of exactly t slots, so that a read of slot t is a read out of bounds
        std::vector<float> stage(snaps.begin() + folded * nodes, snaps.begin() + (folded + t) * nodes);
        const float* m = has_map ? map.data() : nullptr;
        switch (S) {
            case 1: fold<1>(stage.data(), state, sums, m, threshold, coef.data(), bin_first, table, (uint32_t)folded, nodes, t, K); break;
            case 2: fold<2>(stage.data(), state, sums, m, threshold, coef.data(), bin_first, table, (uint32_t)folded, nodes, t, K); break;
            case 3: fold<3>(stage.data(), state, sums, m, threshold, coef.data(), bin_first, table, (uint32_t)folded, nodes, t, K); break;
            default: fold<4>(stage.data(), state, sums, m, threshold, coef.data(), bin_first, table, (uint32_t)folded, nodes, t, K); break;
        }
        folded += t;
    }
    // every band's copy of the onset is the same
    const uint32_t* onset = reinterpret_cast<const uint32_t*>(sums + wv::arrival_bands_onset_offset(nodes, K, n_bins));
    for (uint32_t k = 1; k < K; ++k)
        if (std::memcmp(onset, onset + (uint64_t)k * nodes, nodes * 4) != 0) return 3;
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::fwrite(sums, 1, bytes, o);
    std::fwrite(state, 1, state_bytes, o);
    std::fclose(o);
    delete[] sums;
    delete[] state;
    delete[] bin_first;
    return 0;
}

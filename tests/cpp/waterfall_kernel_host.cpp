// waterfall_kernel_host.cpp -- (CPU, stand-alone) the text of waterfall_fold_kernel (wayverb_amd/csrc/waterfall_kernels.hip.h) compiled
// for the host over tests/cpp/hip_stub and called once per lane, fold after fold as engine_waterfall.hip.h launches it: indices, the
// tail of B, the chunks of frequencies, the held bin and the order of every operation are then the kernel's own, and
// tests/test_waterfall_host.py compares the sums with waterfall.waterfall_fold byte for byte.  The sums, every fold's stage and both of
// its tables are allocated at exactly the sizes the fold may touch, so that under -fsanitize=address an index past either end is seen.
// (What only the device can show -- the code the compiler makes of it for gfx950 -- is tests/test_gpu_waterfall.py's.)
//
// usage: waterfall_kernel_host IN OUT
//   IN:  uint64 nodes, K, n_bins, bin_captures, T, first_fold, first_capture, wide; double tw[T][K][2]; float snaps[T][nodes]
//   OUT: double sums[n_bins][K][2][nodes]
#include "waterfall_kernels.hip.h"

#include <algorithm>
#include <cstdio>
#include <vector>

template <bool WIDE>
static void fold(const float* stage, double* acc, const int32_t* bin, const double* tw, uint64_t nodes, int t, int n_freqs) {
    const uint64_t items = WIDE ? nodes / 2 : nodes;
    for (unsigned bx = 0; bx < (items + 255) / 256; ++bx)
        for (unsigned tx = 0; tx < 256; ++tx) {
            blockIdx = {bx, 0, 0};
            threadIdx = {tx, 0, 0};
            wv::waterfall_fold_kernel<WIDE>(stage, acc, bin, tw, nodes, t, n_freqs);
        }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t h[8];
    if (std::fread(h, 8, 8, f) != 8) return 2;
    const uint64_t nodes = h[0], K = h[1], n_bins = h[2], W = h[3], T = h[4], first_fold = h[5], first_capture = h[6], wide = h[7];
    if (K < 1 || K > wv::kWaterfallMaxFreqs || n_bins < 1 || n_bins > wv::kWaterfallMaxBins || W < 1 || first_fold < 1 ||
        !wv::waterfall_sums_valid((uint32_t)K, (uint32_t)n_bins) || (wide && nodes % 2))
        return 2;
    std::vector<double> tw(T * K * 2);
    std::vector<float> snaps(T * nodes);
    if (std::fread(tw.data(), 8, tw.size(), f) != tw.size() || std::fread(snaps.data(), 4, snaps.size(), f) != snaps.size()) return 2;
    std::fclose(f);
    std::vector<double> sums(wv::waterfall_sum_bytes(nodes, (uint32_t)n_bins, (uint32_t)K) / 8, 0.0);
    for (uint64_t folded = 0; folded < T;) {
        // (the first fold may be short, as one cut by a fetch mid-run is)
        const int t = (int)std::min<uint64_t>(folded == 0 ? first_fold : (uint64_t)wv::kWaterfallStage, T - folded);
        // slot j of the stage = capture first_capture + folded + j; the fold's tables hold exactly its t captures, as the engine copies them
        std::vector<float> stage(snaps.begin() + folded * nodes, snaps.begin() + (folded + t) * nodes);
        std::vector<double> table(tw.begin() + folded * K * 2, tw.begin() + (folded + t) * K * 2);
        std::vector<int32_t> bin((size_t)t);
        for (int j = 0; j < t; ++j) bin[(size_t)j] = (int32_t)wv::waterfall_bin(first_capture + folded + (uint64_t)j, (uint32_t)W, (uint32_t)n_bins);
        if (wide)
            fold<true>(stage.data(), sums.data(), bin.data(), table.data(), nodes, t, (int)K);
        else
            fold<false>(stage.data(), sums.data(), bin.data(), table.data(), nodes, t, (int)K);
        folded += t;
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::fwrite(sums.data(), 8, sums.size(), o);
    std::fclose(o);
    return 0;
}

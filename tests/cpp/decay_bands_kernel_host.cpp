// decay_bands_kernel_host.cpp -- (CPU, stand-alone) the text of decay_bands_fold_kernel (wayverb_amd/csrc/decay_bands_kernels.hip.h)
// compiled for the host over tests/cpp/hip_stub and called once per lane, fold after fold as engine_decay.hip.h launches it: indices,
// the tail of B, the bin switch, the state carried from fold to fold and the order of every operation are then the kernel's own, and
// tests/test_decay_bands_host.py compares bins and states with decay.banded_bins byte for byte.  (What only the device can show --
// the code the compiler makes of it for gfx950 -- is tests/test_gpu_decay_bands.py's.)
//
// usage: decay_bands_kernel_host IN OUT
//   IN:  uint64 nodes, n_bins, K, S, T, W, first_fold; double coef[K][S][5]; float snaps[T][nodes]
//   OUT: double bins[K][n_bins][nodes]; double state[K][S][2][nodes]
#include "decay_bands_kernels.hip.h"

#include <algorithm>
#include <cstdio>
#include <vector>

template <int S>
static void fold(const float* stage, double* state, double* bins, const double* coef, const int32_t* bin, uint64_t nodes, uint32_t n_bins, int t,
                 unsigned n_bands) {
    for (unsigned by = 0; by < n_bands; ++by)
        for (unsigned bx = 0; bx < (nodes + 255) / 256; ++bx)
            for (unsigned tx = 0; tx < 256; ++tx) {
                blockIdx = {bx, by, 0};
                threadIdx = {tx, 0, 0};
                wv::decay_bands_fold_kernel<S>(stage, state, bins, coef, bin, nodes, n_bins, t);
            }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t h[7];
    if (std::fread(h, 8, 7, f) != 7) return 2;
    const uint64_t nodes = h[0], n_bins = h[1], K = h[2], S = h[3], T = h[4], W = h[5], first_fold = h[6];
    std::vector<double> coef(K * S * 5);
    std::vector<float> snaps(T * nodes);
    if (std::fread(coef.data(), 8, coef.size(), f) != coef.size() || std::fread(snaps.data(), 4, snaps.size(), f) != snaps.size()) return 2;
    std::fclose(f);
    std::vector<double> state(K * S * 2 * nodes, 0.0), bins(K * n_bins * nodes, 0.0);
    for (uint64_t folded = 0; folded < T;) {
        // (the first fold may be short, as one cut by a fetch mid-run is)
        const int t = (int)std::min<uint64_t>(folded == 0 ? first_fold : (uint64_t)wv::kDecayStage, T - folded);
        int32_t bin[wv::kDecayStage];
        for (int j = 0; j < t; ++j) bin[j] = (int32_t)wv::decay_bin(folded + j, (uint32_t)W, (uint32_t)n_bins);
        const float* stage = snaps.data() + folded * nodes;   // slot j of the stage = capture folded + j
        switch (S) {
            case 1: fold<1>(stage, state.data(), bins.data(), coef.data(), bin, nodes, (uint32_t)n_bins, t, (unsigned)K); break;
            case 2: fold<2>(stage, state.data(), bins.data(), coef.data(), bin, nodes, (uint32_t)n_bins, t, (unsigned)K); break;
            case 3: fold<3>(stage, state.data(), bins.data(), coef.data(), bin, nodes, (uint32_t)n_bins, t, (unsigned)K); break;
            case 4: fold<4>(stage, state.data(), bins.data(), coef.data(), bin, nodes, (uint32_t)n_bins, t, (unsigned)K); break;
            default: return 2;
        }
        folded += t;
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::fwrite(bins.data(), 8, bins.size(), o);
    std::fwrite(state.data(), 8, state.size(), o);
    std::fclose(o);
    return 0;
}

// modulation_kernel_host.cpp -- (CPU, stand-alone) the text of modulation_fold_kernel (wayverb_amd/csrc/modulation_kernels.hip.h)
// compiled for the host over tests/cpp/hip_stub and called once per lane and band, fold after fold as engine_modulation.hip.h launches
// it: indices, the tail of B, the chunks of frequencies, the state carried from fold to fold and the order of every operation are then
// the kernel's own, and tests/test_modulation_host.py compares sums and states with modulation.modulation_fold byte for byte.  The
// blocks are allocated at exactly modulation_plan.h's byte counts, so that under -fsanitize=address an index past either end is seen.
// (What only the device can show -- the code the compiler makes of it for gfx950 -- is tests/test_gpu_modulation.py's.)
//
// usage: modulation_kernel_host IN OUT
//   IN:  uint64 nodes, K, S, M, T, first_fold; double coef[K][S][5]; double tw[T][M][2]; float snaps[T][nodes]
//   OUT: double sums[K][1 + 2 M][nodes]; double state[K][S][2][nodes]
#include "modulation_kernels.hip.h"

#include <algorithm>
#include <cstdio>
#include <vector>

template <int S>
static void fold(const float* stage, double* state, double* sums, const double* coef, const double* tw, uint64_t nodes, int n_freqs, int t, unsigned n_bands) {
    for (unsigned by = 0; by < n_bands; ++by)
        for (unsigned bx = 0; bx < (nodes + 255) / 256; ++bx)
            for (unsigned tx = 0; tx < 256; ++tx) {
                blockIdx = {bx, by, 0};
                threadIdx = {tx, 0, 0};
                wv::modulation_fold_kernel<S>(stage, state, sums, coef, tw, nodes, n_freqs, t);
            }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t h[6];
    if (std::fread(h, 8, 6, f) != 6) return 2;
    const uint64_t nodes = h[0], K = h[1], S = h[2], M = h[3], T = h[4], first_fold = h[5];
    if (!wv::modulation_valid((uint32_t)K, (uint32_t)S, (uint32_t)M) || first_fold < 1) return 2;
    std::vector<double> coef(K * S * 5), tw(T * M * 2);
    std::vector<float> snaps(T * nodes);
    if (std::fread(coef.data(), 8, coef.size(), f) != coef.size() || std::fread(tw.data(), 8, tw.size(), f) != tw.size() ||
        std::fread(snaps.data(), 4, snaps.size(), f) != snaps.size())
        return 2;
    std::fclose(f);
    std::vector<double> state(wv::modulation_state_bytes(nodes, (uint32_t)K, (uint32_t)S) / 8, 0.0);
    std::vector<double> sums(wv::modulation_sums_bytes(nodes, (uint32_t)K, (uint32_t)M) / 8, 0.0);
    for (uint64_t folded = 0; folded < T;) {
        // (the first fold may be short, as one cut by a fetch mid-run is)
        const int t = (int)std::min<uint64_t>(folded == 0 ? first_fold : (uint64_t)wv::kModulationStage, T - folded);
        // slot j of the stage = capture folded + j; the fold's table holds exactly its t captures' twiddles, as the engine copies them
        std::vector<float> stage(snaps.begin() + folded * nodes, snaps.begin() + (folded + t) * nodes);
        std::vector<double> table(tw.begin() + folded * M * 2, tw.begin() + (folded + t) * M * 2);
        switch (S) {
            case 1: fold<1>(stage.data(), state.data(), sums.data(), coef.data(), table.data(), nodes, (int)M, t, (unsigned)K); break;
            case 2: fold<2>(stage.data(), state.data(), sums.data(), coef.data(), table.data(), nodes, (int)M, t, (unsigned)K); break;
            case 3: fold<3>(stage.data(), state.data(), sums.data(), coef.data(), table.data(), nodes, (int)M, t, (unsigned)K); break;
            case 4: fold<4>(stage.data(), state.data(), sums.data(), coef.data(), table.data(), nodes, (int)M, t, (unsigned)K); break;
            default: return 2;
        }
        folded += t;
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::fwrite(sums.data(), 8, sums.size(), o);
    std::fwrite(state.data(), 8, state.size(), o);
    std::fclose(o);
    return 0;
}

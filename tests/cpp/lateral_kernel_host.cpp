// lateral_kernel_host.cpp -- (CPU, stand-alone) the text of lateral_fold_kernel (wayverb_amd/csrc/lateral_kernels.hip.h) compiled for
// the host over tests/cpp/hip_stub and called once per lane, fold after fold as engine_lateral.hip.h launches it: indices, the tail of
// B, the onset, the integrator that runs ahead of it, the lane's own bin switch with its ten held sums, the state carried from fold
// to fold (and what is NOT stored because it cannot have changed) and the order of every operation are then the kernel's own, and
// tests/test_lateral_host.py compares onset, pre, the velocities and all ten bin planes with lateral.lateral_fold byte for byte.
// The state lies in one block at lateral_plan.h's offsets, as the engine allocates it, so a wrong offset or size shows under
// -fsanitize=address.  (What only the device can show -- the code the compiler makes of it for gfx950 -- is
// tests/test_gpu_lateral.py's.)
//
// usage: lateral_kernel_host IN OUT
//   IN:  uint64 nodes, n_bins, T, first_fold, has_map; uint32 edges[8]; float threshold; double k; float map[nodes] (if has_map);
//        float staged[T][4][nodes] (pressure, gx, gy, gz of every capture, as intensity_gather_kernel writes them)
//   OUT: the state block as it lies: double pre[B], velocity[3][B], bins[10][n_bins][B]; uint32 onset[B]
#include "lateral_kernels.hip.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t h[5];
    uint32_t plan_edges[wv::kLateralMaxBins];
    float threshold;
    double k;
    if (std::fread(h, 8, 5, f) != 5 || std::fread(plan_edges, 4, 8, f) != 8 || std::fread(&threshold, 4, 1, f) != 1 || std::fread(&k, 8, 1, f) != 1) return 2;
    const uint64_t nodes = h[0], T = h[2], first_fold = h[3], has_map = h[4];
    const uint32_t n_bins = (uint32_t)h[1];
    if (n_bins > wv::kLateralMaxBins || !wv::arrival_edges_valid(plan_edges, n_bins) || first_fold < 1 || first_fold > (uint64_t)wv::kLateralStage) return 2;
    // (as the engine fills the kernel's table: the plan's entries first)
    wv::ArrivalEdges edges;
    for (uint32_t m = 0; m < wv::kArrivalMaxBins; ++m) edges.e[m] = m < wv::kLateralMaxBins ? plan_edges[m] : wv::kLateralNone;
    std::vector<float> map(has_map ? nodes : 0), snaps(T * 4 * nodes);
    if (std::fread(map.data(), 4, map.size(), f) != map.size() || std::fread(snaps.data(), 4, snaps.size(), f) != snaps.size()) return 2;
    std::fclose(f);
    // the engine's allocation and initialisation: zeros, then all bits set in the onsets
    const uint64_t bytes = wv::lateral_state_bytes(nodes, n_bins);
    if (bytes == wv::kDecayNoSize) return 2;
    unsigned char* state = new unsigned char[bytes];   // (exactly the size: the sanitizer sees a byte past it)
    std::memset(state, 0, bytes);
    std::memset(state + wv::lateral_onset_offset(nodes, n_bins), 0xFF, nodes * 4);
    for (uint64_t folded = 0; folded < T;) {
        // (the first fold may be short, as one cut by a fetch mid-run is)
        const int t = (int)std::min<uint64_t>(folded == 0 ? first_fold : (uint64_t)wv::kLateralStage, T - folded);
        // slot j of the stage = capture folded + j; a stage of exactly t slots, so that a read of slot t is a read out of bounds
        std::vector<float> stage(snaps.begin() + folded * 4 * nodes, snaps.begin() + (folded + t) * 4 * nodes);
        for (unsigned bx = 0; bx < (nodes + 255) / 256; ++bx)
            for (unsigned tx = 0; tx < 256; ++tx) {
                blockIdx = {bx, 0, 0};
                threadIdx = {tx, 0, 0};
                wv::lateral_fold_kernel(stage.data(), reinterpret_cast<double*>(state + wv::lateral_pre_offset()),
                                        reinterpret_cast<double*>(state + wv::lateral_velocity_offset(nodes)),
                                        reinterpret_cast<double*>(state + wv::lateral_bins_offset(nodes)),
                                        reinterpret_cast<uint32_t*>(state + wv::lateral_onset_offset(nodes, n_bins)), has_map ? map.data() : nullptr,
                                        threshold, edges, n_bins, (uint32_t)folded, nodes, k, t);
            }
        folded += t;
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::fwrite(state, 1, bytes, o);
    std::fclose(o);
    delete[] state;
    return 0;
}

// arrival_kernel_host.cpp -- (CPU, stand-alone) the text of arrival_fold_kernel (wayverb_amd/csrc/arrival_kernels.hip.h) compiled for
// the host over tests/cpp/hip_stub and called once per lane, fold after fold as engine_arrival.hip.h launches it: indices, the tail of
// B, the onset, the lane's own bin switch, the state carried from fold to fold (and what is NOT stored because it cannot have changed)
// and the order of every operation are then the kernel's own, and tests/test_arrival_host.py compares all six outputs with
// arrival.arrival_fold byte for byte.  The state lies in one block at arrival_plan.h's offsets, as the engine allocates it, so a
// wrong offset or size shows under -fsanitize=address.  (What only the device can show -- the code the compiler makes of it for
// gfx950 -- is tests/test_gpu_arrival.py's.)
//
// usage: arrival_kernel_host IN OUT
//   IN:  uint64 nodes, n_bins, T, first_fold, has_map; uint32 edges[16]; float threshold; float map[nodes] (if has_map);
//        float snaps[T][nodes]
//   OUT: the state block as it lies: double pre[B], moment[B], bins[n_bins][B]; uint32 onset[B]; float peak[B]; uint32 peak_capture[B]
#include "arrival_kernels.hip.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t h[5];
    wv::ArrivalEdges edges;
    float threshold;
    if (std::fread(h, 8, 5, f) != 5 || std::fread(edges.e, 4, 16, f) != 16 || std::fread(&threshold, 4, 1, f) != 1) return 2;
    const uint64_t nodes = h[0], T = h[2], first_fold = h[3], has_map = h[4];
    const uint32_t n_bins = (uint32_t)h[1];
    if (!wv::arrival_edges_valid(edges.e, n_bins) || first_fold < 1 || first_fold > (uint64_t)wv::kArrivalStage) return 2;
    std::vector<float> map(has_map ? nodes : 0), snaps(T * nodes);
    if (std::fread(map.data(), 4, map.size(), f) != map.size() || std::fread(snaps.data(), 4, snaps.size(), f) != snaps.size()) return 2;
    std::fclose(f);
    // the engine's allocation and initialisation: zeros, then all bits set in the onsets and the peak captures
    const uint64_t bytes = wv::arrival_state_bytes(nodes, n_bins);
    if (bytes == wv::kDecayNoSize) return 2;
    unsigned char* state = new unsigned char[bytes];   // (exactly the size: the sanitizer sees a byte past it)
    std::memset(state, 0, bytes);
    std::memset(state + wv::arrival_onset_offset(nodes, n_bins), 0xFF, nodes * 4);
    std::memset(state + wv::arrival_peak_capture_offset(nodes, n_bins), 0xFF, nodes * 4);
    for (uint64_t folded = 0; folded < T;) {
        // (the first fold may be short, as one cut by a fetch mid-run is)
        const int t = (int)std::min<uint64_t>(folded == 0 ? first_fold : (uint64_t)wv::kArrivalStage, T - folded);
        // slot j of the stage = capture folded + j; a stage of exactly t slots, so that a read of slot t is a read out of bounds
        std::vector<float> stage(snaps.begin() + folded * nodes, snaps.begin() + (folded + t) * nodes);
        for (unsigned bx = 0; bx < (nodes + 255) / 256; ++bx)
            for (unsigned tx = 0; tx < 256; ++tx) {
                blockIdx = {bx, 0, 0};
                threadIdx = {tx, 0, 0};
                wv::arrival_fold_kernel(stage.data(), reinterpret_cast<double*>(state + wv::arrival_pre_offset()),
                                        reinterpret_cast<double*>(state + wv::arrival_moment_offset(nodes)),
                                        reinterpret_cast<double*>(state + wv::arrival_bins_offset(nodes)),
                                        reinterpret_cast<uint32_t*>(state + wv::arrival_onset_offset(nodes, n_bins)),
                                        reinterpret_cast<float*>(state + wv::arrival_peak_offset(nodes, n_bins)),
                                        reinterpret_cast<uint32_t*>(state + wv::arrival_peak_capture_offset(nodes, n_bins)),
                                        has_map ? map.data() : nullptr, threshold, edges, n_bins, (uint32_t)folded, nodes, t);
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

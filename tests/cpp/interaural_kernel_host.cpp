// interaural_kernel_host.cpp -- (CPU, stand-alone) the text of interaural_fold_kernel and ear_gather_kernel
// (wayverb_amd/csrc/interaural_kernels.hip.h) compiled for the host over tests/cpp/hip_stub and called once per lane, fold after fold as
// engine_interaural.hip.h launches it -- the same instance for the same plan, the same places inside the two blocks: indices, the tail
// of B, the ring of the history, the passes over the lags, the held bin and the order of every operation are then the kernel's own, and
// tests/test_interaural_host.py compares onset, pre and bins with interaural.interaural_fold byte for byte.  Both blocks and every
// fold's stage are allocated at exactly the sizes the plan header gives, so that under -fsanitize=address an index past either end is
// seen.  (What only the device can show -- the code the compiler makes of it for gfx950 -- is tests/test_gpu_interaural.py's.)
//
// usage: interaural_kernel_host IN OUT
//   IN:  uint64 nodes, L, n_bins, S, T, first_fold, first_capture, has_map; uint32 edges[4]; float threshold; float map[nodes] (if
//        has_map); double coef[S][5]; float a[T][nodes]; float b[T][nodes]
//   OUT: block 0 as it lies: double pre[2][nodes], bins[n_bins][2 L + 3][nodes]; uint32 onset[nodes]
//
// usage: interaural_kernel_host gather IN OUT
//   IN:  int32 mesh nx, ny, nz, pitch; x0, y0, z0, nx, ny, nz, sx, sy, sz; ear_a[3], ear_b[3]; float field[nz][ny][pitch]
//   OUT: float stage[2][nodes]
#include <hip/hip_runtime.h>
static thread_local wv_stub_dim3 gridDim;  // (the capture kernel strides over the grid; the stand-in has the two indices only)

#include "interaural_kernels.hip.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

template <int SMAX, int LMAX>
static void fold(const float* stage, unsigned char* sums, unsigned char* carry, const double* coef, const float* map, float threshold,
                 const wv::InterauralEdges& edges, uint32_t n_bins, uint32_t L, uint32_t S, uint32_t first, uint64_t nodes, int t) {
    for (unsigned bx = 0; bx < (nodes + 255) / 256; ++bx)
        for (unsigned tx = 0; tx < 256; ++tx) {
            blockIdx = {bx, 0, 0};
            threadIdx = {tx, 0, 0};
            wv::interaural_fold_kernel<SMAX, LMAX>(stage, reinterpret_cast<double*>(sums + wv::interaural_pre_offset()),
                                                   reinterpret_cast<double*>(sums + wv::interaural_bins_offset(nodes)),
                                                   reinterpret_cast<uint32_t*>(sums + wv::interaural_onset_offset(nodes, n_bins, L)),
                                                   reinterpret_cast<double*>(carry), reinterpret_cast<double*>(carry + wv::interaural_filter_offset(nodes, L)), coef,
                                                   map, threshold, edges, n_bins, L, S, first, nodes, t);
        }
}

static int gather(const char* in, const char* out) {
    FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    int32_t h[19];
    if (std::fread(h, 4, 19, f) != 19) return 2;
    const int64_t pitch = h[3];
    std::vector<float> field((size_t)h[2] * h[1] * pitch);
    if (std::fread(field.data(), 4, field.size(), f) != field.size()) return 2;
    std::fclose(f);
    wv::EarGatherArgs<float> a{};
    a.field = field.data();
    a.pitch = pitch, a.mesh_ny = h[1];
    a.x0 = h[4], a.y0 = h[5], a.z0 = h[6], a.nx = h[7], a.ny = h[8], a.nz = h[9], a.sx = h[10], a.sy = h[11], a.sz = h[12];
    a.nodes = (int64_t)a.nx * a.ny * a.nz;
    a.ear_a = ((int64_t)h[15] * h[1] + h[14]) * pitch + h[13];
    a.ear_b = ((int64_t)h[18] * h[1] + h[17]) * pitch + h[16];
    std::vector<float> stage((size_t)a.nodes * 2);
    a.dst = stage.data();
    gridDim = {2, 2, 1};  // (fewer blocks than the box needs: the stride loops run)
    for (unsigned by = 0; by < gridDim.y; ++by)
        for (unsigned bx = 0; bx < gridDim.x; ++bx)
            for (unsigned tx = 0; tx < 256; ++tx) {
                blockIdx = {bx, by, 0};
                threadIdx = {tx, 0, 0};
                wv::ear_gather_kernel<float>(a);
            }
    FILE* o = std::fopen(out, "wb");
    if (!o) return 2;
    std::fwrite(stage.data(), 4, stage.size(), o);
    std::fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "gather")) return gather(argv[2], argv[3]);
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t h[8];
    if (std::fread(h, 8, 8, f) != 8) return 2;
    const uint64_t nodes = h[0], T = h[4], first_fold = h[5], first_capture = h[6], has_map = h[7];
    const uint32_t L = (uint32_t)h[1], n_bins = (uint32_t)h[2], S = (uint32_t)h[3];
    wv::InterauralEdges edges;
    float threshold;
    if (std::fread(edges.e, 4, 4, f) != 4 || std::fread(&threshold, 4, 1, f) != 1) return 2;
    if (L > wv::kInterauralMaxLag || n_bins < 1 || n_bins > wv::kInterauralMaxBins || S > wv::kInterauralMaxSections || first_fold < 1) return 2;
    std::vector<float> map(has_map ? nodes : 0);
    std::vector<double> coef((size_t)S * 5);
    std::vector<float> a(T * nodes), b(T * nodes);
    if (std::fread(map.data(), 4, map.size(), f) != map.size() || std::fread(coef.data(), 8, coef.size(), f) != coef.size() ||
        std::fread(a.data(), 4, a.size(), f) != a.size() || std::fread(b.data(), 4, b.size(), f) != b.size())
        return 2;
    std::fclose(f);
    // the setter's first contents: +0.0 everywhere, NONE in the onsets
    std::vector<unsigned char> sums(wv::interaural_sums_bytes(nodes, n_bins, L), 0), carry(wv::interaural_carry_bytes(nodes, L, S), 0);
    std::memset(sums.data() + wv::interaural_onset_offset(nodes, n_bins, L), 0xFF, nodes * 4);
    for (uint64_t folded = 0; folded < T;) {
        // (the first fold may be short, as one cut by a fetch mid-run is)
        const int t = (int)std::min<uint64_t>(folded == 0 ? first_fold : (uint64_t)wv::kInterauralStage, T - folded);
        std::vector<float> stage((size_t)t * 2 * nodes);  // slot j: ear a's plane, then ear b's, exactly the t captures
        for (int j = 0; j < t; ++j) {
            std::copy(a.begin() + (folded + j) * nodes, a.begin() + (folded + j + 1) * nodes, stage.begin() + (size_t)j * 2 * nodes);
            std::copy(b.begin() + (folded + j) * nodes, b.begin() + (folded + j + 1) * nodes, stage.begin() + ((size_t)j * 2 + 1) * nodes);
        }
        const uint32_t first = (uint32_t)(first_capture + folded);
        const float* m = has_map ? map.data() : nullptr;
        const double* c = S ? coef.data() : nullptr;
#define FOLD(SMAX, LMAX) fold<SMAX, LMAX>(stage.data(), sums.data(), carry.data(), c, m, threshold, edges, n_bins, L, S, first, nodes, t)
        switch (wv::interaural_lag_class(L) + (S ? 1u : 0u)) {  // (engine_interaural.hip.h: interaural_enqueue)
            case 0: FOLD(0, 0); break;
            case 1: FOLD(4, 0); break;
            case 4: FOLD(0, 4); break;
            case 5: FOLD(4, 4); break;
            case 8: FOLD(0, 8); break;
            case 9: FOLD(4, 8); break;
            case 16: FOLD(0, 16); break;
            default: FOLD(4, 16); break;
        }
#undef FOLD
        folded += t;
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::fwrite(sums.data(), 1, sums.size(), o);
    std::fclose(o);
    return 0;
}

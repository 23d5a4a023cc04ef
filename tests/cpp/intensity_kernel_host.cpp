// intensity_kernel_host.cpp -- (CPU, stand-alone) the text of intensity_gather_kernel and intensity_fold_kernel
// (wayverb_amd/csrc/intensity_kernels.hip.h) compiled for the host over tests/cpp/hip_stub and called once per lane: a capture per
// stored field into the next slot of the stage, a fold whenever the stage is full (and at the end), as engine_intensity.hip.h
// launches them.  Indices into the row-padded field, the neighbours' offsets, the tail of B, the bin switch, the velocities carried
// from fold to fold and the order of every operation are then the kernels' own, and tests/test_intensity_plan.py compares bins and
// velocities with intensity.intensity_bins byte for byte.  (What only the device can show -- the code the compiler makes of it for
// gfx950 -- is tests/test_gpu_intensity.py's.)
//
// usage: intensity_kernel_host IN OUT
//   IN:  uint64 real_bytes (4 | 8), mesh_ny, mesh_nz, pitch, x0, y0, z0, nx, ny, nz, sx, sy, sz, n_bins, W, T, first_fold, grid_x, grid_y
//        (grid 0 = the engine's); double spacing, k; Real fields[T][mesh_nz][mesh_ny][pitch]
//   OUT: double bins[4][n_bins][B]; double velocity[3][B]
#include <hip/hip_runtime.h>

static thread_local wv_stub_dim3 gridDim;  // (the stub has the two indices only)

#include "intensity_kernels.hip.h"

#include <algorithm>
#include <cstdio>
#include <vector>

template <typename Real>
static int run(FILE* f, const uint64_t* h, double spacing, double k, const char* out_path) {
    const uint64_t mesh_ny = h[1], mesh_nz = h[2], pitch = h[3], n_bins = h[13], W = h[14], T = h[15], first_fold = h[16];
    const int32_t nx = (int32_t)h[7], ny = (int32_t)h[8], nz = (int32_t)h[9];
    const uint64_t nodes = (uint64_t)nx * ny * nz, field_elems = mesh_nz * mesh_ny * pitch;
    std::vector<Real> fields(T * field_elems);
    if (std::fread(fields.data(), sizeof(Real), fields.size(), f) != fields.size()) return 2;
    std::vector<float> stage((size_t)wv::kIntensityStage * 4 * nodes, 0.0f);
    std::vector<double> velocity(3 * nodes, 0.0), bins(4 * n_bins * nodes, 0.0);
    const uint64_t items = (uint64_t)nx * ny;
    const unsigned gx = h[17] ? (unsigned)h[17] : (unsigned)std::min<uint64_t>((items + 255) / 256, 1u << 14);
    const unsigned gy = h[18] ? (unsigned)h[18] : (unsigned)std::min(nz, 1024);
    uint64_t folded = 0;
    int staged = 0;
    for (uint64_t j = 0; j < T; ++j) {
        wv::IntensityGatherArgs<Real> a{};
        a.field = fields.data() + j * field_elems;
        a.dst = stage.data() + (size_t)staged * 4 * nodes;
        a.pitch = (int64_t)pitch;
        a.nodes = (int64_t)nodes;
        a.mesh_ny = (int32_t)mesh_ny;
        a.x0 = (int32_t)h[4], a.y0 = (int32_t)h[5], a.z0 = (int32_t)h[6];
        a.nx = nx, a.ny = ny, a.nz = nz;
        a.sx = (int32_t)h[10], a.sy = (int32_t)h[11], a.sz = (int32_t)h[12];
        a.spacing = spacing;
        gridDim = {gx, gy, 1};
        for (unsigned by = 0; by < gy; ++by)
            for (unsigned bx = 0; bx < gx; ++bx)
                for (unsigned tx = 0; tx < 256; ++tx) {
                    blockIdx = {bx, by, 0};
                    threadIdx = {tx, 0, 0};
                    wv::intensity_gather_kernel<Real>(a);
                }
        ++staged;
        // (the first fold may be short, as one cut by a fetch mid-run is)
        const int due = (int)(folded == 0 ? std::min<uint64_t>(first_fold, wv::kIntensityStage) : (uint64_t)wv::kIntensityStage);
        if (staged == due || j + 1 == T) {
            int32_t bin[wv::kIntensityStage];
            for (int s = 0; s < staged; ++s) bin[s] = (int32_t)wv::decay_bin(folded + s, (uint32_t)W, (uint32_t)n_bins);
            gridDim = {(unsigned)((nodes + 255) / 256), 1, 1};
            for (unsigned bx = 0; bx < gridDim.x; ++bx)
                for (unsigned tx = 0; tx < 256; ++tx) {
                    blockIdx = {bx, 0, 0};
                    threadIdx = {tx, 0, 0};
                    wv::intensity_fold_kernel(stage.data(), velocity.data(), bins.data(), bin, nodes, (uint32_t)n_bins, k, staged);
                }
            folded += staged;
            staged = 0;
        }
    }
    FILE* o = std::fopen(out_path, "wb");
    if (!o) return 2;
    std::fwrite(bins.data(), 8, bins.size(), o);
    std::fwrite(velocity.data(), 8, velocity.size(), o);
    std::fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t h[19];
    double d[2];
    if (std::fread(h, 8, 19, f) != 19 || std::fread(d, 8, 2, f) != 2) return 2;
    const int rc = h[0] == 4 ? run<float>(f, h, d[0], d[1], argv[2]) : h[0] == 8 ? run<double>(f, h, d[0], d[1], argv[2]) : 2;
    std::fclose(f);
    return rc;
}

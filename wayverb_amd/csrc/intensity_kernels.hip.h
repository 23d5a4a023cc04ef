// intensity_kernels.hip.h -- the two kernels of intensity maps (wv_set_intensity; engine_intensity.hip.h launches them): the sound
// intensity I = p v of postprocessor::directional_receiver (src/waveguide/src/postprocessor/directional_receiver.cpp:29-69) at every
// node of a box, summed into time bins on the device.
//
// intensity_gather_kernel<Real> is the capture.  Per node taken it reads the centre and its six neighbours from the stored
// (row-padded) field -- node (x, y, z) at (z * ny + y) * pitch + x -- and evaluates directional_accumulate_kernel's float lines
// (receiver_kernels.hip.h:58-64, the same casts, the same association):
//
//     pressure       = (float)field[c]
//     surrounding[i] = (float)((double)((float)field[n_i] - pressure) / spacing)       i = 0 .. 5: ports nx, px, ny, py, nz, pz
//     gx = surrounding[1] - surrounding[0]                                             (gy, gz likewise)
//
// and writes four dense float planes stage[slot][4][B]: pressure, gx, gy, gz -- 16 bytes per node and capture where the seven raw
// floats would be 28.  Lanes run along x of the dense box with snapshot_gather_kernel's index arithmetic (grid x over a dense plane,
// grid y over the planes); the +-y / +-z neighbours are the same lanes one stored row / plane away, the +-x neighbours lie in the
// lines the row touches anyway.  No LDS, no scratch, no branch on data.  The engine refuses a box with a node on the mesh's faces
// (intensity_plan.h), so every neighbour is a stored node.
//
// intensity_fold_kernel folds the first t staged captures, in order, into the velocities double[3][B] and the bins
// double[4][n_bins][B] (Ix, Iy, Iz, E):
//
//     m  = (double)g * 0.5
//     v  = v - m / k                              k = ambient_density * sample_rate: an IEEE division, never a multiplication by 1 / k
//     I[a][bin[j]] = I[a][bin[j]] + v[a] * (double)pressure                            (the product is rounded, then the sum)
//     E[bin[j]]    = E[bin[j]]    + (double)pressure * (double)pressure
//
// with decay_fold_kernel's scheme (decay_kernels.hip.h): the host writes int32 bin[t], non-decreasing, reached through a __restrict__
// argument with indices that depend on the unrolled loop counter only, so every branch on it is wave-uniform; lanes run along the
// dense node index; a lane holds FOUR accumulators and stores / reloads them only where bin[j] changes.  All planes are planar, so
// every access of a wave is contiguous.  No LDS, no atomics, no scratch.  The library is built with -ffp-contract=off.
//
// Traffic model: B * (16 t + 48 + 64 r) bytes per fold, r the number of distinct bins among the t captures.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fold_parts.hip.h"
#include "intensity_plan.h"

namespace wv {

template <typename Real>
struct IntensityGatherArgs {
    const Real* field;    // the stored field that holds the step
    float* dst;           // [4][nz][ny][nx] dense: pressure, gx, gy, gz
    int64_t pitch;        // elements per stored row
    int64_t nodes;        // B: floats per plane of dst
    int32_t mesh_ny;      // rows per stored plane
    int32_t x0, y0, z0;
    int32_t nx, ny, nz;   // nodes taken
    int32_t sx, sy, sz;
    double spacing;       // mesh_descriptor::spacing
};

template <typename Real>
__global__ void __launch_bounds__(256) intensity_gather_kernel(const IntensityGatherArgs<Real> a) {
    // x of the grid strides over the nodes of one dense plane (32-bit arithmetic, one division), y over the planes
    const uint32_t per_row = (uint32_t)a.nx;
    const uint32_t n = per_row * (uint32_t)a.ny;
    const int64_t plane_floats = (int64_t)a.nx * a.ny;
    const int64_t row = a.pitch, slab = a.pitch * a.mesh_ny;  // a stored row / plane away
    for (int32_t zz = (int32_t)blockIdx.y; zz < a.nz; zz += (int32_t)gridDim.y) {
        const Real* plane = a.field + ((int64_t)(a.z0 + (int64_t)zz * a.sz) * a.mesh_ny + a.y0) * a.pitch + a.x0;
        float* out = a.dst + (int64_t)zz * plane_floats;
        for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
            const uint32_t yy = i / per_row;
            const uint32_t c = i - yy * per_row;
            const Real* src = plane + (int64_t)yy * a.sy * a.pitch + (int64_t)c * a.sx;
            const float pressure = (float)src[0];
            const float port[6] = {(float)src[-1], (float)src[1], (float)src[-row], (float)src[row], (float)src[-slab], (float)src[slab]};
            float surrounding[6];
#pragma unroll
            for (int p = 0; p < 6; ++p) surrounding[p] = (float)((double)(port[p] - pressure) / a.spacing);
            out[i] = pressure;
            out[a.nodes + i] = surrounding[1] - surrounding[0];
            out[2 * a.nodes + i] = surrounding[3] - surrounding[2];
            out[3 * a.nodes + i] = surrounding[5] - surrounding[4];
        }
    }
}

// stage [T][4][B]: the first t slots hold captures; velocity [3][B]; bins [4][n_bins][B]; bin [t]: the bin of staged capture j, each
// inside 0 .. n_bins - 1; nodes = B; t = staged captures to fold, 1 .. kIntensityStage.  (Separate __restrict__ kernel arguments, not
// members of a struct: the stores must be known not to touch the table, or its loads cannot go through the scalar path.)
__global__ void __launch_bounds__(256) intensity_fold_kernel(const float* __restrict__ stage, double* __restrict__ velocity, double* __restrict__ bins,
                                                             const int32_t* __restrict__ bin, const uint64_t nodes, const uint32_t n_bins, const double k,
                                                             const int32_t t) {
    const uint64_t node = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (node >= nodes || t < 1) return;
    double v[3], e[4];
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] = velocity[(uint64_t)a * nodes + node];
    auto load = [&](int32_t b) {
#pragma unroll
        for (int a = 0; a < 4; ++a) e[a] = bins[((uint64_t)a * n_bins + (uint64_t)b) * nodes + node];
    };
    auto store = [&](int32_t b) {
#pragma unroll
        for (int a = 0; a < 4; ++a) bins[((uint64_t)a * n_bins + (uint64_t)b) * nodes + node] = e[a];
    };
    int32_t held = bin[0];
    load(held);
#pragma unroll
    for (int j = 0; j < kIntensityStage; ++j) {
        if (j < t) {
            const float* src = stage + (uint64_t)j * 4u * nodes + node;
            const float pressure = src[0];
            const float g[3] = {src[nodes], src[2 * nodes], src[3 * nodes]};
            const int32_t b = bin[j];  // (no lane in it)
            if (b != held) {
                store(held);
                held = b;
                load(held);
            }
            const double p = (double)pressure;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                v[a] = integrate(v[a], g[a], k);
                e[a] = e[a] + v[a] * p;
            }
            e[3] = e[3] + p * p;
        }
    }
    store(held);
#pragma unroll
    for (int a = 0; a < 3; ++a) velocity[(uint64_t)a * nodes + node] = v[a];
}

}  // namespace wv

// compressed_kernels.hip.h -- one step of the free-field waveguide folded onto 1/48 of space, the generator of the mesh's
// own impulse response that transparent sources subtract (compensation_signal.hip).
//
// Replaces the reference's `compressed_waveguide` kernel (src/waveguide/compensation_signal/lib/src/waveguide.cpp:23-114):
// node (x, y, z) with x >= y >= z >= 0 lives at tetrahedron(x) + triangle(y) + z, a neighbour outside the wedge is brought
// back into it by `fold_locator` (|.|, then three conditional swaps), and every updated node becomes
//     float( double(nx + px + ny + py + nz + pz) / 3.0 - double(prev) )
// with the six float additions in that direction order whatever node a fold lands on.
//
// Launch shape: the nodes of shells x <= r form the contiguous range [0, tetrahedron(r + 1)); lanes take consecutive indices
// of it (grid-stride), decode (x, y, z) in closed form (integer-corrected cube and square roots, not the reference's O(x)
// walk) and read their neighbours at plain offsets inside the wedge (+-1, +(y+1) / -y, +triangle(x+1) / -triangle(x)).
// Only nodes on a face of the wedge (x == y, y == z or z == 0) take `fold_locator`.  Node indices are 64-bit: the
// reference's int tetrahedron() overflows its product from x ~ 1290, node counts pass 2^31 at ~4700 taps.
//
// The source sample is injected inside the same launch: lanes 0 and 1 -- node 0 and the one node that reads node 0, (1,0,0)
// -- form the injected value v from the SAME load of cur[0] (hard: input[k]; soft: cur[0] + input[k]); node 1 uses v where
// it would read cur[0], node 0's lane stores v into cur[0] (where the next step reads it back as its `prev`, as the
// reference's write_value before the kernel leaves it) and records its own new value as the step's output.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hip.h"

namespace wv {

// Coordinates stay below 2^15 (wv_compressed_waveguide_run refuses more than 2^16 steps), so triangle() fits 32 bits;
// tetrahedron() and node indices are 64-bit.
__host__ __device__ inline int32_t cw_triangle(int32_t i) { return i * (i + 1) / 2; }
__host__ __device__ inline int64_t cw_tetrahedron(int64_t i) { return i * (i + 1) * (i + 2) / 6; }

// fold_locator + to_index (waveguide.cpp:56-77): `plane` is taken from |x| before any swap, as there
__device__ inline int64_t cw_fold_index(int32_t x, int32_t y, int32_t z) {
    x = x < 0 ? -x : x;
    y = y < 0 ? -y : y;
    z = z < 0 ? -z : z;
    const int32_t plane = x + 1;
    int32_t t;
    if (plane <= y) { t = x; x = y; y = t; }
    if (plane <= z) { t = x; x = z; z = t; }
    if (y < z) { t = y; y = z; z = t; }
    return cw_tetrahedron(x) + cw_triangle(y) + z;
}

struct CompressedArgs {
    float* prev;          // field at t-1, overwritten with the new values
    float* cur;           // field at t; node 0 receives the injected sample
    const float* input;   // [2 * dim] source samples, zero-padded past the caller's signal
    float* output;        // [2 * dim] node 0 after each step
    int64_t step;         // k
    int64_t nodes;        // nodes updated this step: tetrahedron(r + 1), r the step's largest shell
    int32_t soft;         // 1: soft source (cur[0] += input[k]); 0: hard (cur[0] = input[k])
};

__global__ void __launch_bounds__(256) compressed_waveguide_kernel(CompressedArgs a) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.nodes; i += stride) {
        // x: tetrahedron(x) <= i < tetrahedron(x + 1), from a single-precision cube root (cbrt(6 i) lies in (x, x + 2))
        // corrected by exact integer steps (tetrahedron(x + 1) = tetrahedron(x) + triangle(x + 1)): the guess only
        // decides how many steps are taken, never the result
        int32_t x = (int32_t)cbrtf(6.0f * (float)i);
        int64_t tx = cw_tetrahedron(x);
        while (tx > i) tx -= cw_triangle(x--);
        while (tx + cw_triangle(x + 1) <= i) tx += cw_triangle(++x);
        // y: triangle(y) <= r < triangle(y + 1) inside slice x, the same way from a square root
        const int32_t r = (int32_t)(i - tx);
        int32_t y = (int32_t)((sqrtf(8.0f * (float)r + 1.0f) - 1.0f) * 0.5f);
        int32_t ty = cw_triangle(y);
        while (ty > r) ty -= y--;
        while (ty + y + 1 <= r) ty += ++y;
        const int32_t z = r - ty;

        float v = 0.0f;  // the injected value, for lanes 0 and 1 only (one load of cur[0] for both)
        if (i <= 1) {
            v = a.input[a.step];
            if (a.soft) v = a.cur[0] + v;
        }
        float nx, px, ny, py, nz, pz;
        if (x > y && y > z && z > 0) {  // inside the wedge: no neighbour folds
            nx = a.cur[i - cw_triangle(x)];
            px = a.cur[i + cw_triangle(x + 1)];
            ny = a.cur[i - y];
            py = a.cur[i + y + 1];
            nz = a.cur[i - 1];
            pz = a.cur[i + 1];
        } else {
            const int64_t j[6] = {cw_fold_index(x - 1, y, z), cw_fold_index(x + 1, y, z), cw_fold_index(x, y - 1, z),
                                  cw_fold_index(x, y + 1, z), cw_fold_index(x, y, z - 1), cw_fold_index(x, y, z + 1)};
            float c[6];
#pragma unroll
            for (int d = 0; d < 6; ++d) c[d] = j[d] == 0 ? v : a.cur[j[d]];  // only (1,0,0) has node 0 as a neighbour
            nx = c[0], px = c[1], ny = c[2], py = c[3], nz = c[4], pz = c[5];
        }
        const float s = ((((nx + px) + ny) + py) + nz) + pz;
        const float n = (float)(div3((double)s) - (double)a.prev[i]);
        a.prev[i] = n;
        if (i == 0) {
            a.cur[0] = v;
            a.output[a.step] = n;
        }
    }
}

}  // namespace wv

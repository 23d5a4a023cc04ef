// receiver_kernels.hip.h -- receiver arrays: the receiver gather of a step spread over the chip, and the directional receivers'
// integrator (postprocessor::directional_receiver, src/waveguide/src/postprocessor/directional_receiver.cpp:29-67) on the device.
//
// pre_post_kernel (boundary_kernels.hip.h) serves a step's receivers with ONE wave: right for the reference's census of a dozen
// columns, 110 dependent round trips of that wave for a thousand receivers of seven columns each.  Above 64 columns
// Engine::launch_pre_post puts receiver_gather_kernel in front of it and leaves it the flag words, the source store and the fix-up list.
#pragma once
#include "device_common.hip.h"

namespace wv {

// One lane per column: recv_out[r] = what pre_post_body records for column r.  Launched BEFORE the launch that stores the source
// sample, so cur[source_node] still holds the value the loop's `pre` finds there; the sample a receiver on the source node records is
// formed here, per lane, by pre_post_body's own expression.  Reads the field, writes the step's row: never the field, never a flag word.
// One scattered 4- or 8-byte load per lane: bound by the latency of a cache line, not by bytes.  No LDS, no atomics.
template <typename Real>
__global__ void __launch_bounds__(256) receiver_gather_kernel(const PrePostArgs<Real> a) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.n_recv) return;
    Real injected = 0;
    const bool has_source = a.source_kind != 0;
    if (has_source) {
        const Real s = (Real)a.signal[a.signal_pos + (a.signal_base ? *a.signal_base : 0ull)];
        injected = (a.source_kind == 1) ? s : (Real)(a.cur[a.source_node] + s);
    }
    const uint64_t node = a.recv[r];
    Real v = 0;
    if (node != ~0ull) v = (has_source && node == a.source_node) ? injected : a.cur[node];
    a.recv_out[r] = v;
}

// wv_directional_output as the device writes it: one 16-byte store per record
struct alignas(16) DirectionalRecord {
    float ix, iy, iz, pressure;
};

template <typename Real>
struct DirectionalArgs {
    const Real* rows;         // [n_rows][7 * n]: per receiver the centre, then ports nx, px, ny, py, nz, pz
    uint32_t n_rows, n;       // steps of the batch, receivers
    double spacing;           // mesh_descriptor::spacing
    double k;                 // ambient_density * sample_rate
    double* velocity;         // [n][3], carried from batch to batch
    DirectionalRecord* out;   // [n_rows][n]
};

// One lane per receiver, the batch's rows in step order: directional_receiver::accumulate of include/wayverb_amd/waveguide.h, operation
// for operation (seven values cast to float, float differences, a double division by the spacing rounded to float, a float difference
// promoted to double and halved, the velocity a double).  The library is built with -ffp-contract=off and IEEE division.
template <typename Real>
__global__ void __launch_bounds__(64) directional_accumulate_kernel(const DirectionalArgs<Real> a) {
    const uint32_t r = blockIdx.x * 64u + threadIdx.x;
    if (r >= a.n) return;
    double vx = a.velocity[3 * (size_t)r], vy = a.velocity[3 * (size_t)r + 1], vz = a.velocity[3 * (size_t)r + 2];
    const size_t width = 7 * (size_t)a.n;
    for (uint32_t row = 0; row < a.n_rows; ++row) {
        const Real* p7 = a.rows + (size_t)row * width + 7 * (size_t)r;
        const float pressure = (float)p7[0];
        float surrounding[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) surrounding[i] = (float)((double)((float)p7[1 + i] - pressure) / a.spacing);
        const double mx = (double)(surrounding[1] - surrounding[0]) * 0.5;
        const double my = (double)(surrounding[3] - surrounding[2]) * 0.5;
        const double mz = (double)(surrounding[5] - surrounding[4]) * 0.5;
        vx -= mx / a.k;
        vy -= my / a.k;
        vz -= mz / a.k;
        const double p = (double)pressure;
        a.out[(size_t)row * a.n + r] = DirectionalRecord{(float)(vx * p), (float)(vy * p), (float)(vz * p), pressure};
    }
    a.velocity[3 * (size_t)r] = vx;
    a.velocity[3 * (size_t)r + 1] = vy;
    a.velocity[3 * (size_t)r + 2] = vz;
}

}  // namespace wv

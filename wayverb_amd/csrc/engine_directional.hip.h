// engine_directional.hip.h -- receiver arrays: R directional receivers (postprocessor::directional_receiver,
// src/waveguide/src/postprocessor/directional_receiver.cpp:10-69) recorded and integrated on the device.
//
// The reference runs its whole mesh once per source-receiver pair (src/combined/src/threaded_engine.cpp:155-162) although a run costs
// the same however many points listen.  Here the 7 * R columns are recorded as any columns are (above 64 of them by the wide gather,
// receiver_kernels.hip.h), the integrator runs over a batch's rows at the end of the batch, one lane per receiver, and the 16-byte
// records come to the host where the 56 bytes of raw columns would have.
//
// Part of the engine behind the C ABI of include/wayverb_amd.h (engine.hip is the translation unit; see engine.hip.h for
// the class and the map of which file holds what).
#pragma once
#include "engine.hip.h"

namespace wv {

static_assert(sizeof(wv_directional_output) == sizeof(DirectionalRecord) && sizeof(DirectionalRecord) == 16,
              "the device writes wv_directional_output as one 16-byte record");

template <typename Real>
void Engine<Real>::directional_release() {
    if (dir_.velocity) (void)hipFree(dir_.velocity);
    if (dir_.dev) (void)hipFree(dir_.dev);
    if (dir_.host) (void)hipHostFree(dir_.host);
    const uint64_t generation = dir_.generation + (dir_.active ? 1 : 0), launches = dir_.launches;
    dir_ = Directional{};
    dir_.generation = generation;
    dir_.launches = launches;
}

template <typename Real>
int Engine<Real>::set_directional_receivers(const uint64_t* nodes, uint32_t n, double spacing, double sample_rate, double ambient_density) {
    DeviceGuard guard(device_);
    if (!nodes || !n) return set_receivers(nullptr, 0);  // leaves the mode
    // A receiver next to a cut has a neighbour in a ghost plane, and nothing pins the reading of ghost planes by receivers in every form
    // of pass: chains record columns and integrate them on the host (wv_directional_accumulate).
    if (opt_.ghost_lo || opt_.ghost_hi || (comm_ && comm_->nranks() > 1)) return fail(WV_E_STATE, kDirectionalOnSlab);
    if (!(spacing > 0) || !(sample_rate > 0) || !(ambient_density > 0))
        return fail(WV_E_INVALID_ARGUMENT, "wv_set_directional_receivers: spacing, sample rate and ambient density must be positive");
    if ((uint64_t)n * 7 > 0xFFFFFFFFull) return fail(WV_E_INVALID_ARGUMENT, "wv_set_directional_receivers: too many receivers");
    // the columns: per receiver the centre, then compute_neighbors' ports (nx, px, ny, py, nz, pz)
    std::vector<uint64_t> cols((size_t)n * 7);
    const uint64_t row = (uint64_t)nx_, plane = (uint64_t)nx_ * (uint64_t)ny_;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t c = nodes[i];
        if (c >= n_nodes_) return fail(WV_E_INVALID_ARGUMENT, "receiver node outside the mesh");
        const uint64_t x = c % row, y = (c / row) % (uint64_t)ny_, z = c / plane;
        if (x == 0 || x + 1 >= (uint64_t)nx_ || y == 0 || y + 1 >= (uint64_t)ny_ || z == 0 || z + 1 >= (uint64_t)nz_)
            return fail(WV_E_INVALID_ARGUMENT, "Can't place directional_receiver at this node as it is adjacent to a boundary.");
        uint64_t* o = cols.data() + (size_t)i * 7;
        o[0] = c;
        o[1] = c - 1;
        o[2] = c + 1;
        o[3] = c - row;
        o[4] = c + row;
        o[5] = c - plane;
        o[6] = c + plane;
    }
    // everything is allocated before the engine's state changes (set_columns does the same with the columns' buffers)
    ScopedDevice velocity, dev;
    wv_directional_output* host = nullptr;
    WV_HIP(hipMalloc(&velocity.p, (size_t)n * 3 * sizeof(double)));
    WV_HIP(hipMalloc(&dev.p, (size_t)kRing * n * sizeof(DirectionalRecord)));
    WV_HIP(hipHostMalloc((void**)&host, (size_t)kRing * n * sizeof(wv_directional_output), hipHostMallocDefault));
    int rc = WV_OK;
    if (hipMemsetAsync(velocity.p, 0, (size_t)n * 3 * sizeof(double), stream_) != hipSuccess ||
        hipStreamSynchronize(stream_) != hipSuccess) {
        note_hip_error(hipGetLastError());
        rc = fail(WV_E_HIP, "wv_set_directional_receivers: zeroing the velocities failed");
    }
    if (rc == WV_OK) rc = set_columns(cols.data(), (uint32_t)cols.size());
    if (rc != WV_OK) {
        (void)hipHostFree(host);
        return rc;
    }
    directional_release();
    dir_.active = true;
    dir_.n = n;
    dir_.spacing = spacing;
    dir_.k = ambient_density * sample_rate;
    dir_.velocity = static_cast<double*>(velocity.p);
    dir_.dev = static_cast<DirectionalRecord*>(dev.p);
    dir_.host = host;
    velocity.p = dev.p = nullptr;
    ++dir_.generation;
    return WV_OK;
}

// The integrator over rows [0, batch) of the receiver ring, then the records to the page-locked twin: enqueued by collect_batch where
// the raw rows would have been copied.
template <typename Real>
int Engine<Real>::directional_enqueue(uint64_t batch) {
    if (!batch) return WV_OK;
    wv::DirectionalArgs<Real> a{};
    a.rows = recv_out_;
    a.n_rows = (uint32_t)batch;
    a.n = dir_.n;
    a.spacing = dir_.spacing;
    a.k = dir_.k;
    a.velocity = dir_.velocity;
    a.out = dir_.dev;
    hipLaunchKernelGGL(wv::directional_accumulate_kernel<Real>, dim3((dir_.n + 63u) / 64u), dim3(64), 0, stream_, a);
    WV_HIP(hipGetLastError());
    ++dir_.launches;
    WV_HIP(hipMemcpyAsync(dir_.host, dir_.dev, (size_t)batch * dir_.n * sizeof(DirectionalRecord), hipMemcpyDeviceToHost, stream_));
    return WV_OK;
}

template <typename Real>
int Engine<Real>::fetch_directional(uint64_t first, uint64_t n, wv_directional_output* dst) {
    if (!dir_.active) return fail(WV_E_STATE, "wv_fetch_directional: no directional receivers are set (wv_set_directional_receivers)");
    if (first < recv_first_step_) return fail(WV_E_INVALID_ARGUMENT, "steps before wv_set_directional_receivers are not recorded");
    const uint64_t off = first - recv_first_step_;
    if ((off + n) * dir_.n > dir_.log.size()) return fail(WV_E_INVALID_ARGUMENT, "steps not recorded yet");
    if (n && !dst) return fail(WV_E_INVALID_ARGUMENT, "null argument");
    if (n) std::memcpy(dst, dir_.log.data() + off * dir_.n, (size_t)n * dir_.n * sizeof(wv_directional_output));
    return WV_OK;
}

// The integrator's carried state as it lies, [n][3]: what the records of the completed steps left behind.
template <typename Real>
int Engine<Real>::fetch_directional_velocity(double* dst) {
    DeviceGuard guard(device_);
    if (!dir_.active) return fail(WV_E_STATE, "wv_fetch_directional_velocity: no directional receivers are set (wv_set_directional_receivers)");
    if (!dst) return fail(WV_E_INVALID_ARGUMENT, "null argument");
    WV_HIP(hipStreamSynchronize(stream_));
    WV_HIP(hipMemcpy(dst, dir_.velocity, (size_t)dir_.n * 3 * sizeof(double), hipMemcpyDeviceToHost));
    return WV_OK;
}

}  // namespace wv

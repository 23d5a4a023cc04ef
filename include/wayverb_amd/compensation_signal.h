// wayverb_amd/compensation_signal.h -- C++14 mirror of wayverb's transparent sources over the C ABI of wayverb_amd.h.
// Header only; link against libwayverb_amd.so.
//
// Same names and argument meaning as the reference (paths relative to the reference repository root):
//   waveguide::compressed_rectangular_waveguide   src/waveguide/compensation_signal/lib/include/compensation_signal/
//                                                 waveguide.h:42-131 (run_hard_source, run_soft_source)
//   waveguide::make_transparent                   src/waveguide/include/waveguide/make_transparent.h,
//                                                 src/waveguide/src/make_transparent.cpp:10-30
//
// What differs, deliberately:
//   - the reference compiles its 512-tap mesh impulse response in (mesh_impulse_response.h, written at build time by
//     `write_compensation_signal 512`); here make_transparent generates it on the device at its first call and keeps it for
//     the process, so make_transparent needs a GPU and throws engine_error without one.  make_transparent(begin, end, taps)
//     takes a table of another length.
//   - the waveguide runs all its steps on the device in one call (wv_compressed_waveguide_run); `per_step(count)` is fired
//     for every step, in order, once the run is over (the reference fires it as it goes, for a progress bar).
//   - the results are std::vector<float>, not util::aligned::vector<float>.
#pragma once

#include <cstddef>
#include <cstdint>
#include <iterator>
#include <map>
#include <mutex>
#include <vector>

#include "../wayverb_amd.h"
#include "waveguide.h"

namespace wayverb {
namespace waveguide {

class compressed_rectangular_waveguide final {
public:
    /// `cc` names the HIP device as `run` reads it (its `.device`, or the calling thread's current one)
    template <typename Context>
    compressed_rectangular_waveguide(const Context& cc, size_t steps)
            : device_{detail::device_of(cc)}
            , steps_{steps} {}

    template <typename It, typename T>
    std::vector<float> run_hard_source(It begin, It end, const T& per_step) {
        return run(WV_SOURCE_HARD, begin, end, per_step);
    }

    template <typename It, typename T>
    std::vector<float> run_soft_source(It begin, It end, const T& per_step) {
        return run(WV_SOURCE_SOFT, begin, end, per_step);
    }

private:
    template <typename It, typename T>
    std::vector<float> run(int kind, It begin, It end, const T& per_step) {
        const size_t n = 2 * ((steps_ + 1) / 2);
        std::vector<float> input;
        for (; begin != end && input.size() != n; ++begin) input.push_back(static_cast<float>(*begin));  // (the rest is never read)
        std::vector<float> ret(n);
        detail::check(wv_compressed_waveguide_run(device_, steps_, kind, input.data(), input.size(), ret.data()));
        for (size_t count = 0; count != n; ++count) per_step(count);
        return ret;
    }

    int device_;
    size_t steps_;
};

namespace detail {
struct hip_device final {  // a context naming the calling thread's current device (device_of reads `.device`)
    int device;
};

/// The mesh's impulse response of `taps` taps on the calling thread's current device, made once per process.
inline const std::vector<float>& mesh_impulse_response(size_t taps) {
    static std::mutex mutex;
    static std::map<size_t, std::vector<float>> tables;
    std::lock_guard<std::mutex> lock{mutex};
    auto it = tables.find(taps);
    if (it == tables.end()) {
        const std::vector<float> sig{0.0f, 1.0f};  // compensation_signal/cmd/main.cpp:48-53
        auto out = compressed_rectangular_waveguide{hip_device{-1}, taps}.run_hard_source(sig.begin(), sig.end(),
                                                                                              [](size_t) {});
        out.resize(taps);
        it = tables.emplace(taps, std::move(out)).first;
    }
    return it->second;
}
}  // namespace detail

/// make_transparent.cpp:10-30 with a mesh impulse response of `taps` taps (the reference's table has 512)
inline std::vector<float> make_transparent(const float* begin, const float* end, size_t taps) {
    const auto& response = detail::mesh_impulse_response(taps);
    const auto n = static_cast<size_t>(std::distance(begin, end));
    std::vector<float> ret(n + taps - 1);
    detail::check(wv_make_transparent(begin, n, response.data(), static_cast<uint32_t>(taps), ret.data()));
    return ret;
}

inline std::vector<float> make_transparent(const float* begin, const float* end) { return make_transparent(begin, end, 512); }

}  // namespace waveguide
}  // namespace wayverb

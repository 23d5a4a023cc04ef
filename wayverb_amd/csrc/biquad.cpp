// biquad.cpp -- (host only, no HIP) the band filters of banded decay maps (wv_set_decay_bands, include/wayverb_amd.h): the cascade the
// fold kernel runs per node, restated for the host, and the two designs that supply its sections.
//
// Replaces:
//   biquad::filter, series_biquads<N>::filter, run_one_pass     src/core/include/core/filters_common.h:92-136, 173-199
//   compute_{hipass,lopass}_butterworth_coefficients<N>          filters_common.h:217-245, src/core/src/filters_common.cpp:93-122
//   compute_bandpass_biquad_coefficients                         filters_common.cpp:37-56
//
// Every expression keeps the reference's order of operations, one rounding per operation (the build's -ffp-contract=off), so the
// coefficients and the filtered series can be compared to the last bit (tests/golden/biquad_reference.npz holds the reference's).
// decay_bands_kernels.hip.h evaluates wv_biquad_step's three lines on the device; tests/cpp/decay_bands_test.cpp covers this file.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/wayverb_amd.h"

namespace wv {
int fail_with(int code, const std::string& msg);  // engine.hip
}

namespace {

constexpr double kPi = 3.14159265358979323846;  // M_PI

// transposed direct form II: the three statements of biquad::filter
inline double biquad_step(const wv_biquad& c, double x, double& z1, double& z2) {
    const double out = x * c.b0 + z1;
    z1 = x * c.b1 - c.a1 * out + z2;
    z2 = x * c.b2 - c.a2 * out;
    return out;
}

wv_biquad lopass_butterworth_segment(double cf, size_t order, size_t segment) {
    const double cf2 = cf * cf;
    const double p = 2 * cf * std::cos(kPi * (order + 2 * (segment + 1) - 1) / (2 * order));
    const double a0 = 1 - p + cf2;
    return {cf2 / a0, (2.0 * cf2) / a0, cf2 / a0, (2.0 * (cf2 - 1.0)) / a0, (cf2 + p + 1.0) / a0};
}

wv_biquad hipass_butterworth_segment(double cf, size_t order, size_t segment) {
    const double cf2 = cf * cf;
    const double cf3 = cf * cf2;
    const double p = 2 * cf2 * std::cos(kPi * (order + 2 * (segment + 1) - 1) / (2 * order));
    const double a0 = cf - p + cf3;
    return {cf / a0, (-2.0 * cf) / a0, cf / a0, (2.0 * (cf3 - cf)) / a0, (cf3 + p + cf) / a0};
}

bool band_ok(double lo, double hi, double sr) {
    return std::isfinite(lo) && std::isfinite(hi) && std::isfinite(sr) && lo > 0 && hi > lo && sr > 0 && hi < sr / 2;
}

}  // namespace

extern "C" {

int wv_biquad_run(const wv_biquad* sections, uint32_t n_sections, const double* in, uint64_t n, double* state, double* out) {
    if (!sections || n_sections < 1 || (n && (!in || !out))) return wv::fail_with(WV_E_INVALID_ARGUMENT, "wv_biquad_run: null argument or no sections");
    std::vector<double> own;
    if (!state) {
        own.assign((size_t)n_sections * 2, 0.0);
        state = own.data();
    }
    for (uint64_t i = 0; i < n; ++i) {
        double x = in[i];
        for (uint32_t s = 0; s < n_sections; ++s) x = biquad_step(sections[s], x, state[2 * s], state[2 * s + 1]);
        out[i] = x;
    }
    return WV_OK;
}

int wv_butterworth_bandpass(double lo_hz, double hi_hz, double sample_rate, wv_biquad out[4]) {
    if (!out) return wv::fail_with(WV_E_INVALID_ARGUMENT, "wv_butterworth_bandpass: null argument");
    if (!band_ok(lo_hz, hi_hz, sample_rate))
        return wv::fail_with(WV_E_INVALID_ARGUMENT, "wv_butterworth_bandpass: 0 < lo_hz < hi_hz < sample_rate / 2 is required");
    const double cl = std::tan(kPi * lo_hz / sample_rate), ch = std::tan(kPi * hi_hz / sample_rate);
    for (size_t i = 0; i < 2; ++i) out[i] = hipass_butterworth_segment(cl, 4, i);
    for (size_t i = 0; i < 2; ++i) out[2 + i] = lopass_butterworth_segment(ch, 4, i);
    return WV_OK;
}

int wv_bandpass_biquad(double lo_hz, double hi_hz, double sample_rate, wv_biquad* out) {
    if (!out) return wv::fail_with(WV_E_INVALID_ARGUMENT, "wv_bandpass_biquad: null argument");
    if (!band_ok(lo_hz, hi_hz, sample_rate))
        return wv::fail_with(WV_E_INVALID_ARGUMENT, "wv_bandpass_biquad: 0 < lo_hz < hi_hz < sample_rate / 2 is required");
    const double c = std::sqrt(lo_hz * hi_hz);
    const double omega = 2 * kPi * c / sample_rate;
    const double cs = std::cos(omega);
    const double sn = std::sin(omega);
    const double bandwidth = std::log2(hi_hz / lo_hz);
    const double Q = sn / (std::log(2) * bandwidth * omega);
    const double alpha = sn * std::sinh(1 / (2 * Q));
    const double a0 = 1 + alpha;
    const double nrm = 1 / a0;
    *out = {nrm * alpha, nrm * 0, nrm * -alpha, nrm * (-2 * cs), nrm * (1 - alpha)};
    return WV_OK;
}

}  // extern "C"

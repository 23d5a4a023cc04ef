// decay_bands_test.cpp -- (CPU, stand-alone) the host side of band-limited decay maps: wv_biquad_run, wv_butterworth_bandpass and
// wv_bandpass_biquad (wayverb_amd/csrc/biquad.cpp) against hand-derived cases, and the sizes / limits / traffic model decay_plan.h
// holds for a banded plan.  Build: g++ -std=c++17 -I include -I wayverb_amd/csrc tests/cpp/decay_bands_test.cpp
// wayverb_amd/csrc/biquad.cpp (tests/test_decay_bands_host.py does); it is also the program to run under -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "decay_plan.h"
#include "wayverb_amd.h"

namespace wv {
int fail_with(int code, const std::string&) { return code; }  // (engine.hip's keeps the message for wv_last_error)
}

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);        \
            ++failures;                                                  \
        }                                                                \
    } while (0)

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
}

// a small deterministic series with both signs and a wide range (no library random numbers: the same everywhere)
static std::vector<double> series(size_t n) {
    std::vector<double> x(n);
    uint64_t s = 0x9e3779b97f4a7c15ull;
    for (size_t i = 0; i < n; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        x[i] = ((double)(int64_t)(s >> 11) / (double)(1ull << 52) - 1.0) * std::exp(-(double)i / 40.0);
    }
    return x;
}

int main() {
    static_assert(sizeof(wv_biquad) == 40, "five doubles");
    // ---- wv_biquad_run
    const wv_biquad identity = {1, 0, 0, 0, 0};
    const std::vector<double> x = series(257);
    std::vector<double> y(x.size());
    CHECK(wv_biquad_run(&identity, 1, x.data(), x.size(), nullptr, y.data()) == WV_OK);
    CHECK(same_bits(x, y));
    {   // a FIR section: the impulse response is b0, b1, b2, then +0.0 for ever
        const wv_biquad fir = {0.5, -0.25, 0.125, 0, 0};
        const double imp[5] = {1, 0, 0, 0, 0};
        double out[5], st[2] = {0, 0};
        CHECK(wv_biquad_run(&fir, 1, imp, 5, st, out) == WV_OK);
        CHECK(out[0] == 0.5 && out[1] == -0.25 && out[2] == 0.125 && out[3] == 0 && out[4] == 0 && st[0] == 0 && st[1] == 0);
    }
    {   // one pole at 0.5 (a1 = -0.5): 1, 1/2, 1/4, ... exactly; z1 holds the next output
        const wv_biquad pole = {1, 0, 0, -0.5, 0};
        const double imp[6] = {1, 0, 0, 0, 0, 0};
        double out[6], st[2] = {0, 0};
        CHECK(wv_biquad_run(&pole, 1, imp, 6, st, out) == WV_OK);
        for (int i = 0; i < 6; ++i) CHECK(out[i] == std::ldexp(1.0, -i));
        CHECK(st[0] == std::ldexp(1.0, -6) && st[1] == 0);
    }
    {   // two sections in series == one after the other; the three statements by hand for the first two samples
        const wv_biquad a = {0.3, 0.2, -0.1, -0.4, 0.25}, b = {1.5, -0.75, 0.5, 0.125, -0.0625};
        const wv_biquad both[2] = {a, b};
        std::vector<double> ya(x.size()), yab(x.size()), y2(x.size());
        CHECK(wv_biquad_run(&a, 1, x.data(), x.size(), nullptr, ya.data()) == WV_OK);
        CHECK(wv_biquad_run(&b, 1, ya.data(), ya.size(), nullptr, yab.data()) == WV_OK);
        CHECK(wv_biquad_run(both, 2, x.data(), x.size(), nullptr, y2.data()) == WV_OK);
        CHECK(same_bits(yab, y2));
        const double o0 = x[0] * a.b0 + 0.0;
        const double z1 = (x[0] * a.b1 - a.a1 * o0) + 0.0;
        const double z2 = x[0] * a.b2 - a.a2 * o0;
        const double o1 = x[1] * a.b0 + z1;
        CHECK(ya[0] == o0 && ya[1] == o1);
        const double z1b = (x[1] * a.b1 - a.a1 * o1) + z2;
        CHECK(ya[2] == x[2] * a.b0 + z1b);
        // in two halves with the state carried == in one call, outputs and final state; in place == out of place
        for (size_t cut : {size_t(0), size_t(1), size_t(100), x.size()}) {
            std::vector<double> h(x.size());
            double st[4] = {0, 0, 0, 0}, whole[4] = {0, 0, 0, 0};
            CHECK(wv_biquad_run(both, 2, x.data(), cut, st, h.data()) == WV_OK);
            CHECK(wv_biquad_run(both, 2, x.data() + cut, x.size() - cut, st, h.data() + cut) == WV_OK);
            CHECK(wv_biquad_run(both, 2, x.data(), x.size(), whole, y.data()) == WV_OK);
            CHECK(same_bits(h, y2) && same_bits(y, y2) && std::memcmp(st, whole, sizeof st) == 0);
        }
        std::vector<double> inplace = x;
        CHECK(wv_biquad_run(both, 2, inplace.data(), inplace.size(), nullptr, inplace.data()) == WV_OK);
        CHECK(same_bits(inplace, y2));
    }
    CHECK(wv_biquad_run(nullptr, 1, x.data(), 1, nullptr, y.data()) == WV_E_INVALID_ARGUMENT);
    CHECK(wv_biquad_run(&identity, 0, x.data(), 1, nullptr, y.data()) == WV_E_INVALID_ARGUMENT);
    CHECK(wv_biquad_run(&identity, 1, nullptr, 1, nullptr, y.data()) == WV_E_INVALID_ARGUMENT);
    CHECK(wv_biquad_run(&identity, 1, x.data(), 1, nullptr, nullptr) == WV_E_INVALID_ARGUMENT);
    CHECK(wv_biquad_run(&identity, 1, nullptr, 0, nullptr, nullptr) == WV_OK);   // nothing to do

    // ---- the designs: what any correct Butterworth band-pass has
    const double rates[] = {1333.0, 4000.0, 12000.0};
    for (double sr : rates)
        for (double centre : {63.0, 125.0, 250.0}) {
            const double lo = centre / std::sqrt(2.0), hi = centre * std::sqrt(2.0);
            if (hi >= sr / 2) continue;
            wv_biquad s[4];
            CHECK(wv_butterworth_bandpass(lo, hi, sr, s) == WV_OK);
            for (int i = 0; i < 4; ++i) {
                CHECK(std::fabs(s[i].a2) < 1 && std::fabs(s[i].a1) < 1 + s[i].a2);   // poles inside the unit circle
                const double dc = (s[i].b0 + s[i].b1 + s[i].b2) / (1 + s[i].a1 + s[i].a2);
                const double ny = (s[i].b0 - s[i].b1 + s[i].b2) / (1 - s[i].a1 + s[i].a2);
                if (i < 2) {   // high-pass: nothing at DC (b1 = -2 b0 exactly), everything at Nyquist
                    CHECK(s[i].b0 + s[i].b1 + s[i].b2 == 0 && s[i].b0 == s[i].b2 && std::fabs(ny - 1) < 1e-9);
                } else {       // low-pass: the converse
                    CHECK(s[i].b0 - s[i].b1 + s[i].b2 == 0 && s[i].b0 == s[i].b2 && std::fabs(dc - 1) < 1e-9);
                }
            }
            // |H| of the cascade at the two edges: each side is 3 dB down at its own edge, the other side nearly flat there
            for (double f : {lo, hi}) {
                const double w = 2 * 3.14159265358979323846 * f / sr;
                double mag2 = 1;
                for (int i = 0; i < 4; ++i) {
                    const double nr = s[i].b0 + s[i].b1 * std::cos(w) + s[i].b2 * std::cos(2 * w), ni = -s[i].b1 * std::sin(w) - s[i].b2 * std::sin(2 * w);
                    const double dr = 1 + s[i].a1 * std::cos(w) + s[i].a2 * std::cos(2 * w), di = -s[i].a1 * std::sin(w) - s[i].a2 * std::sin(2 * w);
                    mag2 *= (nr * nr + ni * ni) / (dr * dr + di * di);
                }
                // 1/2 from the side whose edge it is, times 1 / (1 + (1/2)^8) at the least from the other (an octave away on the
                // analogue axis or further: the bilinear warp only stretches the distance)
                CHECK(mag2 <= 0.5 + 1e-9 && mag2 >= 0.5 / (1 + 1.0 / 256) - 1e-9);
            }
            wv_biquad bp;
            CHECK(wv_bandpass_biquad(lo, hi, sr, &bp) == WV_OK);
            CHECK(bp.b1 == 0 && bp.b2 == -bp.b0 && bp.b0 > 0 && std::fabs(bp.a2) < 1 && std::fabs(bp.a1) < 1 + bp.a2);
            {   // unit gain at the geometric centre
                const double w = 2 * 3.14159265358979323846 * std::sqrt(lo * hi) / sr;
                const double nr = bp.b0 + bp.b2 * std::cos(2 * w), ni = -bp.b2 * std::sin(2 * w);
                const double dr = 1 + bp.a1 * std::cos(w) + bp.a2 * std::cos(2 * w), di = -bp.a1 * std::sin(w) - bp.a2 * std::sin(2 * w);
                CHECK(std::fabs((nr * nr + ni * ni) / (dr * dr + di * di) - 1) < 1e-9);
            }
        }
    {
        wv_biquad s[4];
        const double nan = std::numeric_limits<double>::quiet_NaN();
        CHECK(wv_butterworth_bandpass(100, 100, 4000, s) == WV_E_INVALID_ARGUMENT);
        CHECK(wv_butterworth_bandpass(0, 100, 4000, s) == WV_E_INVALID_ARGUMENT);
        CHECK(wv_butterworth_bandpass(100, 2000, 4000, s) == WV_E_INVALID_ARGUMENT);
        CHECK(wv_butterworth_bandpass(nan, 200, 4000, s) == WV_E_INVALID_ARGUMENT);
        CHECK(wv_butterworth_bandpass(100, 200, 0, s) == WV_E_INVALID_ARGUMENT);
        CHECK(wv_butterworth_bandpass(100, 200, 4000, nullptr) == WV_E_INVALID_ARGUMENT);
        CHECK(wv_bandpass_biquad(200, 100, 4000, s) == WV_E_INVALID_ARGUMENT);
        CHECK(wv_bandpass_biquad(100, 200, 4000, nullptr) == WV_E_INVALID_ARGUMENT);
    }

    // ---- decay_plan.h: limits, sizes, traffic model
    CHECK(wv::decay_bands_valid(1, 1) && wv::decay_bands_valid(8, 4) && !wv::decay_bands_valid(0, 1) && !wv::decay_bands_valid(9, 1));
    CHECK(!wv::decay_bands_valid(1, 0) && !wv::decay_bands_valid(1, 5));
    CHECK(wv::decay_band_bins_bytes(630, 7, 3) == 630ull * 8 * 7 * 3);
    CHECK(wv::decay_band_state_bytes(630, 3, 4) == 630ull * 16 * 4 * 3);
    CHECK(wv::decay_band_state_bytes(1, 1, 1) == 16 && wv::decay_band_coef_bytes(8, 4) == 8 * 4 * 40);
    CHECK(wv::decay_band_bins_bytes(1ull << 60, 4096, 8) == wv::kDecayNoSize && wv::decay_band_state_bytes(1ull << 58, 8, 4) == wv::kDecayNoSize);
    CHECK(wv::decay_bands_fold_traffic(65536, 4, 4, 16, 2) == 65536ull * 4 * (64 + 128 + 32));
    CHECK(wv::decay_bands_fold_traffic(567, 1, 1, 1, 1) == 567ull * (4 + 32 + 16));
    CHECK(wv::decay_bands_fold_traffic(1ull << 62, 8, 4, 16, 16) == wv::kDecayNoSize);

    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("DECAY BANDS OK\n");
    return 0;
}

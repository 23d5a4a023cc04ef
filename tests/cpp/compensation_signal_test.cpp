// tests/cpp/compensation_signal_test.cpp -- the reference's tests of transparent sources, restated against the C++ mirror
// (include/wayverb_amd/compensation_signal.h):
//   verify_compensation_signal_compressed   src/waveguide/tests/verify_compensation_signal.cpp:35-48 (100 identical runs)
//   waveguide_init                          src/waveguide/tests/waveguide_init.cpp:19-64 (a transparent soft source
//                                           reproduces its input at the source node)
// Exit code 0 = all assertions held, 2 = an exception (without a GPU: engine_error "no HIP device").
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "wayverb_amd/compensation_signal.h"
#include "wayverb_amd/setup.h"
#include "wayverb_amd/waveguide.h"

using namespace wayverb::waveguide;
using namespace wayverb::core;

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("REQUIRE failed: %s (line %d)\n", #cond, __LINE__);  \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

static void verify_compensation_signal_compressed() {
    const std::vector<float> input{1, 2, 3, 4, 5, 4, 3, 2, 1};
    const auto transparent = make_transparent(input.data(), input.data() + input.size());
    REQUIRE(transparent.size() == input.size() + 511);

    const size_t steps = 100;
    compressed_rectangular_waveguide waveguide{compute_context{}, steps};
    size_t fired = 0;
    const auto proper_output = waveguide.run_soft_source(transparent.begin(), transparent.end(), [&](size_t step) {
        REQUIRE(step == fired);
        ++fired;
    });
    REQUIRE(proper_output.size() == steps && fired == steps);
    for (int i = 0; i != 100; ++i) {
        const auto output = waveguide.run_soft_source(transparent.begin(), transparent.end(), [](size_t) {});
        REQUIRE(output == proper_output);
    }
    // the node's pressure right after the injection of step k is output[k - 1] + transparent[k]: the input, then silence
    double worst_in = 0, worst_after = 0;
    for (size_t k = 0; k != steps; ++k) {
        const double p = (k ? proper_output[k - 1] : 0.0f) + transparent[k];
        if (k < input.size())
            worst_in = std::max(worst_in, std::fabs(p - input[k]));
        else
            worst_after = std::max(worst_after, std::fabs(p));
    }
    std::printf("verify_compensation_signal_compressed: |p - input| <= %.3g over the input, |p| <= %.3g after it\n", worst_in,
                worst_after);
    REQUIRE(worst_in <= 1e-4 && worst_after <= 1e-4);
}

static void waveguide_init() {
    const compute_context cc{};
    const double spacing = 0.04, speed_of_sound = 340.0;
    const int n = (int)std::lround(2.2 / spacing) + 1;  // the 2 m box with 0.1 m of padding
    const double absorption[8] = {0.001, 0.001, 0.001, 0.001, 0.001, 0.001, 0.001, 0.001};
    const auto wall = to_impedance_coefficients(
            compute_reflectance_filter_coefficients(absorption, 1.0 / config::time_step(speed_of_sound, spacing)));
    const auto model = make_box_mesh(n, n, n, (float)spacing, wall);
    const auto receiver_index = compute_index(model.get_descriptor(), ivec3{n / 2, n / 2, n / 2});

    const std::vector<float> input(20, 1);
    auto transparent = make_transparent(input.data(), input.data() + input.size());
    const size_t steps = 100;
    transparent.resize(steps, 0);

    for (int precision : {WV_PRECISION_F64, WV_PRECISION_F32}) {
        default_precision() = precision;
        auto prep = preprocessor::make_soft_source(receiver_index, transparent.begin(), transparent.end());
        callback_accumulator<postprocessor::node> receiver{receiver_index};
        run(cc, model, [&](auto& queue, auto& buffer, auto step) { return prep(queue, buffer, step); },
            [&](auto& queue, const auto& buffer, auto step) { receiver(queue, buffer, step); }, true);
        REQUIRE(receiver.get_output().size() == transparent.size());
        double worst = 0;
        for (size_t i = 0; i != input.size(); ++i)
            worst = std::max(worst, std::fabs((double)receiver.get_output()[i] - input[i]));
        std::printf("waveguide_init (%s): |output - input| <= %.3g over the first %zu steps\n",
                    precision == WV_PRECISION_F64 ? "f64" : "f32", worst, input.size());
        REQUIRE(worst <= 1e-4);
    }
}

int main() {
    try {
        verify_compensation_signal_compressed();
        waveguide_init();
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    std::puts("COMPENSATION SIGNAL OK");
    return 0;
}

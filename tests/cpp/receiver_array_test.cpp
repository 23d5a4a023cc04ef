// tests/cpp/receiver_array_test.cpp -- `canonical_many` of include/wayverb_amd/waveguide.h: four receivers out of ONE run of a 40^3 room
// (wv_set_directional_receivers: recorded and integrated on the device), each band bytewise equal to `canonical` for that receiver
// alone; the progress callback fires once per step, in order.  tests/test_cpp_receiver_arrays.py builds and runs this.
// Exit code 0 = all assertions held; 2 = no HIP device; 1 = anything else.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "wayverb_amd/setup.h"

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("REQUIRE failed: %s (line %d)\n", #cond, __LINE__);  \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

using namespace wayverb;

int main() {
    try {
        const core::compute_context cc{};
        const core::environment env{};
        const int n = 40;
        const float spacing = 0.05f;
        const auto mesh = waveguide::make_box_mesh(n, n, n, spacing, waveguide::to_flat_coefficients(0.1));
        const double sample_rate = waveguide::compute_sample_rate(mesh.get_descriptor(), env.speed_of_sound);
        const size_t steps = 90;
        const double t = ((double)steps - 0.5) / sample_rate;
        const waveguide::vec3 source{n / 2 * spacing, n / 2 * spacing, n / 2 * spacing};
        const std::vector<waveguide::vec3> receivers{
                {(n / 2 + 5) * spacing, n / 2 * spacing, n / 2 * spacing},   // five nodes from the source
                {n / 2 * spacing, n / 2 * spacing, n / 2 * spacing},         // the source node itself
                {2 * spacing, 3 * spacing, (n - 3) * spacing},               // one layer inside the walls
                {(n / 2) * spacing, (n / 2 + 1) * spacing, n / 2 * spacing}  // next to the source
        };
        const std::atomic_bool keep_going{true};
        const waveguide::single_band_parameters params{200.0, 0.6};

        std::vector<size_t> fired;
        const auto many = waveguide::canonical_many(cc, mesh, source, receivers, env, params, t, keep_going, [&](size_t step, size_t total) {
            REQUIRE(total == steps);
            fired.push_back(step);
        });
        REQUIRE(bool(many) && many->size() == receivers.size());
        REQUIRE(fired.size() == steps);
        for (size_t i = 0; i < steps; ++i) REQUIRE(fired[i] == i);
        REQUIRE(waveguide::last_run_stats().steps == steps && waveguide::last_run_stats().rollbacks == 0 &&
                waveguide::last_run_stats().checkpoints == 0);

        bool heard = false;
        for (size_t r = 0; r < receivers.size(); ++r) {
            const auto one = waveguide::canonical(cc, mesh, source, receivers[r], env, params, t, keep_going, [](size_t, size_t) {});
            REQUIRE(bool(one) && one->size() == 1);
            const auto& want = (*one)[0];
            const auto& got = (*many)[r];
            REQUIRE(got.band.sample_rate == want.band.sample_rate);
            REQUIRE(got.valid_hz.get_min() == want.valid_hz.get_min() && got.valid_hz.get_max() == want.valid_hz.get_max());
            REQUIRE(got.band.directional.size() == steps && want.band.directional.size() == steps);
            static_assert(sizeof(got.band.directional[0]) == 16, "records are four floats");
            REQUIRE(std::memcmp(got.band.directional.data(), want.band.directional.data(), steps * sizeof(got.band.directional[0])) == 0);
            for (const auto& d : got.band.directional)
                if (d.intensity.x != 0.0f || d.intensity.y != 0.0f || d.intensity.z != 0.0f) heard = true;
        }
        REQUIRE(heard);

        // cancelled: nothing
        const std::atomic_bool stop{false};
        REQUIRE(!waveguide::canonical_many(cc, mesh, source, receivers, env, params, t, stop, [](size_t, size_t) {}));
        // a receiver next to the mesh's edge: canonical's own error
        bool threw = false;
        try {
            std::vector<waveguide::vec3> bad = receivers;
            bad.push_back({0.0f, 5 * spacing, 5 * spacing});
            (void)waveguide::canonical_many(cc, mesh, source, bad, env, params, t, keep_going, [](size_t, size_t) {});
        } catch (const std::runtime_error& e) {
            threw = std::strstr(e.what(), "outside mesh") || std::strstr(e.what(), "adjacent to a boundary");
        }
        REQUIRE(threw);
        std::printf("%zu receivers, %zu steps, %zu batches\n", receivers.size(), steps, waveguide::last_run_stats().batches);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return std::strstr(e.what(), "no HIP device") ? 2 : 1;
    }
    std::puts("RECEIVER ARRAYS OK");
    return 0;
}

// interaural_plan_test.cpp -- (CPU, stand-alone) wayverb_amd/csrc/interaural_plan.h against hand-derived cases: every refusal alone, the
// ORDER of the refusals (every fault together with every later one answers with the earlier one's sentence), the ears on the mesh's
// faces, the bin of a capture (arrival_bin's rule), the lag class, sizes and places of the two blocks with their overflow answers, the
// ring of the history and the traffic model.  tests/test_interaural_host.py builds and runs it.
#include "interaural_plan.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <vector>

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static const int32_t NX = 24, NY = 20, NZ = 18;
static wv_biquad good[4] = {{1, 0, 0, 0, 0}, {0.5, 0.1, 0.2, -0.3, 0.4}, {1, 2, 3, 4, 5}, {1, 0, 0, 0, 0}};
static wv_biquad bad[4] = {{1, 0, 0, 0, 0}, {0.5, std::numeric_limits<double>::infinity(), 0.2, -0.3, 0.4}, {1, 2, 3, 4, 5}, {1, 0, 0, 0, 0}};

static wv_interaural_plan base() {
    wv_interaural_plan p;
    std::memset(&p, 0, sizeof p);
    p.x0 = 8, p.y0 = 8, p.z0 = 8, p.nx = 4, p.ny = 2, p.nz = 1, p.sx = 2, p.sy = 1, p.sz = 1;
    p.first_step = 0, p.period = 1;
    p.ear_a[1] = -2, p.ear_b[1] = 2;
    p.max_lag = 5, p.n_bins = 2, p.threshold = 0.0f, p.edges[1] = 8, p.n_sections = 2;
    return p;
}

struct Fault {
    const char* sentence;
    std::function<void(wv_interaural_plan&, const wv_biquad*&)> make;
};

static const char* answer(const wv_interaural_plan& p, const wv_biquad* sections) {
    const char* why = nullptr;
    const int rc = wv::interaural_plan_check(p, sections, NX, NY, NZ, &why);
    CHECK((rc == WV_OK) == (why == nullptr));
    CHECK(rc == WV_OK || rc == WV_E_INVALID_ARGUMENT);
    return why;
}

int main() {
    using namespace wv;
    CHECK(kInterauralStage == 16 && kInterauralMaxBins == 4 && kInterauralMaxLag == 16 && kInterauralMaxEar == 8 && kInterauralMaxSections == 4);
    CHECK(sizeof(wv_interaural_plan) == 112);

    // every refusal, in the order of the contract
    const std::vector<Fault> faults = {
        {"wv_set_interaural: n_bins must be 1 .. 4", [](wv_interaural_plan& p, const wv_biquad*&) { p.n_bins = 5; }},
        {"wv_set_interaural: edges[0] must be 0 and the edges strictly increasing", [](wv_interaural_plan& p, const wv_biquad*&) { p.edges[0] = 1; }},
        {"wv_set_interaural: the threshold must be >= 0 and finite", [](wv_interaural_plan& p, const wv_biquad*&) { p.threshold = -1.0f; }},
        {"wv_set_interaural: max_lag must be 0 .. 16", [](wv_interaural_plan& p, const wv_biquad*&) { p.max_lag = 17; }},
        {"wv_set_interaural: every component of an ear offset must be -8 .. 8", [](wv_interaural_plan& p, const wv_biquad*&) { p.ear_b[2] = 9; }},
        {"wv_set_interaural: n_sections must be 0 .. 4", [](wv_interaural_plan& p, const wv_biquad*&) { p.n_sections = 5; }},
        {"wv_set_interaural: every coefficient must be finite", [](wv_interaural_plan&, const wv_biquad*& s) { s = bad; }},
        {"wv_set_interaural: strides must be >= 1", [](wv_interaural_plan& p, const wv_biquad*&) { p.sy = 0; }},
        {"wv_set_interaural: period must be >= 1", [](wv_interaural_plan& p, const wv_biquad*&) { p.period = 0; }},
        {"wv_set_interaural: the box leaves the mesh", [](wv_interaural_plan& p, const wv_biquad*&) { p.z0 = NZ; }},
        {"wv_set_interaural: an ear leaves the mesh", [](wv_interaural_plan& p, const wv_biquad*&) { p.ear_a[0] = -8, p.x0 = 7; }},
    };
    CHECK(answer(base(), good) == nullptr);
    for (size_t i = 0; i < faults.size(); ++i)
        for (size_t k = i; k < faults.size(); ++k) {
            wv_interaural_plan p = base();
            const wv_biquad* s = good;
            faults[k].make(p, s);
            faults[i].make(p, s);
            const char* why = answer(p, s);
            CHECK(why && !std::strcmp(why, faults[i].sentence));
            p = base(), s = good;  // (and in the other order of making them)
            faults[i].make(p, s);
            faults[k].make(p, s);
            why = answer(p, s);
            CHECK(why && !std::strcmp(why, faults[i].sentence));
        }
    {   // further forms of the same faults
        wv_interaural_plan p = base();
        p.n_bins = 0;
        CHECK(!std::strcmp(answer(p, good), "wv_set_interaural: n_bins must be 1 .. 4"));
        p = base(), p.edges[1] = 0;
        CHECK(!std::strcmp(answer(p, good), "wv_set_interaural: edges[0] must be 0 and the edges strictly increasing"));
        p = base(), p.threshold = std::nanf("");
        CHECK(!std::strcmp(answer(p, good), "wv_set_interaural: the threshold must be >= 0 and finite"));
        p = base(), p.ear_a[0] = -9;
        CHECK(!std::strcmp(answer(p, good), "wv_set_interaural: every component of an ear offset must be -8 .. 8"));
        p = base();
        CHECK(!std::strcmp(answer(p, nullptr), "null argument"));
        p.n_sections = 0;
        CHECK(answer(p, nullptr) == nullptr && answer(p, bad) == nullptr);  // (no sections: the array is not looked at)
        p = base(), p.n_sections = 1;
        CHECK(answer(p, bad) == nullptr);                                    // (only the plan's own sections are)
        p = base(), p.max_lag = 0;
        CHECK(answer(p, good) == nullptr);
        p.max_lag = 16, p.n_bins = 4, p.edges[2] = 9, p.edges[3] = 10, p.n_sections = 4;
        CHECK(answer(p, good) == nullptr);
        // a plane of 2^31 nodes: the last check, on a mesh that holds it
        p = base(), p.x0 = 8, p.y0 = 8, p.nx = 1 << 16, p.ny = 1 << 15, p.sx = 1;
        const char* why = nullptr;
        CHECK(interaural_plan_check(p, good, (1 << 16) + 16, (1 << 15) + 16, NZ, &why) == WV_E_INVALID_ARGUMENT &&
              !std::strcmp(why, "wv_set_interaural: more than 2^31 nodes per plane of the box"));
        p.ear_a[0] = -8, p.x0 = 7;
        CHECK(interaural_plan_check(p, good, (1 << 16) + 16, (1 << 15) + 16, NZ, &why) == WV_E_INVALID_ARGUMENT &&
              !std::strcmp(why, "wv_set_interaural: an ear leaves the mesh"));
    }
    {   // the ears on the faces: the first and the last node taken, strides counted
        wv_interaural_plan p = base();
        p.x0 = 8, p.nx = 4, p.sx = 2;                        // x = 8, 10, 12, 14
        p.ear_a[0] = -8, p.ear_b[0] = 8;
        CHECK(answer(p, good) == nullptr);                    // 0 .. 22 < 24
        p.x0 = 9;                                             // 9 .. 15: 15 + 8 = 23, the last node
        CHECK(answer(p, good) == nullptr);
        p.x0 = 10;                                            // 16 + 8 = 24: off
        CHECK(!std::strcmp(answer(p, good), "wv_set_interaural: an ear leaves the mesh"));
        p.x0 = 7;                                             // 7 - 8 < 0
        CHECK(!std::strcmp(answer(p, good), "wv_set_interaural: an ear leaves the mesh"));
        p = base(), p.z0 = 0, p.ear_a[2] = -1;
        CHECK(!std::strcmp(answer(p, good), "wv_set_interaural: an ear leaves the mesh"));
        p.ear_a[2] = 0, p.z0 = NZ - 1, p.ear_b[2] = 1;
        CHECK(!std::strcmp(answer(p, good), "wv_set_interaural: an ear leaves the mesh"));
        p.ear_b[2] = 0;
        CHECK(answer(p, good) == nullptr);
        CHECK(interaural_axis_holds(0, 1, 1, 0, 1) && !interaural_axis_holds(0, 1, 1, 1, 1) && !interaural_axis_holds(0, 1, 1, -1, 1));
        CHECK(interaural_axis_holds(3, 5, 4, -3, 20) && !interaural_axis_holds(3, 5, 4, 1, 20) && interaural_axis_holds(3, 5, 4, 0, 20));
    }

    // the bin of a capture is arrival_bin over four entries
    const uint32_t e4[16] = {0, 3, 8, 20}, e1[16] = {0};
    for (uint32_t n = 1; n <= 4; ++n)
        for (uint32_t rel = 0; rel < 40; ++rel) CHECK(interaural_bin(rel, e4, n) == arrival_bin(rel, e4, n));
    CHECK(interaural_bin(0, e4, 4) == 0 && interaural_bin(2, e4, 4) == 0 && interaural_bin(3, e4, 4) == 1 && interaural_bin(19, e4, 4) == 2);
    CHECK(interaural_bin(20, e4, 4) == 3 && interaural_bin(0xFFFFFFFEu, e4, 4) == 3 && interaural_bin(1000, e1, 1) == 0);

    // the lag class, the planes
    CHECK(interaural_lag_class(0) == 0 && interaural_lag_class(1) == 4 && interaural_lag_class(4) == 4 && interaural_lag_class(5) == 8);
    CHECK(interaural_lag_class(8) == 8 && interaural_lag_class(9) == 16 && interaural_lag_class(16) == 16);
    CHECK(interaural_planes(0) == 3 && interaural_planes(5) == 13 && interaural_planes(16) == 35);
    CHECK(interaural_lag_plane(5, -5) == 2 && interaural_lag_plane(5, 0) == 7 && interaural_lag_plane(5, 5) == 12 && interaural_lag_plane(0, 0) == 2);

    // sizes and places: block 0 pre[2][B], bins[n_bins][2 L + 3][B], onset[B]; block 1 history[2][L][B], z[2][S][2][B]
    CHECK(interaural_stage_bytes(630) == 630ull * 16 * 2 * 4);
    CHECK(interaural_pre_offset() == 0 && interaural_bins_offset(630) == 630ull * 16);
    CHECK(interaural_bins_bytes(630, 3, 5) == 630ull * 3 * 13 * 8);
    CHECK(interaural_onset_offset(630, 3, 5) == interaural_bins_offset(630) + interaural_bins_bytes(630, 3, 5));
    CHECK(interaural_sums_bytes(630, 3, 5) == interaural_onset_offset(630, 3, 5) + 630ull * 4);
    CHECK(interaural_sums_bytes(1, 4, 16) == 16 + 4 * 35 * 8 + 4);                    // 1140 bytes per node at the most
    CHECK(interaural_fetch_bytes(630, 3, 5) == interaural_sums_bytes(630, 3, 5));
    CHECK(interaural_history_bytes(630, 5) == 630ull * 2 * 5 * 8 && interaural_filter_offset(630, 5) == interaural_history_bytes(630, 5));
    CHECK(interaural_carry_bytes(630, 5, 3) == 630ull * (10 + 12) * 8 && interaural_carry_bytes(630, 0, 0) == 0);
    CHECK(interaural_carry_bytes(1, 16, 4) == (32 + 16) * 8);
    CHECK(interaural_map_bytes(630) == 2520 && interaural_coef_bytes(0) == 0 && interaural_coef_bytes(4) == 160);
    CHECK(interaural_stage_bytes(kDecayNoSize) == kDecayNoSize && interaural_sums_bytes(1ull << 61, 4, 16) == kDecayNoSize);
    CHECK(interaural_carry_bytes(1ull << 61, 16, 4) == kDecayNoSize);

    // the ring of the history
    CHECK(interaural_history_slot(0, 5) == 0 && interaural_history_slot(4, 5) == 4 && interaural_history_slot(5, 5) == 0 && interaural_history_slot(17, 1) == 0);
    CHECK(interaural_history_slot(0xFFFFFFFEu, 16) == 14);

    // the traffic model
    CHECK(interaural_fold_traffic(630, 16, 0, 0, 1, false) == 630ull * (128 + 4 + 48));
    CHECK(interaural_fold_traffic(630, 16, 16, 4, 2, true) == 630ull * (128 + 4 + 256 + 256 + 256 + 16 * 35 * 2 + 4));
    CHECK(interaural_fold_traffic(630, 3, 8, 0, 1, false) == 630ull * (24 + 4 + 128 + 48 + 16 * 19));
    CHECK(interaural_fold_traffic(kDecayNoSize, 16, 1, 1, 1, false) == kDecayNoSize);

    if (failures == 0) std::printf("INTERAURAL PLAN OK\n");
    return failures ? 1 : 0;
}

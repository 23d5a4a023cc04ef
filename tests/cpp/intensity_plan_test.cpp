// intensity_plan_test.cpp -- wayverb_amd/csrc/intensity_plan.h on the CPU (tests/test_intensity_plan.py builds and runs this).  Every
// expectation below is derived by hand from the contract in include/wayverb_amd.h and DESIGN.md 4.12, none recorded from the code.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "intensity_plan.h"

static int g_failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++g_failures;                                                   \
        }                                                                   \
    } while (0)

using namespace wv;

// a good plan on a 24 x 20 x 28 mesh: the whole interior
static wv_intensity_plan good() {
    wv_intensity_plan p{};
    p.x0 = p.y0 = p.z0 = 1;
    p.nx = 22, p.ny = 18, p.nz = 26;
    p.sx = p.sy = p.sz = 1;
    p.first_step = 0, p.period = 1;
    p.n_bins = 7, p.bin_captures = 3;
    p.spacing = 0.05, p.sample_rate = 12000.0, p.ambient_density = 1.225;
    return p;
}

static int check(const wv_intensity_plan& p, const char** why = nullptr) {
    const char* w = nullptr;
    const int rc = intensity_plan_check(p, 24, 20, 28, &w);
    CHECK((rc == WV_OK) == (w == nullptr));
    if (why) *why = w;
    return rc;
}

static bool refused_with(const wv_intensity_plan& p, const char* part) {
    const char* w = nullptr;
    return check(p, &w) == WV_E_INVALID_ARGUMENT && w && std::strstr(w, part);
}

static void arguments() {
    CHECK(check(good()) == WV_OK);
    CHECK(intensity_plan_check(good(), 24, 20, 28, nullptr) == WV_OK);   // (why may be NULL)
    wv_intensity_plan p = good();
    p.n_bins = 0;
    CHECK(refused_with(p, "n_bins"));
    p.n_bins = 4097;
    CHECK(refused_with(p, "n_bins"));
    p.n_bins = 4096;
    CHECK(check(p) == WV_OK);
    p = good(), p.bin_captures = 0;
    CHECK(refused_with(p, "bin_captures"));
    p = good(), p.sx = 0;
    CHECK(refused_with(p, "strides"));
    p = good(), p.sy = -1;
    CHECK(refused_with(p, "strides"));
    p = good(), p.sz = 0;
    CHECK(refused_with(p, "strides"));
    p = good(), p.period = 0;
    CHECK(refused_with(p, "period"));
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (double bad : {0.0, -1.0, inf, -inf, nan}) {
        p = good(), p.spacing = bad;
        CHECK(refused_with(p, "positive and finite"));
        p = good(), p.sample_rate = bad;
        CHECK(refused_with(p, "positive and finite"));
        p = good(), p.ambient_density = bad;
        CHECK(refused_with(p, "positive and finite"));
    }
    p = good(), p.spacing = std::numeric_limits<double>::denorm_min();   // positive and finite, however small
    CHECK(check(p) == WV_OK);
    p = good(), p.nx = 0;
    CHECK(refused_with(p, "leaves the mesh"));
    p = good(), p.x0 = -1;
    CHECK(refused_with(p, "leaves the mesh"));
    p = good(), p.nx = 24;   // 1 + 23 = 24: past the last node
    CHECK(refused_with(p, "leaves the mesh"));
    intensity_plan_check(p, 24, 20, 28, nullptr);
}

// a taken node with a neighbour off the grid, on each of the six sides, at stride 1 and at stride 3
static void edges() {
    wv_intensity_plan p = good();
    // stride 1: first node 0 / last node mesh - 1 on each axis
    p = good(), p.x0 = 0;
    CHECK(refused_with(p, "adjacent to a boundary"));
    p = good(), p.nx = 23;    // 1 .. 23
    CHECK(refused_with(p, "adjacent to a boundary"));
    p = good(), p.y0 = 0;
    CHECK(refused_with(p, "adjacent to a boundary"));
    p = good(), p.ny = 19;    // 1 .. 19
    CHECK(refused_with(p, "adjacent to a boundary"));
    p = good(), p.z0 = 0;
    CHECK(refused_with(p, "adjacent to a boundary"));
    p = good(), p.nz = 27;    // 1 .. 27
    CHECK(refused_with(p, "adjacent to a boundary"));
    // the largest boxes that pass
    p = good();
    CHECK(check(p) == WV_OK);  // 1 .. 22, 1 .. 18, 1 .. 26
    p.x0 = 22, p.nx = 1, p.y0 = 18, p.ny = 1, p.z0 = 26, p.nz = 1;
    CHECK(check(p) == WV_OK);
    // stride 3 from 1: x takes 1, 4, .., 22 (8 nodes), y 1 .. 16 (6), z 1 .. 25 (9); one more node on an axis lands on 25 (off x), 19 (the
    // last y node), 28 (off z)
    p = good(), p.sx = p.sy = p.sz = 3, p.nx = 8, p.ny = 6, p.nz = 9;
    CHECK(check(p) == WV_OK);
    p.ny = 7;                 // 1 + 6 * 3 = 19 = mesh_ny - 1: on the grid, its +y neighbour is not
    CHECK(refused_with(p, "adjacent to a boundary"));
    p.ny = 6, p.nx = 9;       // 25: off the grid altogether
    CHECK(refused_with(p, "leaves the mesh"));
    p = good(), p.sx = p.sy = p.sz = 3, p.x0 = 2, p.nx = 8, p.ny = 6, p.nz = 9;   // 2 .. 23 = mesh_nx - 1
    CHECK(refused_with(p, "adjacent to a boundary"));
    p = good(), p.sx = p.sy = p.sz = 3, p.nx = 8, p.ny = 6, p.z0 = 3, p.nz = 9;   // 3 .. 27 = mesh_nz - 1
    CHECK(refused_with(p, "adjacent to a boundary"));
    p = good(), p.sx = p.sy = p.sz = 3, p.nx = 8, p.ny = 6, p.nz = 9;
    p.x0 = 0, p.nx = 8;       // 0 .. 21
    CHECK(refused_with(p, "adjacent to a boundary"));
    p.x0 = 1, p.y0 = 0;       // 0 .. 15
    CHECK(refused_with(p, "adjacent to a boundary"));
    p.y0 = 1, p.z0 = 0;       // 0 .. 24
    CHECK(refused_with(p, "adjacent to a boundary"));
    // the sentence is the reference's, word for word
    const char* w = nullptr;
    p = good(), p.x0 = 0;
    check(p, &w);
    CHECK(w && !std::strcmp(w, "Can't place directional_receiver at this node as it is adjacent to a boundary."));
    // a mesh too thin to hold any node with both neighbours
    p = good(), p.nz = 1, p.z0 = 1;
    CHECK(intensity_plan_check(p, 24, 20, 2, nullptr) == WV_E_INVALID_ARGUMENT);
    CHECK(intensity_plan_check(p, 24, 20, 3, nullptr) == WV_OK);
}

static void sizes() {
    // B = 630: stage 16 slots x 4 planes x 4 bytes = 256 B per node; bins 32 n_bins; velocities 24
    CHECK(intensity_stage_bytes(630) == 630ull * 256);
    CHECK(intensity_bins_bytes(630, 7) == 630ull * 7 * 32);
    CHECK(intensity_velocity_bytes(630) == 630ull * 24);
    CHECK(intensity_stage_bytes(1) == 256 && intensity_bins_bytes(1, 1) == 32 && intensity_velocity_bytes(1) == 24);
    CHECK(intensity_stage_bytes(0) == 0);
    // past 64 bits
    CHECK(intensity_stage_bytes(1ull << 57) == kDecayNoSize);
    CHECK(intensity_bins_bytes(1ull << 50, 4096) == kDecayNoSize);
    CHECK(intensity_stage_bytes(kDecayNoSize) == kDecayNoSize && intensity_velocity_bytes(kDecayNoSize) == kDecayNoSize);
    // the traffic model B (16 t + 48 + 64 r): a full stage into one bin, into 16 bins; one capture
    CHECK(intensity_fold_traffic(1000, 16, 1) == 1000ull * (256 + 48 + 64));
    CHECK(intensity_fold_traffic(1000, 16, 16) == 1000ull * (256 + 48 + 1024));
    CHECK(intensity_fold_traffic(1, 1, 1) == 128);
    CHECK(kIntensityStage == 16 && kIntensityPlanes == 4);
    CHECK(sizeof(wv_intensity_plan) == 88);
}

int main() {
    arguments();
    edges();
    sizes();
    if (g_failures) {
        std::printf("%d failures\n", g_failures);
        return 1;
    }
    std::printf("INTENSITY PLAN OK\n");
    return 0;
}

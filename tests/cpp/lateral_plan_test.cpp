// lateral_plan_test.cpp -- wayverb_amd/csrc/lateral_plan.h on the CPU (tests/test_lateral_plan.py builds and runs this).  Every
// expectation below is derived by hand from the contract in include/wayverb_amd.h and DESIGN.md 4.14, none recorded from the code.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "lateral_plan.h"

static int g_failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++g_failures;                                                   \
        }                                                                   \
    } while (0)

using namespace wv;

// a plan the 24 x 20 x 28 mesh accepts: the whole interior, three bins
static wv_lateral_plan good() {
    wv_lateral_plan p;
    std::memset(&p, 0, sizeof p);
    p.x0 = p.y0 = p.z0 = 1;
    p.nx = 22, p.ny = 18, p.nz = 26;
    p.sx = p.sy = p.sz = 1;
    p.first_step = 0, p.period = 1;
    p.n_bins = 3;
    p.threshold = 1e-3f;
    p.edges[0] = 0, p.edges[1] = 40, p.edges[2] = 640;   // 5 and 80 ms at 8 kHz
    p.spacing = 0.05, p.sample_rate = 8000.0, p.ambient_density = 1.2;
    return p;
}

static bool refused(const wv_lateral_plan& p, const char* with) {
    const char* why = nullptr;
    const int rc = lateral_plan_check(p, 24, 20, 28, &why);
    return rc == WV_E_INVALID_ARGUMENT && why && std::strstr(why, with);
}

static void refusals() {
    const char* why = "x";
    CHECK(lateral_plan_check(good(), 24, 20, 28, &why) == WV_OK && why == nullptr);
    CHECK(lateral_plan_check(good(), 24, 20, 28, nullptr) == WV_OK);
    wv_lateral_plan p = good();
    p.n_bins = 0;
    CHECK(refused(p, "n_bins must be 1 .. 8"));
    p.n_bins = 9;
    CHECK(refused(p, "n_bins must be 1 .. 8"));
    p = good(), p.n_bins = 8;                     // the fourth entry is 0: not increasing
    CHECK(refused(p, "edges"));
    for (uint32_t k = 0; k < 8; ++k) p.edges[k] = 5 * k;
    CHECK(lateral_plan_check(p, 24, 20, 28, &why) == WV_OK);
    p.edges[7] = 0xFFFFFFFEu;                     // the largest rel there is
    CHECK(lateral_plan_check(p, 24, 20, 28, &why) == WV_OK);
    p = good(), p.edges[0] = 1;
    CHECK(refused(p, "edges[0] must be 0"));
    p = good(), p.edges[2] = 40;
    CHECK(refused(p, "strictly increasing"));
    p = good(), p.threshold = -1e-30f;
    CHECK(refused(p, "threshold"));
    p.threshold = std::numeric_limits<float>::infinity();
    CHECK(refused(p, "threshold"));
    p.threshold = std::numeric_limits<float>::quiet_NaN();
    CHECK(refused(p, "threshold"));
    p.threshold = 0.0f;                           // legal: every onset is capture 0
    CHECK(lateral_plan_check(p, 24, 20, 28, &why) == WV_OK);
    p = good(), p.sy = 0;
    CHECK(refused(p, "strides"));
    p = good(), p.period = 0;
    CHECK(refused(p, "period"));
    p = good(), p.spacing = 0;
    CHECK(refused(p, "positive and finite"));
    p = good(), p.sample_rate = -8000.0;
    CHECK(refused(p, "positive and finite"));
    p = good(), p.ambient_density = std::numeric_limits<double>::infinity();
    CHECK(refused(p, "positive and finite"));
    p = good(), p.spacing = std::numeric_limits<double>::quiet_NaN();
    CHECK(refused(p, "positive and finite"));
    p = good(), p.nx = 24;                        // x0 + nx - 1 = 24: leaves the mesh
    CHECK(refused(p, "leaves the mesh"));
    p = good(), p.nz = 0;
    CHECK(refused(p, "leaves the mesh"));
    // a taken node on a face of the mesh has a neighbour off the grid: the reference's sentence, on every face
    p = good(), p.x0 = 0;
    CHECK(refused(p, "Can't place directional_receiver at this node as it is adjacent to a boundary."));
    p = good(), p.nx = 23;                        // the last node taken is x = 23, the +x face
    CHECK(refused(p, "adjacent to a boundary"));
    p = good(), p.y0 = 0;
    CHECK(refused(p, "adjacent to a boundary"));
    p = good(), p.ny = 19;
    CHECK(refused(p, "adjacent to a boundary"));
    p = good(), p.z0 = 0;
    CHECK(refused(p, "adjacent to a boundary"));
    p = good(), p.nz = 27;
    CHECK(refused(p, "adjacent to a boundary"));
    // decimated: x = 1, 4, ..., 22 is 8 nodes and ends on the last interior node; 9 would leave the mesh
    p = good(), p.sx = 3, p.nx = 8;
    CHECK(lateral_plan_check(p, 24, 20, 28, &why) == WV_OK);
    p.nx = 9;
    CHECK(refused(p, "leaves the mesh"));
    p = good(), p.sx = 2, p.x0 = 1, p.nx = 12;    // x = 1, 3, ..., 23: the last one is on the face
    CHECK(refused(p, "adjacent to a boundary"));
    // the order of the checks: n_bins before edges before the threshold before the box
    p = good(), p.n_bins = 0, p.edges[0] = 1, p.threshold = -1, p.x0 = 0;
    CHECK(refused(p, "n_bins"));
    p.n_bins = 3;
    CHECK(refused(p, "edges"));
    p.edges[0] = 0;
    CHECK(refused(p, "threshold"));
    const SnapshotBox b = lateral_box(good());
    CHECK(b.x0 == 1 && b.y0 == 1 && b.z0 == 1 && b.nx == 22 && b.ny == 18 && b.nz == 26 && b.sx == 1 && b.sy == 1 && b.sz == 1);
    CHECK(kLateralMaxBins == 8 && kLateralPlanes == 10 && kLateralStage == 16 && kLateralNone == 0xFFFFFFFFu && kLateralMaxCaptures == 0xFFFFFFFFull);
}

static void sizes() {
    // B = 630, 3 bins: doubles first -- pre at 0, velocity at 5040 (15120 bytes), bins at 20160 (30 planes of 5040 = 151200 bytes),
    // then onset at 171360; 173880 bytes = 630 * (36 + 240)
    CHECK(lateral_pre_offset() == 0);
    CHECK(lateral_velocity_offset(630) == 5040);
    CHECK(lateral_velocity_bytes(630) == 15120);
    CHECK(lateral_bins_offset(630) == 20160);
    CHECK(lateral_bins_bytes(630, 3) == 151200);
    CHECK(lateral_onset_offset(630, 3) == 171360);
    CHECK(lateral_state_bytes(630, 3) == 173880);
    // an odd B: every double part starts on a multiple of 8, the onsets on a multiple of 4
    for (uint64_t nodes : {1ull, 567ull, 255ull, 257ull})
        for (uint32_t n_bins = 1; n_bins <= 8; ++n_bins) {
            CHECK(lateral_velocity_offset(nodes) % 8 == 0 && lateral_bins_offset(nodes) % 8 == 0 && lateral_onset_offset(nodes, n_bins) % 8 == 0);
            CHECK(lateral_bins_offset(nodes) + lateral_bins_bytes(nodes, n_bins) == lateral_onset_offset(nodes, n_bins));
            CHECK(lateral_velocity_offset(nodes) + lateral_velocity_bytes(nodes) == lateral_bins_offset(nodes));
            CHECK(lateral_state_bytes(nodes, n_bins) == nodes * (36 + 80 * n_bins));
        }
    CHECK(lateral_state_bytes(1, 1) == 116 && lateral_state_bytes(1, 8) == 676 && lateral_state_bytes(0, 8) == 0);
    // the stage is the intensity plan's: 16 slots of four floats, 256 bytes per node; the map one float
    CHECK(lateral_stage_bytes(630) == 630 * 256 && lateral_map_bytes(630) == 2520);
    // past 64 bits: kDecayNoSize, never a wrapped number
    const uint64_t huge = 1ull << 60;
    CHECK(lateral_state_bytes(huge, 8) == kDecayNoSize);
    CHECK(lateral_state_bytes(huge, 1) == kDecayNoSize);       // 116 * 2^60
    CHECK(lateral_onset_offset(huge, 1) == kDecayNoSize);      // 112 * 2^60
    CHECK(lateral_bins_bytes(huge, 1) == kDecayNoSize);        // 80 * 2^60
    CHECK(lateral_bins_offset(huge) == kDecayNoSize);          // 32 * 2^60 = 2^65
    CHECK(lateral_velocity_offset(huge) == 8 * huge);
    CHECK(lateral_stage_bytes(huge) == kDecayNoSize);
    CHECK(lateral_map_bytes(1ull << 62) == kDecayNoSize);
    CHECK(lateral_state_bytes(kDecayNoSize, 1) == kDecayNoSize);
    // 2^57 nodes, one bin: 116 * 2^57 = 14.5 * 2^60 fits; 2^58: 29 * 2^60 > 2^64 -> no size
    CHECK(lateral_state_bytes(1ull << 57, 1) == 116 * (1ull << 57));
    CHECK(lateral_state_bytes(1ull << 58, 1) == kDecayNoSize);
    // the traffic model: four floats per capture, the onset and the velocities there and back (52 bytes), ten sums per bin read and
    // written, 4 more with a map
    CHECK(lateral_fold_traffic(1000, 16, 1, false) == 1000 * (256 + 52 + 160));
    CHECK(lateral_fold_traffic(1000, 16, 2, true) == 1000 * (256 + 52 + 320 + 4));
    CHECK(lateral_fold_traffic(1, 1, 1, false) == 228);
    CHECK(lateral_fold_traffic(huge, 16, 1, false) == kDecayNoSize);
}

int main() {
    refusals();
    sizes();
    if (g_failures) {
        std::printf("%d FAILURES\n", g_failures);
        return 1;
    }
    std::printf("LATERAL PLAN OK\n");
    return 0;
}

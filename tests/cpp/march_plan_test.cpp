// march_plan_test.cpp -- the march planners of wayverb_amd/csrc/march_plan.h on the CPU (tests/test_march_plan.py builds and runs this).
//
// Inputs come from fixed formulas below; what the planners make of them is printed as one JSON object, which the Python side compares
// with tests/golden/march_plan_cases.json (recorded from the planners as they stood inside the engine before they moved here).  What must
// hold by construction is checked right here: a failed check prints a line and the program exits 1.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <set>
#include <sstream>
#include <string>
#include <utility>

#include "march_plan.h"

namespace {

int failures = 0;
#define CHECK(cond, name)                                                         \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::printf("CHECK FAILED %s: %s (line %d)\n", name, #cond, __LINE__); \
            ++failures;                                                           \
        }                                                                         \
    } while (0)

std::ostringstream out;
bool first_case = true;
void begin_case(const std::string& name) {
    out << (first_case ? "" : ",\n") << "\"" << name << "\": ";
    first_case = false;
}

uint64_t fnv1a(uint64_t h, const void* data, size_t n) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001B3ull;
    return h;
}
constexpr uint64_t kFnvBasis = 0xCBF29CE484222325ull;
std::string hex(uint64_t v) {
    char b[32];
    std::snprintf(b, sizeof b, "\"%016" PRIx64 "\"", v);
    return b;
}
template <typename T>
std::string list_of(const T* v, int n) {
    std::ostringstream s;
    s << "[";
    for (int i = 0; i < n; ++i) s << (i ? "," : "") << (long long)v[i];
    s << "]";
    return s.str();
}

// ---- windows --------------------------------------------------------------------------------------------------------------------------
// every row length from 1 to 50 waves: windows and widest per length, a hash over all window tables, the tables of 16 and 50 waves in full
void windows_case(const std::string& name, const std::function<int(int, uint8_t (*)[wv::kMarchMaxWindows], int*)>& split) {
    int n_of[50], widest_of[50];
    uint64_t h = kFnvBasis;
    std::string full;
    for (int row = 1; row <= 50; ++row) {
        uint8_t win[4][wv::kMarchMaxWindows] = {};
        int widest = -7;
        const int n = split(row, win, &widest);
        n_of[row - 1] = n;
        widest_of[row - 1] = widest;
        for (int k = 0; k < n; ++k) {
            const uint8_t e[4] = {win[0][k], win[1][k], win[2][k], win[3][k]};
            h = fnv1a(h, e, 4);
            // a window stores a non-empty range inside what it runs, the ranges tile the row
            CHECK(e[2] < e[3] && e[0] <= e[2] && e[3] <= e[0] + e[1] && e[0] + e[1] <= row, name.c_str());
            CHECK(e[2] == (k ? win[3][k - 1] : 0) && (k + 1 < n || e[3] == row), name.c_str());
            CHECK(e[1] <= widest, name.c_str());
        }
        if (row == 16 || row == 50) {
            full += std::string(", \"row") + std::to_string(row) + "\": [";
            for (int j = 0; j < 4; ++j) full += (j ? "," : "") + list_of(win[j], n > 0 ? n : 0);
            full += "]";
        }
    }
    begin_case(name);
    out << "{\"windows\": " << list_of(n_of, 50) << ", \"widest\": " << list_of(widest_of, 50) << ", \"tables\": " << hex(h) << full << "}";
}

// ---- chunks ---------------------------------------------------------------------------------------------------------------------------
struct March {  // what differs between the two marches in choose_chunks
    int warmup, search_planes, least_planes;
};
const March kTwoStep{3, 8, 8}, kThreeStep{4, 12, 4};

// workgroups the chip holds at once (engine_pair.hip.h / engine_triple.hip.h)
int64_t pair_slots(int nw) { return 256ll * std::max(1, 8 / nw); }
int64_t triple_slots(int nw, int lane_bytes) {
    const int max_waves = lane_bytes == 8 ? 12 : 8;
    const size_t lds = (size_t)nw * 18 * 64 * lane_bytes + (size_t)2 * 18 * (max_waves + 2) * 2 * lane_bytes;
    return 256ll * std::min(std::max<int>(1, (int)((160u * 1024u) / lds)), std::max(1, max_waves / nw));
}

void chunks_case(const std::string& name, const March& m, int rows, int row_waves_pair, int owned, int64_t want_rounds, int forced, int lane_bytes = 0) {
    wv::MarchPlan p;
    p.z0 = 2;
    p.z1 = 2 + owned;
    p.strips = (rows + 3) / 4;
    int64_t wgs, slots;
    if (!lane_bytes) {  // two-step: 16-byte lanes, rows of up to 8 waves in one workgroup (longer ones: the planner counts strips all the same)
        p.nw = std::min(row_waves_pair, 8);
        wgs = p.strips;
        slots = pair_slots(p.nw);
    } else {  // three-step: lanes of lane_bytes, equal-share windows where a row is longer than a workgroup
        const int row_waves = row_waves_pair * 16 / lane_bytes;
        p.windows = wv::triple_windows(row_waves, p.win, &p.nw, false, lane_bytes == 8 ? 12 : 8);
        CHECK(p.windows >= 0, name.c_str());
        wgs = (int64_t)p.strips * std::max(1, p.windows);
        slots = triple_slots(p.nw, lane_bytes);
    }
    wv::choose_chunks(p, wgs, slots, m.warmup, m.search_planes, m.least_planes, want_rounds, forced);
    CHECK(p.zc >= 1 && p.chunks >= 1 && (int64_t)p.zc * p.chunks >= owned && (int64_t)p.zc * (p.chunks - 1) < owned, name.c_str());
    begin_case(name);
    out << "{\"zc\": " << p.zc << ", \"chunks\": " << p.chunks << "}";
}

// ---- unit lists -----------------------------------------------------------------------------------------------------------------------
struct Room {
    int nx, ny, nz;
    std::function<bool(int, int, int)> inside;
};
struct Activity {
    int strips, row_waves;
    std::vector<uint8_t> active;
    std::vector<uint16_t> bits;
};
Activity activity_of(const Room& room, int wave_cols) {
    Activity a;
    a.strips = (room.ny + 3) / 4;
    a.row_waves = room.nx / wave_cols;
    a.active.assign((size_t)room.nz * a.strips, 0);
    a.bits.assign((size_t)room.nz * a.strips, 0);
    for (int z = 0; z < room.nz; ++z)
        for (int y = 0; y < room.ny; ++y)
            for (int x = 0; x < room.nx; ++x)
                if (room.inside(x, y, z)) {
                    a.active[(size_t)z * a.strips + y / 4] = 1;
                    a.bits[(size_t)z * a.strips + y / 4] |= (uint16_t)(1u << (x / wave_cols));
                }
    return a;
}

wv::UnitRules two_step_rules(const Activity& a, int nz, int start_height, bool search, bool spans, bool by_chunk = true) {
    wv::UnitRules r{};
    r.nz = nz;
    r.row_waves = a.row_waves;
    r.warmup = 3;
    r.halo = 2;
    r.extra_lo = r.extra_hi = 0;
    r.slots_per_xcd = 32ll * std::max(1, 8 / a.row_waves);
    r.start_height = start_height;
    r.search = search;
    r.search_in_limit = true;
    r.search_follows = true;
    r.chunk_shift = 16;
    r.first_shift = 25;
    r.span_shift = 28;
    r.spans = spans;
    r.by_chunk = by_chunk;
    return r;
}
wv::UnitRules three_step_rules(const Activity& a, int nz, int start_height, bool search, int extra_lo, int extra_hi) {
    wv::UnitRules r{};
    r.nz = nz;
    r.row_waves = a.row_waves;
    r.warmup = 4;
    r.halo = 3;
    r.extra_lo = extra_lo;
    r.extra_hi = extra_hi;
    r.slots_per_xcd = 32ll * std::max(1, 12 / a.row_waves);
    r.start_height = start_height;
    r.search = search;
    r.search_in_limit = false;
    r.search_follows = false;
    r.chunk_shift = 14;
    r.first_shift = 23;
    r.span_shift = 27;
    r.spans = true;
    r.by_chunk = true;
    return r;
}

// what must hold of a list whatever the golden data say
void check_list(const std::string& name, const wv::MarchPlan& p, const wv::UnitRules& r, const Activity& a) {
    const char* n = name.c_str();
    const uint32_t strip_mask = (1u << r.chunk_shift) - 1u;
    std::set<std::pair<int, int>> listed;
    for (uint32_t e : p.units) {
        const int s = (int)(e & strip_mask), c = (int)((e >> r.chunk_shift) & 0x1FFu);
        CHECK(s < p.strips && c < p.chunks, n);
        CHECK(listed.insert({s, c}).second, n);  // once
        const int zb = p.z0 + c * p.zc, ze = std::min(zb + p.zc, p.z1);
        if (r.spans) {
            const uint32_t first = (e >> r.first_shift) & ((1u << (r.span_shift - r.first_shift)) - 1u), span = (e >> r.span_shift) + 1u;
            CHECK(first + span <= (uint32_t)r.row_waves, n);
            uint32_t bits = 0;
            for (int z = std::max(0, zb - r.halo); z < std::min(r.nz, ze + r.halo); ++z)
                for (int ss = std::max(0, s - 1); ss <= std::min(p.strips - 1, s + 1); ++ss) bits |= a.bits[(size_t)z * p.strips + ss];
            const uint32_t covered = ((1u << span) - 1u) << first;
            CHECK((bits & ~covered) == 0, n);
        } else {
            CHECK((e >> (r.chunk_shift + 9)) == 0, n);
        }
    }
    size_t live = 0;
    for (int s = 0; s < p.strips; ++s)
        for (int c = 0; c < p.chunks; ++c) {
            const int zb = p.z0 + c * p.zc, ze = std::min(zb + p.zc, p.z1);
            bool any = false;
            for (int z = zb - (c == 0 ? r.extra_lo : 0); z < ze + (c == p.chunks - 1 ? r.extra_hi : 0); ++z) any = any || a.active[(size_t)z * p.strips + s];
            live += any;
            CHECK(any == (listed.count({s, c}) != 0), n);  // every live unit, no dead one
        }
    CHECK(live == p.units.size(), n);
    uint32_t longest = 0;
    for (int k = 0; k < 8; ++k) {
        CHECK(p.unit_start[k] <= p.unit_start[k + 1], n);
        longest = std::max(longest, p.unit_start[k + 1] - p.unit_start[k]);
        for (uint32_t i = p.unit_start[k]; r.by_chunk && i + 1 < p.unit_start[k + 1]; ++i)
            CHECK(((p.units[i] >> r.chunk_shift) & 0x1FFu) <= ((p.units[i + 1] >> r.chunk_shift) & 0x1FFu), n);
    }
    CHECK(p.unit_start[0] == 0 && p.unit_start[8] == p.units.size(), n);
    CHECK(longest == p.units_longest, n);
}

wv::MarchPlan units_case(const std::string& name, const Activity& a, const wv::UnitRules& r, int z0, int z1) {
    wv::MarchPlan p;
    p.z0 = z0;
    p.z1 = z1;
    p.strips = a.strips;
    p.nw = a.row_waves;
    p.zc = -1;  // (a plan without a list keeps what it had)
    p.chunks = -1;
    const bool ok = wv::plan_units(p, r, a.active.data(), a.bits.data());
    CHECK(ok == !p.units.empty(), name.c_str());
    begin_case(name);
    if (!ok) {
        CHECK(p.zc == -1 && p.chunks == -1, name.c_str());
        out << "{\"list\": false}";
        return p;
    }
    check_list(name, p, r, a);
    char frac[40];
    std::snprintf(frac, sizeof frac, "%.17g", p.live_frac);
    out << "{\"list\": true, \"zc\": " << p.zc << ", \"chunks\": " << p.chunks << ", \"unit_start\": " << list_of(p.unit_start, 9)
        << ", \"units_longest\": " << p.units_longest << ", \"live_frac\": " << frac << ", \"n\": " << p.units.size()
        << ", \"fnv1a\": " << hex(fnv1a(kFnvBasis, p.units.data(), p.units.size() * sizeof(uint32_t)));
    if (p.units.size() <= 48) out << ", \"units\": " << list_of(p.units.data(), (int)p.units.size());
    out << "}";
    return p;
}

// a room through both marches: the two-step march with and without spans, the three-step march (whose entries always carry spans; without
// them a list must be the same units with the rows' full width, which is checked against the list with spans)
void room_cases(const std::string& name, const Room& room, int pair_height, bool pair_search, int triple_height, bool triple_search,
                int lo = 0, int hi = 0, int64_t slots_per_xcd = 0) {
    // 64 columns: 8 waves of 16-byte lanes, 16 waves of 8-byte lanes (scaled down from 128 / 64 doubles a wave)
    const Activity a2 = activity_of(room, room.nx / 8), a3 = activity_of(room, room.nx / 16);
    const int z0 = lo ? 2 : 0, z1 = room.nz - (hi ? 2 : 0);
    wv::UnitRules r2 = two_step_rules(a2, room.nz, pair_height, pair_search, true), r3 = three_step_rules(a3, room.nz, triple_height, triple_search, lo, hi);
    if (slots_per_xcd) r2.slots_per_xcd = r3.slots_per_xcd = slots_per_xcd;
    units_case(name + "/two-step/spans", a2, r2, z0 - (lo ? 1 : 0), z1 + (hi ? 1 : 0));
    r2.spans = false;
    units_case(name + "/two-step/rows", a2, r2, z0 - (lo ? 1 : 0), z1 + (hi ? 1 : 0));
    const wv::MarchPlan with = units_case(name + "/three-step/spans", a3, r3, z0, z1);
    r3.spans = false;
    wv::MarchPlan without;
    without.z0 = z0;
    without.z1 = z1;
    without.strips = a3.strips;
    const bool ok = wv::plan_units(without, r3, a3.active.data(), a3.bits.data());
    const std::string n = name + "/three-step/rows";
    CHECK(ok == !with.units.empty() && without.units.size() == with.units.size(), n.c_str());
    if (ok) {
        check_list(n, without, r3, a3);
        CHECK(without.zc == with.zc && without.chunks == with.chunks && without.units_longest == with.units_longest, n.c_str());
        for (size_t i = 0; i < with.units.size() && i < without.units.size(); ++i) CHECK(without.units[i] == (with.units[i] & ((1u << 23) - 1u)), n.c_str());
        CHECK(without.live_frac == (double)((uint64_t)with.units.size() * a3.row_waves) / ((double)a3.strips * with.chunks * a3.row_waves), n.c_str());
    }
}

}  // namespace

int main() {
    // ---- windows: the two-step WIDE march (cap 8), wv_tuning::pair_split_rows (4 by default, 3, 2), the three-step march (12 / 8 waves,
    // full windows first and equal shares)
    for (int cap : {8, 4, 3, 2}) windows_case("split_row/cap" + std::to_string(cap), [cap](int row, uint8_t(*win)[wv::kMarchMaxWindows], int* widest) { return wv::split_row(row, cap, win, widest); });
    for (int max_waves : {12, 8})
        for (bool full_first : {true, false})
            windows_case(std::string("triple_windows/") + (full_first ? "full_first" : "equal") + std::to_string(max_waves),
                         [=](int row, uint8_t(*win)[wv::kMarchMaxWindows], int* widest) { return wv::triple_windows(row, win, widest, full_first, max_waves); });
    {  // too long: 8 windows of 8 store 7 + 6 * 6 + 7 = 50 waves
        uint8_t win[4][wv::kMarchMaxWindows];
        int widest = 0;
        CHECK(wv::split_row(50, 8, win, &widest) == 8 && wv::split_row(51, 8, win, &widest) == -1, "split_row/too long");
        CHECK(wv::triple_windows(200, win, &widest, true, 12) == -1 && wv::triple_windows(200, win, &widest, false, 12) == -1, "triple_windows/too long");
    }
    // ---- chunks of a full mesh.  row_waves_pair: waves of 16-byte lanes in a row (1024 doubles: 8, 1024 floats: 4)
    chunks_case("chunks/bench_f64/two-step", kTwoStep, 1024, 8, 1024, 1, 0);
    chunks_case("chunks/bench_f32/two-step", kTwoStep, 1024, 4, 1024, 1, 0);
    for (int lb : {8, 16}) {
        chunks_case("chunks/bench_f64/three-step/lanes" + std::to_string(lb), kThreeStep, 1024, 8, 1024, 1, 0, lb);
        chunks_case("chunks/bench_f32/three-step/lanes" + std::to_string(lb), kThreeStep, 1024, 4, 1024, 1, 0, lb);
    }
    for (int n : {256, 512, 768}) {
        chunks_case("chunks/cube" + std::to_string(n) + "/two-step", kTwoStep, n, n / 128, n, 1, 0);
        for (int lb : {8, 16}) chunks_case("chunks/cube" + std::to_string(n) + "/three-step/lanes" + std::to_string(lb), kThreeStep, n, n / 128, n, 1, 0, lb);
    }
    chunks_case("chunks/wide_row_1280/two-step", kTwoStep, 320, 10, 320, 1, 0);
    // Geometries where the rounds and the warm-up planes pull opposite ways, so that the count of warm-up planes decides.  80 strips of 8
    // waves through 640 planes, 256 slots: a plane more (two-step) / a plane less (three-step) settles on other chunks.
    chunks_case("chunks/320_rows_640_planes/two-step", kTwoStep, 320, 8, 640, 1, 0);
    chunks_case("chunks/320_rows_640_planes/three-step", kThreeStep, 320, 8, 640, 1, 0, 16);
    // Two rounds wanted: 80 strips of 4 waves through 320 planes (two-step: 17 / 27 / 54 planes a chunk with 2 / 3 / 4 warm-up planes),
    // 112 strips of 8 waves through 128 planes (three-step: 15 / 32 / 64 with 3 / 4 / 5) -- a plane more or less either way
    chunks_case("chunks/320_rows_320_planes/rounds2/two-step", kTwoStep, 320, 4, 320, 2, 0);
    chunks_case("chunks/448_rows_128_planes/rounds2/three-step", kThreeStep, 448, 8, 128, 2, 0, 16);
    for (int owned : {128, 508})
        for (int want : {1, 2}) {
            const std::string tag = "chunks/slab" + std::to_string(owned) + "/rounds" + std::to_string(want);
            chunks_case(tag + "/two-step", kTwoStep, 1024, 8, owned, want, 0);
            chunks_case(tag + "/three-step", kThreeStep, 1024, 8, owned, want, 0, 16);
            chunks_case(tag + "/two-step/256", kTwoStep, 256, 2, owned, want, 0);
            chunks_case(tag + "/three-step/256", kThreeStep, 256, 2, owned, want, 0, 8);
        }
    chunks_case("chunks/thin/two-step", kTwoStep, 512, 4, 5, 2, 0);
    chunks_case("chunks/thin/three-step", kThreeStep, 512, 4, 5, 2, 0, 8);
    chunks_case("chunks/forced_over/two-step", kTwoStep, 512, 4, 100, 1, 1000);
    chunks_case("chunks/forced_over/three-step", kThreeStep, 512, 4, 100, 1, 1000, 8);
    chunks_case("chunks/forced/two-step", kTwoStep, 512, 4, 100, 1, 5);
    chunks_case("chunks/forced/three-step", kThreeStep, 512, 4, 100, 1, 5, 8);

    // ---- unit lists.  Rooms of 64 x 256 x 200 nodes (64 strips); heights as the engine starts from (wv_tuning::pair_unit_planes = 32,
    // + 8 for the three-step march)
    const int nx = 64, ny = 256, nz = 200;
    const Room sphere{nx, ny, nz, [=](int x, int y, int z) {
                          const double dx = (x + 0.5) / nx - 0.5, dy = (y + 0.5) / ny - 0.5, dz = (z + 0.5) / nz - 0.5;
                          return dx * dx + dy * dy + dz * dz < 0.25;
                      }};
    const Room two_rooms{nx, ny, nz, [](int x, int y, int z) {  // (tests/test_tile_lists.py, _two_rooms, in this mesh's proportions)
                             return (z >= 25 && z < 166 && y >= 26 && y < 230 && x >= 2 && x < 26) || (z >= 50 && z < 125 && y >= 51 && y < 192 && x >= 43 && x < 60);
                         }};
    const Room one_wave{nx, ny, nz, [](int x, int y, int z) { return x >= 16 && x < 24 && y >= 40 && y < 200 && z >= 10 && z < 150; }};
    const Room ell{nx, ny, nz, [](int x, int y, int z) { return z >= 4 && z < 190 && y >= 8 && y < 250 && x >= 3 && x < 61 && (y < 90 || x < 20); }};
    const Room empty{nx, ny, nz, [](int, int, int) { return false; }};
    const Room full{nx, ny, nz, [](int, int, int) { return true; }};
    room_cases("units/sphere", sphere, 32, true, 40, true);
    room_cases("units/two_rooms", two_rooms, 32, true, 40, true);
    room_cases("units/one_wave", one_wave, 32, true, 40, true);
    room_cases("units/ell", ell, 32, true, 40, true);
    room_cases("units/empty", empty, 32, true, 40, true);
    room_cases("units/full", full, 32, true, 40, true);
    room_cases("units/sphere/short_units", sphere, 25, false, 40, true);  // a full mesh's chunks shorter than pair_unit_planes: no search
    room_cases("units/ell/slab_lo", ell, 32, true, 40, true, 1, 0);      // a slab's range, the extra plane at one end ...
    room_cases("units/ell/slab_both", ell, 32, true, 40, true, 1, 1);    // ... and at both
    room_cases("units/sphere/slab_both", sphere, 32, true, 40, true, 1, 1);
    room_cases("units/sphere/forced_7_chunks", sphere, 32, true, std::max(4, (nz + 6) / 7), false);  // wv_tuning::triple_chunks = 7
    // fewer slots than units in a run: several rounds, where the warm-up planes tip the choice of height.  The first two settle elsewhere
    // with a plane more of them (two-step, 3 -> 4) / a plane less (three-step, 4 -> 3); the third with a plane less (two-step: 32 -> 38
    // planes) / a plane more (three-step: 32 -> 38); the fourth with a plane more (two-step: 25 -> 38) and, three-step, either way (38 -> 25 /
    // 30).  Together: either set, either direction.
    room_cases("units/two_rooms/8_slots", two_rooms, 40, true, 40, true, 0, 0, 8);
    room_cases("units/ell/16_slots", ell, 40, true, 40, true, 0, 1, 16);
    room_cases("units/ell/8_slots_from_36", ell, 36, true, 36, true, 0, 0, 8);
    room_cases("units/one_wave/5_slots", one_wave, 32, true, 32, true, 0, 0, 5);
    // The two searches end at different heights: the two-step one at 5/4 of the height chosen so far, the three-step one at 5/4 of the
    // height it started from (UnitRules::search_follows).  Here a first clear win at 24 planes ends the two-step search at 30, and the
    // three-step search goes on to find 40.
    room_cases("units/sphere/40_slots", sphere, 32, true, 32, true, 0, 0, 40);
    {  // strip by strip (wv_tuning::pair_units_by_chunk = 0: no search either)
        const Activity a = activity_of(sphere, nx / 8);
        units_case("units/sphere/two-step/by_strip", a, two_step_rules(a, nz, 32, false, true, false), 0, nz);
    }
    {  // a room whose live planes end inside the extra plane only: the unit at that end is live for the three-step march alone
        const Room low{nx, ny, nz, [](int x, int y, int z) { return z < 2 && y >= 16 && y < 64 && x < 30; }};
        room_cases("units/low/slab_lo", low, 32, true, 40, true, 1, 0);
    }
    {  // too many strips for an entry's bits (2^16 / 2^14), in a mesh of 8 planes
        Activity a;
        a.row_waves = 8;
        for (int strips : {1 << 16, (1 << 16) - 1, 1 << 14, (1 << 14) - 1}) {
            a.strips = strips;
            a.active.assign((size_t)8 * strips, 1);
            a.bits.assign((size_t)8 * strips, 0x3C);
            units_case("units/strips" + std::to_string(strips) + "/two-step", a, two_step_rules(a, 8, 8, false, true), 0, 8);
            units_case("units/strips" + std::to_string(strips) + "/three-step", a, three_step_rules(a, 8, 8, false, 0, 0), 0, 8);
        }
    }
    {  // 512 chunks or more: one strip through 4 090 planes.  Units of 8 planes are 512 chunks: no list.  A search around 10 planes finds 8
       // the clear win: the two-step search passes over it and settles on 9, the three-step search takes it and ends without a list.
        Activity a;
        a.strips = 1;
        a.row_waves = 8;
        a.active.assign(4090, 1);
        a.bits.assign(4090, 0xFF);
        auto roomy = [](wv::UnitRules r) {  // (every unit in one round: a unit's cost is its height + warm-up planes)
            r.slots_per_xcd = 512;
            return r;
        };
        units_case("units/chunks512/two-step", a, roomy(two_step_rules(a, 4090, 8, false, true)), 0, 4090);
        units_case("units/chunks512/three-step", a, roomy(three_step_rules(a, 4090, 8, false, 0, 0)), 0, 4090);
        units_case("units/chunks512/two-step/search", a, roomy(two_step_rules(a, 4090, 10, true, true)), 0, 4090);
        units_case("units/chunks512/three-step/search", a, roomy(three_step_rules(a, 4090, 10, true, 0, 0)), 0, 4090);
        wv::UnitRules swapped = roomy(three_step_rules(a, 4090, 10, true, 0, 0));
        swapped.search_in_limit = true;  // (the flag is what tells the two searches apart)
        wv::MarchPlan p;
        p.z1 = 4090;
        p.strips = 1;
        CHECK(wv::plan_units(p, swapped, a.active.data(), a.bits.data()) && p.zc == 9, "units/chunks512/search_in_limit");
    }
    std::printf("{\n%s\n}\n", out.str().c_str());
    if (failures) {
        std::printf("%d CHECKS FAILED\n", failures);
        return 1;
    }
    std::printf("MARCH PLAN OK\n");
    return 0;
}

// march_plan.h -- what a march (pair_kernels.hip.h, triple_kernels.hip.h) is launched with, and the integer logic that decides it:
// how a long row is cut into windows, how many chunks along z a full mesh takes, the work list of a room that leaves much of its mesh
// outside.  One set of functions for the two-step and the three-step march; what differs between them arrives as numbers.
//
// Host only: nothing but the standard library, so that tests/cpp/march_plan_test.cpp exercises it without a GPU.  The engine gathers the
// activity arrays, reads wv_tuning, fills in the parameters and uploads the list (engine_pair.hip.h, engine_triple.hip.h).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace wv {

constexpr int kMarchMaxWindows = 8;  // workgroups side by side on one row (PairArgs / TripleArgs: a byte per window in each win_* word)

struct MarchPlan {
    int z0 = 0, z1 = 0;        // the planes the march produces
    int nw = 1;                // waves per workgroup
    int strips = 0;            // strips of four rows
    int zc = 0, chunks = 1;    // planes per chunk, chunks along z
    int windows = 0;           // workgroups side by side per row (0: one)
    uint8_t win[4][kMarchMaxWindows] = {};  // per window: first wave run, waves run, first wave stored, end of the stored waves
    // sparse rooms: the work list (plan_units), empty = every unit by the arithmetic mapping; XCD k's run starts at unit_start[k]
    std::vector<uint32_t> units;
    uint32_t unit_start[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t units_longest = 0;
    double live_frac = 1.0;    // live waves of listed units / all waves of all units
};

// A row of `row_waves` waves as windows of at most `cap` waves, one halo wave on every interior side, as many full windows as the row
// gives and a short one for the rest.  win[0..3][k] as in MarchPlan.  Returns the number of windows, -1 if the row is too long for
// kMarchMaxWindows of them; *widest = the most waves any window runs.
inline int split_row(int row_waves, int cap, uint8_t win[4][kMarchMaxWindows], int* widest) {
    int n = 0, at = 0;
    *widest = 0;
    while (at < row_waves && n < kMarchMaxWindows) {
        const int lo_halo = at > 0 ? 1 : 0;
        int end = at + cap - lo_halo;                    // storing [at, end) with no halo above ...
        if (end < row_waves) end -= 1;                   // ... or one wave less and a halo wave
        end = std::max(at + 1, std::min(end, row_waves));  // (caps below 3 leave an interior window nothing but its halo waves: one wave then)
        const int first = at - lo_halo, count = end + (end < row_waves ? 1 : 0) - first;
        win[0][n] = (uint8_t)first;
        win[1][n] = (uint8_t)count;
        win[2][n] = (uint8_t)at;
        win[3][n] = (uint8_t)end;
        *widest = std::max(*widest, count);
        ++n;
        at = end;
    }
    return at < row_waves ? -1 : n;
}

// How a row of `row_waves` waves is shared out by the three-step march: windows of at most `max_waves` waves (triple_max_waves), one halo
// wave on every interior side.  `full_first`: as many full workgroups (12 waves: three on every SIMD) as the row gives and one short one
// for the rest -- two short ones share a CU -- instead of equal shares (16 waves: 12 + 6 instead of 9 + 9, whose 9 waves are
// 3 + 2 + 2 + 2 on a CU's SIMDs and as slow as 12).
// Returns the number of windows (0: the row is one workgroup), -1 if the row is too long; *widest = waves per workgroup.
inline int triple_windows(int row_waves, uint8_t win[4][kMarchMaxWindows], int* widest, bool full_first = true, int max_waves = 12) {
    *widest = row_waves;
    if (row_waves <= max_waves) return 0;
    if (full_first) return split_row(row_waves, max_waves, win, widest);
    int n = 2;  // the widest window stores ceil(row_waves / n) waves and has a halo wave on one side (n = 2) or two
    *widest = 0;
    while (n <= kMarchMaxWindows && (row_waves + n - 1) / n + (n > 2 ? 2 : 1) > max_waves) ++n;
    if (n > kMarchMaxWindows) return -1;
    for (int k = 0; k < n; ++k) {
        const int lo = row_waves * k / n, hi = row_waves * (k + 1) / n;
        const int first = lo - (k > 0 ? 1 : 0), last = hi + (k + 1 < n ? 1 : 0);
        win[0][k] = (uint8_t)first;
        win[1][k] = (uint8_t)(last - first);
        win[2][k] = (uint8_t)lo;
        win[3][k] = (uint8_t)hi;
        if (last - first > *widest) *widest = last - first;
    }
    return n;
}

// Chunks along z of a full mesh's march over [p.z0, p.z1): sets p.zc and p.chunks.  `slots` workgroups are what the chip holds at once
// (256 CUs x workgroups per CU); chunks are chosen so that the `wgs_per_chunk` x chunks workgroups fill whole rounds of that, weighed
// against the `warmup` planes every chunk recomputes or loads before its first output plane.  The search goes up to chunks of
// `search_planes` planes; `forced` > 0 (wv_tuning) sets the number instead, down to chunks of `least_planes` planes.
// `want_rounds` = 2, a slab with a neighbour: the exchange of its t+1 faces is to run under the march, and whatever carries it (RCCL's
// send / receive kernels, the runtime's copy kernels) needs a CU -- a march of ONE round holds every register of every CU until all its
// workgroups retire together at the end, and the exchange would start after it.  At least two rounds then: the first round's end is
// where the exchange gets in.  (... where that costs little: a mesh that fills two rounds only with much shorter chunks keeps the
// unconstrained choice)
inline void choose_chunks(MarchPlan& p, int64_t wgs_per_chunk, int64_t slots, int warmup, int search_planes, int least_planes,
                          int64_t want_rounds, int forced) {
    const int owned = p.z1 - p.z0;
    int chunks = forced;
    if (chunks <= 0) {
        double best[2] = {0, 0};
        int at[2] = {0, 0};  // [0] any number of rounds, [1] at least `want_rounds`
        for (int c = 1; c <= std::max(1, owned / search_planes) && c <= 256; ++c) {
            const int64_t wgs = wgs_per_chunk * c;
            const int64_t rounds = (wgs + slots - 1) / slots;
            const double zc = (double)((owned + c - 1) / c);
            const double cost = (double)(rounds * slots) / (double)wgs * (zc + (double)warmup) / zc;
            for (int k = 0; k < 2; ++k)
                if ((k == 0 || rounds >= want_rounds) && (at[k] == 0 || cost < best[k] - 1e-9)) {
                    best[k] = cost;
                    at[k] = c;
                }
        }
        chunks = (at[1] && best[1] <= 1.06 * best[0]) ? at[1] : at[0];
    }
    chunks = std::max(1, std::min(chunks, std::max(1, owned / least_planes)));
    p.zc = (owned + chunks - 1) / chunks;
    p.chunks = (owned + p.zc - 1) / p.zc;
}

// A sparse room's units go to the eight XCDs as runs of neighbouring strips with about the same number of units each: run k ends where
// the strips so far hold k + 1 eighths of all `total` units (per_strip[s]: units of strip s).  end[k] = the strip after run k's last;
// returns the units of the longest run.
inline uint64_t eight_runs(const std::vector<uint32_t>& per_strip, uint64_t total, int end[8]) {
    uint64_t longest = 0, so_far = 0, start = 0;
    int sidx = 0;
    for (int k = 0; k < 8; ++k) {
        const uint64_t want = total * (uint64_t)(k + 1) / 8;  // cumulative share of XCDs 0 .. k
        while (sidx < (int)per_strip.size() && (so_far < want || k == 7)) so_far += per_strip[(size_t)sidx++];
        end[k] = sidx;
        longest = std::max(longest, so_far - start);
        start = so_far;
    }
    return longest;
}

// What plan_units needs to know about the march whose list it makes.
struct UnitRules {
    int nz;                  // planes of the activity arrays
    int row_waves;           // waves of a row (at most 16: the masks' width)
    int warmup;              // planes a unit marches before its first output plane
    int halo;                // planes either side of a unit's own that it reads or hands on (the span of its live waves)
    int extra_lo, extra_hi;  // 1: a unit at that end of [z0, z1) also stores on the plane beyond it (a slab's three-step march)
    int64_t slots_per_xcd;   // workgroups an XCD runs at one time
    int start_height;        // planes to a unit ...
    bool search;             // ... or the best of the heights within a quarter of that
    bool search_in_limit;    // the search passes over heights that make 512 chunks or more (else: such a choice ends in "no list")
    bool search_follows;     // the search's upper end is 5/4 of the height chosen so far: a win below start_height ends it sooner, one
                             // above carries it further (else: 5/4 of start_height)
    int chunk_shift, first_shift, span_shift;  // bit positions in an entry: strip | chunk << . | first wave << . | waves - 1 << .
    bool spans;              // entries carry their unit's live waves (else: every wave of the row)
    bool by_chunk;           // an XCD's run is ordered chunk by chunk (else strip by strip)
};

// The work list of a room that leaves much of its mesh outside: a unit of the march (a strip of four rows through one chunk of planes)
// without a single node to update produces nothing but the zeros its outputs already hold, so only the other units are launched -- each
// XCD a run of neighbouring strips with about the same number of units.
// `active[z * strips + s]`: strip s of plane z holds a node to update; `wave_bits[z * strips + s]`: bit w set when wave w of those rows
// holds anything but `none` nodes (read only where r.spans).  Fills p.units, p.unit_start, p.units_longest, p.live_frac and sets p.zc /
// p.chunks to the units' height; returns false and leaves p without a list where there is none to be had (too many strips or chunks for
// an entry's bits, rows wider than the masks, nothing live).
inline bool plan_units(MarchPlan& p, const UnitRules& r, const uint8_t* active, const uint16_t* wave_bits) {
    p.units.clear();
    const int owned = p.z1 - p.z0, strips = p.strips;
    if (strips >= (1 << r.chunk_shift) || r.row_waves > 16) return false;
    auto live = [&](int sidx, int c, int height) {
        const int zb = p.z0 + c * height, ze = std::min(zb + height, p.z1);
        for (int z = zb - (zb == p.z0 ? r.extra_lo : 0); z < ze + (ze == p.z1 ? r.extra_hi : 0); ++z)
            if (active[(size_t)z * strips + sidx]) return true;
        return false;
    };
    // How many planes to a unit?  About start_height, and among the heights near it the one whose units fill the chip's workgroup slots in
    // the fewest, fullest rounds: an XCD runs slots_per_xcd of its units at a time, a round of them takes (height + warm-up planes), and a
    // last round with two units in it costs as much as a full one -- the concert hall at 1 600 Hz made 1 538 two-step units of 32 planes
    // for 256 slots: six rounds and one nearly empty.
    auto rounds_cost = [&](int height) -> double {
        const int n_chunks = (owned + height - 1) / height;
        std::vector<uint32_t> per_strip((size_t)strips, 0u);
        uint64_t units = 0;
        for (int sidx = 0; sidx < strips; ++sidx)
            for (int c = 0; c < n_chunks; ++c) {
                const bool any = live(sidx, c, height);
                per_strip[(size_t)sidx] += any;
                units += any;
            }
        if (!units) return 0.0;
        int end[8];
        const uint64_t longest = eight_runs(per_strip, units, end);
        return (double)((longest + (uint64_t)r.slots_per_xcd - 1) / (uint64_t)r.slots_per_xcd) * (double)(height + r.warmup);
    };
    int zc = r.start_height;
    if (r.search) {
        double best = rounds_cost(zc);
        for (int height = r.start_height * 3 / 4; height <= (r.search_follows ? zc : r.start_height) * 5 / 4; ++height) {
            if (height < 8 || height > owned || (r.search_in_limit && (owned + height - 1) / height >= (1 << 9))) continue;
            const double cost = rounds_cost(height);
            if (cost > 0 && cost < best * 0.97) {  // (only a clear win moves the height)
                best = cost;
                zc = height;
            }
        }
    }
    const int chunks = (owned + zc - 1) / zc;
    if (chunks >= (1 << 9)) return false;  // (9 bits of a list entry)
    // Which waves of a row does a unit need?  Those between the first and the last column block that holds anything but `none` nodes in
    // the unit's rows +- a strip and planes +- halo (all it reads, produces or hands on): beyond them every field is zero, which is what a
    // missing neighbour counts as (pair_march_kernel / triple_march_kernel, unit lists).
    std::vector<std::vector<uint32_t>> of_strip((size_t)strips);
    uint64_t total = 0, live_waves = 0;
    for (int sidx = 0; sidx < strips; ++sidx)
        for (int c = 0; c < chunks; ++c) {
            if (!live(sidx, c, zc)) continue;
            uint32_t entry = (uint32_t)sidx | ((uint32_t)c << r.chunk_shift), span = (uint32_t)r.row_waves;
            if (r.spans) {
                const int zb = p.z0 + c * zc, ze = std::min(zb + zc, p.z1);
                uint32_t bits = 0;
                for (int z = std::max(0, zb - r.halo); z < std::min(r.nz, ze + r.halo); ++z)
                    for (int ss = std::max(0, sidx - 1); ss <= std::min(strips - 1, sidx + 1); ++ss) bits |= wave_bits[(size_t)z * strips + ss];
                const uint32_t lo = std::min((uint32_t)__builtin_ctz(bits | (1u << 31)), (uint32_t)r.row_waves - 1u);
                const uint32_t hi = std::min(32u - (uint32_t)__builtin_clz(bits | 1u), (uint32_t)r.row_waves);
                span = hi > lo ? hi - lo : 1u;
                entry |= (lo << r.first_shift) | ((span - 1u) << r.span_shift);
            }
            of_strip[(size_t)sidx].push_back(entry);
            live_waves += span;
            ++total;
        }
    if (!total) return false;
    p.live_frac = (double)live_waves / ((double)strips * chunks * r.row_waves);
    p.units.reserve((size_t)total);
    std::vector<uint32_t> per_strip((size_t)strips);
    for (int s = 0; s < strips; ++s) per_strip[(size_t)s] = (uint32_t)of_strip[(size_t)s].size();
    int end[8];
    p.units_longest = (uint32_t)eight_runs(per_strip, total, end);
    for (int k = 0, sidx = 0; k < 8; ++k) {
        p.unit_start[k] = (uint32_t)p.units.size();
        const size_t first = p.units.size();
        for (; sidx < end[k]; ++sidx) p.units.insert(p.units.end(), of_strip[(size_t)sidx].begin(), of_strip[(size_t)sidx].end());
        // An XCD takes its units chunk by chunk, the strips of a chunk side by side -- as the arithmetic mapping of a full mesh does -- so
        // that the workgroups it runs at one time are NEIGHBOURING strips at the same planes and the ring rows two of them both load meet
        // in its L2.  (Until round 3 the order was strip by strip: the 32 workgroups of an XCD were 29 chunks of one strip and shared
        // nothing; every ring row came from HBM -- the concert hall's march ran at 3.3 TB/s where a box's runs at 5.85.)
        if (r.by_chunk) {
            const int shift = r.chunk_shift;
            std::stable_sort(p.units.begin() + (std::ptrdiff_t)first, p.units.end(),
                             [shift](uint32_t a, uint32_t b) { return ((a >> shift) & 0x1FFu) < ((b >> shift) & 0x1FFu); });
        }
    }
    p.unit_start[8] = (uint32_t)p.units.size();
    p.zc = zc;
    p.chunks = chunks;
    return true;
}

// The geometry fields PairArgs and TripleArgs share, from a plan; returns the launch's grid size.  `list`: the uploaded p.units (null
// where the plan has none: the arithmetic mapping).
template <typename Args>
unsigned fill_march_args(Args& a, const MarchPlan& p, const uint32_t* list) {
    a.nw = p.nw;
    a.zc = p.zc;
    a.chunks = p.chunks;
    a.strips = p.strips;
    a.strips_per_xcd = (p.strips + 7) / 8;
    a.windows = p.windows;
    for (int k = 0; k < p.windows; ++k) {
        a.win_first |= (uint64_t)p.win[0][k] << (8 * k);
        a.win_count |= (uint64_t)p.win[1][k] << (8 * k);
        a.win_store_lo |= (uint64_t)p.win[2][k] << (8 * k);
        a.win_store_hi |= (uint64_t)p.win[3][k] << (8 * k);
    }
    if (list) {
        a.unit_list = list;
        for (int k = 0; k < 9; ++k) a.list_start[k] = p.unit_start[k];
        return 8u * p.units_longest;
    }
    return 8u * (unsigned)a.strips_per_xcd * (unsigned)p.chunks * (unsigned)std::max(1, p.windows);
}

}  // namespace wv

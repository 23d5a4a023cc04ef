// snapshot_plan.h -- (host only, no HIP, nothing but the standard library) the integer logic of field snapshots
// (wv_set_snapshots, include/wayverb_amd.h): which steps are snapshot steps, how far a batch of steps may go before the
// next one, whether a box lies inside a mesh, and the dense output's shape and size -- and, for every plan that captures a box as a
// snapshot plan does (the accumulating plans of engine_staged.hip.h), the ONE statement of what every setter checks: the box of a plan,
// the four refusals all setters share, and the checks of frequencies, filter coefficients and physical constants that more than one has.
//
// A two-step pass never holds t+1 as a whole field, a three-step pass neither t+1 nor t+2, and a replayed graph covers a
// whole batch: a snapshot step has to be the END of a pass (of the batch, under graph replay).  engine_batch.hip.h ends its
// batches with snapshot_batch_limit at the last snapshot step the ring has a slot for and cuts the passes inside a batch at the
// ones before it; engine_snapshot.hip.h enqueues each capture behind the pass that produced the step.
// tests/cpp/snapshot_plan_test.cpp covers this file on the CPU.
#pragma once
#include <cstdint>
#include <limits>

namespace wv {

constexpr uint64_t kNoSnapshotStep = std::numeric_limits<uint64_t>::max();

// the box of wv_snapshot_plan: first node, nodes TAKEN and stride per axis
struct SnapshotBox {
    int32_t x0 = 0, y0 = 0, z0 = 0;
    int32_t nx = 0, ny = 0, nz = 0;
    int32_t sx = 1, sy = 1, sz = 1;
};

// one axis: `count` nodes from `first`, every `stride`-th, all of them inside [0, mesh)
inline bool snapshot_axis_valid(int64_t first, int64_t count, int64_t stride, int64_t mesh) {
    return first >= 0 && count >= 1 && stride >= 1 && first < mesh && first + (count - 1) * stride < mesh;
}

inline bool snapshot_box_valid(const SnapshotBox& b, int32_t mesh_nx, int32_t mesh_ny, int32_t mesh_nz) {
    return snapshot_axis_valid(b.x0, b.nx, b.sx, mesh_nx) && snapshot_axis_valid(b.y0, b.ny, b.sy, mesh_ny) &&
           snapshot_axis_valid(b.z0, b.nz, b.sz, mesh_nz);
}

// nodes taken from `extent` consecutive nodes at `stride`: the first, and every stride-th after it (0 for a bad stride)
inline int64_t snapshot_axis_count(int64_t extent, int64_t stride) {
    return (extent < 1 || stride < 1) ? 0 : (extent + stride - 1) / stride;
}

// elements / bytes of one dense [nz][ny][nx] float snapshot
inline uint64_t snapshot_elements(const SnapshotBox& b) {
    return (b.nx < 1 || b.ny < 1 || b.nz < 1) ? 0 : (uint64_t)b.nx * (uint64_t)b.ny * (uint64_t)b.nz;
}
inline uint64_t snapshot_bytes(const SnapshotBox& b) { return snapshot_elements(b) * sizeof(float); }

// the box of any wv_*_plan: they all begin with the same nine ints
template <typename Plan>
inline SnapshotBox plan_box(const Plan& p) {
    SnapshotBox b;
    b.x0 = p.x0, b.y0 = p.y0, b.z0 = p.z0;
    b.nx = p.nx, b.ny = p.ny, b.nz = p.nz;
    b.sx = p.sx, b.sy = p.sy, b.sz = p.sz;
    return b;
}

// the capture takes four nodes per lane where the rows allow 16-byte accesses on both sides (snapshot_kernels.hip.h)
inline bool gather_wide(const SnapshotBox& b) { return b.sx == 1 && b.x0 % 4 == 0 && b.nx % 4 == 0; }

// What every setter refuses a box and a period for, in the order they all ask; the sentences carry the setter's name.
enum PlanFault { kPlanStrides, kPlanPeriod, kPlanLeavesMesh, kPlanPlaneSize };
struct PlanSentences {
    const char* of[4];  // by PlanFault
};
#define WV_PLAN_SENTENCES(setter) \
    {{setter ": strides must be >= 1", setter ": period must be >= 1", setter ": the box leaves the mesh", setter ": more than 2^31 nodes per plane of the box"}}

// The sentence of the first of the faults `first` .. `last` that `plan` has, nullptr when it has none of them.  A setter with checks
// of its own between the shared ones asks in parts; kPlanPlaneSize (the capture kernel indexes a dense plane with 32 bits) takes a box
// that lies inside the mesh.
template <typename Plan>
inline const char* plan_refusal(const Plan& plan, int32_t mesh_nx, int32_t mesh_ny, int32_t mesh_nz, const PlanSentences& says,
                                PlanFault first = kPlanStrides, PlanFault last = kPlanPlaneSize) {
    const SnapshotBox b = plan_box(plan);
    const bool bad[4] = {b.sx < 1 || b.sy < 1 || b.sz < 1, plan.period < 1, !snapshot_box_valid(b, mesh_nx, mesh_ny, mesh_nz),
                         (uint64_t)b.nx * (uint64_t)b.ny >= (1ull << 31)};
    for (int f = first; f <= last; ++f)
        if (bad[f]) return says.of[f];
    return nullptr;
}

// finite: inside the largest double on both sides (a NaN fails both comparisons)
inline bool plan_finite(double v) { return v >= -std::numeric_limits<double>::max() && v <= std::numeric_limits<double>::max(); }
// n biquad sections (b0 b1 b2 a1 a2, as wv_biquad has them): every coefficient finite
template <typename Biquad>
inline bool biquads_finite(const Biquad* sections, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) {
        const Biquad& c = sections[i];
        if (!plan_finite(c.b0) || !plan_finite(c.b1) || !plan_finite(c.b2) || !plan_finite(c.a1) || !plan_finite(c.a2)) return false;
    }
    return true;
}
// a frequency in cycles per step a plan takes: 0 .. 0.5 (a NaN fails both comparisons)
inline bool frequency_valid(double cycles_per_step) { return cycles_per_step >= 0.0 && cycles_per_step <= 0.5; }
// mesh spacing, sample rate and ambient density: positive and finite
inline bool physical_constants_valid(double spacing, double sample_rate, double ambient_density) {
    return spacing > 0 && sample_rate > 0 && ambient_density > 0 && plan_finite(spacing) && plan_finite(sample_rate) && plan_finite(ambient_density);
}

// the smallest first_step + j * period (j = 0, 1, ...) that is >= from; kNoSnapshotStep when there is none in 64 bits
// (or for period 0, which wv_set_snapshots refuses)
inline uint64_t snapshot_next_step(uint64_t first_step, uint64_t period, uint64_t from) {
    if (period == 0) return kNoSnapshotStep;
    if (from <= first_step) return first_step;
    const uint64_t gap = from - first_step;
    const uint64_t j = gap / period + (gap % period != 0);
    if (j > (kNoSnapshotStep - first_step) / period) return kNoSnapshotStep;
    return first_step + j * period;
}

// is `step` a snapshot step of a plan set when the engine stood at `set_at` steps
inline bool snapshot_is_step(uint64_t first_step, uint64_t period, uint64_t set_at, uint64_t step) {
    return step >= set_at && step != kNoSnapshotStep && snapshot_next_step(first_step, period, step) == step;
}

// How many of `batch` steps the next batch may take from `steps_done` when `next` is the next snapshot step not yet
// taken: never past it.  next == steps_done means that snapshot is due BEFORE the batch (the engine takes it first and
// asks again with the one after it): the batch is then not cut.
inline uint64_t snapshot_batch_limit(uint64_t batch, uint64_t steps_done, uint64_t next) {
    if (next == kNoSnapshotStep || next <= steps_done) return batch;
    const uint64_t room = next - steps_done;
    return batch < room ? batch : room;
}

}  // namespace wv

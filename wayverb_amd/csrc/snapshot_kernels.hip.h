// snapshot_kernels.hip.h -- the capture kernel of field snapshots (wv_set_snapshots; engine_snapshot.hip.h launches it).
//
// snapshot_gather_kernel<Real, WIDE> reads a box of the stored (row-padded) field -- node (x, y, z) at (z * ny + y) * pitch + x --
// at the plan's strides, converts with the (float) cast pack_rows_kernel uses (a double rounds to nearest, a float is copied),
// and writes the dense float [nz][ny][nx] block into one slot of the device ring.  Lanes run along x, rows follow each other in
// address order (grid x over a dense plane, grid y over the planes: 32-bit index arithmetic, one division per item).  No LDS, no scratch,
// no branch on data: the only branches are the bounds of the two stride loops.
//
//   WIDE   (sx == 1, x0 and nx multiples of 4; the engine decides) four nodes per lane: 16-byte stores, and 16-byte loads -- one
//          per lane from a float field, two from a double field (rows start on a tile boundary of 1 KiB, so x0 % 4 == 0 is all the
//          alignment either needs)
//   !WIDE  one node per lane.  With sx > 1 this is a strided gather: every 128-byte line of a row is touched anyway until sx
//          exceeds a line, so the field side costs what a dense read of the box's rows costs and the float side is dense
//
// Traffic bound: field lines touched + 4 bytes per node taken.  A 512^2 plane of doubles is 2 MiB in and 1 MiB out.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace wv {

template <typename Real>
struct SnapshotArgs {
    const Real* field;    // the stored field that holds the step
    float* dst;           // [nz][ny][nx] dense
    int64_t pitch;        // elements per stored row
    int32_t mesh_ny;      // rows per stored plane
    int32_t x0, y0, z0;
    int32_t nx, ny, nz;   // nodes taken
    int32_t sx, sy, sz;
};

template <typename Real, bool WIDE>
__global__ void __launch_bounds__(256) snapshot_gather_kernel(const SnapshotArgs<Real> a) {
    typedef Real RealV2 __attribute__((ext_vector_type(2)));
    typedef Real RealV4 __attribute__((ext_vector_type(4)));
    typedef float FloatV4 __attribute__((ext_vector_type(4)));
    // x of the grid strides over the items of one dense plane (32-bit arithmetic, one division), y over the planes
    const uint32_t per_row = WIDE ? (uint32_t)a.nx / 4 : (uint32_t)a.nx;  // lanes' items per output row
    const uint32_t n = per_row * (uint32_t)a.ny;
    const int64_t plane_floats = (int64_t)a.nx * a.ny;
    for (int32_t zz = (int32_t)blockIdx.y; zz < a.nz; zz += (int32_t)gridDim.y) {
        const Real* plane = a.field + ((int64_t)(a.z0 + (int64_t)zz * a.sz) * a.mesh_ny + a.y0) * a.pitch + a.x0;
        float* out_plane = a.dst + (int64_t)zz * plane_floats;
        for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
            const uint32_t yy = i / per_row;
            const uint32_t c = i - yy * per_row;
            const Real* src = plane + (int64_t)yy * a.sy * a.pitch;
            if (WIDE) {
                FloatV4 out;
                if (sizeof(Real) == 4) {
                    const RealV4 v = *reinterpret_cast<const RealV4*>(src + 4 * c);
                    out = FloatV4{(float)v.x, (float)v.y, (float)v.z, (float)v.w};
                } else {
                    const RealV2 lo = *reinterpret_cast<const RealV2*>(src + 4 * c);
                    const RealV2 hi = *reinterpret_cast<const RealV2*>(src + 4 * c + 2);
                    out = FloatV4{(float)lo.x, (float)lo.y, (float)hi.x, (float)hi.y};
                }
                *reinterpret_cast<FloatV4*>(out_plane + 4 * (int64_t)i) = out;
            } else {
                out_plane[i] = (float)src[(int64_t)c * a.sx];
            }
        }
    }
}

}  // namespace wv

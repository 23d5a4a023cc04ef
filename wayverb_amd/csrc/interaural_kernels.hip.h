// interaural_kernels.hip.h -- the capture and the fold kernel of interaural maps (wv_set_interaural; engine_snapshot.hip.h launches
// the capture, engine_interaural.hip.h the fold).
//
// ear_gather_kernel<Real> is the third kind of capture beside snapshot_gather_kernel and intensity_gather_kernel, with the former's
// index arithmetic (grid x over a dense plane, grid y over the planes, stride loops, 32-bit indices, one division per item): per node
// taken by the box it reads the stored (row-padded) field at the node plus ear_a and at the node plus ear_b -- two element offsets the
// host made of the ears, the pitch and the rows per plane -- converts with the (float) cast, and writes two dense float planes
// stage[slot][2][B].  No LDS, no scratch, no branch on data.  The setter has checked that every node read lies on the mesh.
//
// interaural_fold_kernel<SMAX, LMAX> folds the first t staged captures, which are captures number first, first + 1, ... since the
// plan was set, into the per-node state.  Per node and capture c, in capture order (include/wayverb_amd.h has the contract):
//
//     mag = fmaxf(fabsf(a), fabsf(b));  if (onset == NONE && mag >= thr) onset = c
//     xa = cascade(a), xb = cascade(b)          (decay_bands_fold_kernel's section, one state per ear, the coefficients shared)
//     if (onset == NONE) { pre[0] = pre[0] + xa * xa;  pre[1] = pre[1] + xb * xb; }
//     else { w = interaural_bin(c - onset);  Ea[w] += xa * xa;  Eb[w] += xb * xb;  C[w][L] += xa * xb;
//            for l = 1 .. L:  C[w][L + l] += xa(c - l) * xb;  C[w][L - l] += xb(c - l) * xa; }
//
// every product and every sum rounded on its own (-ffp-contract=off), so that a NumPy loop over the snapshots of the two ear planes
// (wayverb_amd/interaural.py: interaural_fold) reproduces all of it bit for bit.  Every sum is a chain of its own, so the ORDER IN
// WHICH THE SUMS ARE VISITED is free, and that is what keeps the kernel out of scratch:
//   - lanes run along the dense node index, one node per lane; a lane reads its 2 t staged floats once (fold_parts.hip.h: stage_read;
//     the onset rule is its onset_update), runs both ears through the cascade and keeps the filtered samples of this fold BEHIND the
//     L samples before it in one register array per ear, x[LMAX + T]: the earlier sample of capture j at lag l is x[LMAX + j - l], an
//     index made of two unrolled loop counters.  Nothing is indexed by a value, nothing is shifted
//   - the sums are taken in passes: Ea, Eb and C[0] first, then the lags in chunks of kInterauralLagChunk on either side (eight sums).
//     A pass walks the captures in order with ONE bin held (arrival_fold_kernel's form: the bin differs from lane to lane, never
//     decreases, and is stored and reloaded only where it changes).  The samples are in registers: no pass reads the stage again
//   - the L samples before the fold come from the history double[2][L][B], in which capture c lies in slot c % L (a ring: what a fold
//     writes is its last min(t, L) samples, wherever they fall); slots no capture has reached hold the +0.0 they were set to
//   - LMAX (0, 4, 8, 16: the engine takes the smallest that holds L) sizes the arrays; SMAX is 0 (no filter: the samples are exactly
//     the floats and are kept as floats, half the registers) or 4 (n_sections of them run, a wave-uniform bound).  L, n_sections,
//     the edges and `first` are kernel arguments and the coefficients are reached through a __restrict__ pointer with indices that hold
//     no lane: all of them live in scalar registers
// No LDS, no atomics, no scratch in any instance (profiles/r23/interaural_kernel_resources.txt); the tail of B is a bounds check.
//
// Traffic model (interaural_plan.h: interaural_fold_traffic) -- a model until measured.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fold_parts.hip.h"
#include "interaural_plan.h"

namespace wv {

template <typename Real>
struct EarGatherArgs {
    const Real* field;    // the stored field that holds the step
    float* dst;           // [2][nz][ny][nx] dense: ear a's plane(s), then ear b's
    int64_t pitch;        // elements per stored row
    int64_t nodes;        // B = nx * ny * nz
    int64_t ear_a, ear_b; // element offsets from a taken node to its ears: (ez * mesh_ny + ey) * pitch + ex
    int32_t mesh_ny;      // rows per stored plane
    int32_t x0, y0, z0;
    int32_t nx, ny, nz;   // nodes taken
    int32_t sx, sy, sz;
};

template <typename Real>
__global__ void __launch_bounds__(256) ear_gather_kernel(const EarGatherArgs<Real> a) {
    // x of the grid strides over the nodes of one dense plane (32-bit arithmetic, one division), y over the planes
    const uint32_t per_row = (uint32_t)a.nx;
    const uint32_t n = per_row * (uint32_t)a.ny;
    const int64_t plane_floats = (int64_t)a.nx * a.ny;
    for (int32_t zz = (int32_t)blockIdx.y; zz < a.nz; zz += (int32_t)gridDim.y) {
        const Real* plane = a.field + ((int64_t)(a.z0 + (int64_t)zz * a.sz) * a.mesh_ny + a.y0) * a.pitch + a.x0;
        float* out_plane = a.dst + (int64_t)zz * plane_floats;
        for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
            const uint32_t yy = i / per_row;
            const uint32_t c = i - yy * per_row;
            const Real* src = plane + (int64_t)yy * a.sy * a.pitch + (int64_t)c * a.sx;
            out_plane[i] = (float)src[a.ear_a];
            out_plane[a.nodes + i] = (float)src[a.ear_b];
        }
    }
}

struct InterauralEdges {
    uint32_t e[kInterauralMaxBins];  // wv_interaural_plan::edges, as it lies
};

template <int SMAX>
struct InterauralSample {
    typedef double type;
};
template <>
struct InterauralSample<0> {
    typedef float type;  // no filter: a sample IS its float
};

// stage [T][2][B]: the first t slots hold captures first .. first + t - 1; pre [2][B]; bins [n_bins][2 L + 3][B]; onset [B]; history
// [2][L][B] (not looked at when L == 0); zstate [2][n_sections][2][B] and coef [n_sections][5] (not looked at when n_sections == 0);
// threshold_map [B] or NULL (then `threshold` for every node); nodes = B; t = staged captures to fold, 1 .. kInterauralStage;
// first + t <= 2^32 - 1; max_lag <= LMAX, and >= 1 where LMAX > 0; n_sections <= SMAX.  (Every pointer a __restrict__ kernel argument:
// the stores must be known not to touch what is read later.)
template <int SMAX, int LMAX>
__global__ void __launch_bounds__(256)
    interaural_fold_kernel(const float* __restrict__ stage, double* __restrict__ pre, double* __restrict__ bins, uint32_t* __restrict__ onset,
                           double* __restrict__ history, double* __restrict__ zstate, const double* __restrict__ coef,
                           const float* __restrict__ threshold_map, const float threshold, const InterauralEdges edges, const uint32_t n_bins,
                           const uint32_t max_lag, const uint32_t n_sections, const uint32_t first, const uint64_t nodes, const int32_t t) {
    typedef typename InterauralSample<SMAX>::type X;
    constexpr int T = kInterauralStage;
    constexpr int CH = kInterauralLagChunk;
    constexpr int S = SMAX ? SMAX : 1;  // (no array of no elements)
    static_assert(SMAX >= 0 && SMAX <= (int)kInterauralMaxSections && LMAX >= 0 && LMAX <= (int)kInterauralMaxLag && LMAX % CH == 0, "0 .. 4 sections, lags in chunks");
    const uint64_t node = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (node >= nodes || t < 1) return;
    const uint32_t L = max_lag;
    const uint64_t planes = 2ull * L + 3ull;
    X xa[LMAX + T], xb[LMAX + T];  // the L samples before the fold at LMAX - L .. LMAX - 1, capture j of the fold at LMAX + j
    {
        float pa[T][1], pb[T][1];
        stage_read(stage, 2 * nodes, node, t, pa);          // (slot j's two planes lie 2 B floats behind slot j - 1's)
        stage_read(stage + nodes, 2 * nodes, node, t, pb);
#pragma unroll
        for (int j = 0; j < T; ++j)
            if (j < t) xa[LMAX + j] = (X)pa[j][0], xb[LMAX + j] = (X)pb[j][0];
    }
    if constexpr (LMAX > 0) {
        const uint32_t base = first % L;  // (no lane in it) the slot of capture `first`
#pragma unroll
        for (int m = 1; m <= LMAX; ++m) {
            if ((uint32_t)m <= L) {
                const uint32_t slot = base >= (uint32_t)m ? base - (uint32_t)m : base + L - (uint32_t)m;
                xa[LMAX - m] = (X)history[(uint64_t)slot * nodes + node];
                xb[LMAX - m] = (X)history[((uint64_t)L + slot) * nodes + node];
            }
        }
    }
    const float thr = threshold_map ? threshold_map[node] : threshold;
    const uint32_t onset_was = onset[node];
    uint32_t on = onset_was;
    double pr[2] = {0.0, 0.0};
    if (onset_was == kInterauralNone) pr[0] = pre[node], pr[1] = pre[nodes + node];  // (final behind the onset: not touched again)
    // ---- the onset, the cascade, what lies ahead of the onset
    {
        double b0[S], b1[S], b2[S], a1[S], a2[S], z1a[S], z2a[S], z1b[S], z2b[S];
        if constexpr (SMAX > 0) {
#pragma unroll
            for (int s = 0; s < SMAX; ++s) {
                if ((uint32_t)s < n_sections) {
                    b0[s] = coef[5 * s], b1[s] = coef[5 * s + 1], b2[s] = coef[5 * s + 2], a1[s] = coef[5 * s + 3], a2[s] = coef[5 * s + 4];
                    z1a[s] = zstate[(uint64_t)(2 * s) * nodes + node], z2a[s] = zstate[(uint64_t)(2 * s + 1) * nodes + node];
                    z1b[s] = zstate[(uint64_t)(2 * (n_sections + s)) * nodes + node], z2b[s] = zstate[(uint64_t)(2 * (n_sections + s) + 1) * nodes + node];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < T; ++j) {
            if (j < t) {
                const uint32_t c = first + (uint32_t)j;  // (no lane in it)
                const float mag = __builtin_fmaxf(__builtin_fabsf((float)xa[LMAX + j]), __builtin_fabsf((float)xb[LMAX + j]));  // (still the floats)
                on = onset_update(on, mag, thr, c, kInterauralNone);
                double va = (double)xa[LMAX + j], vb = (double)xb[LMAX + j];
                if constexpr (SMAX > 0) {
#pragma unroll
                    for (int s = 0; s < SMAX; ++s) {
                        if ((uint32_t)s < n_sections) {
                            const double oa = va * b0[s] + z1a[s];
                            z1a[s] = (va * b1[s] - a1[s] * oa) + z2a[s];
                            z2a[s] = va * b2[s] - a2[s] * oa;
                            va = oa;
                            const double ob = vb * b0[s] + z1b[s];
                            z1b[s] = (vb * b1[s] - a1[s] * ob) + z2b[s];
                            z2b[s] = vb * b2[s] - a2[s] * ob;
                            vb = ob;
                        }
                    }
                    xa[LMAX + j] = (X)va, xb[LMAX + j] = (X)vb;
                }
                if (on == kInterauralNone) {
                    pr[0] = pr[0] + va * va;
                    pr[1] = pr[1] + vb * vb;
                }
            }
        }
        if constexpr (SMAX > 0) {
#pragma unroll
            for (int s = 0; s < SMAX; ++s) {
                if ((uint32_t)s < n_sections) {
                    zstate[(uint64_t)(2 * s) * nodes + node] = z1a[s], zstate[(uint64_t)(2 * s + 1) * nodes + node] = z2a[s];
                    zstate[(uint64_t)(2 * (n_sections + s)) * nodes + node] = z1b[s], zstate[(uint64_t)(2 * (n_sections + s) + 1) * nodes + node] = z2b[s];
                }
            }
        }
    }
    if (on != onset_was) onset[node] = on;
    if (onset_was == kInterauralNone) pre[node] = pr[0], pre[nodes + node] = pr[1];
    double* const sums = bins + node;  // plane p of bin w: sums[(w * planes + p) * nodes]
    // ---- the pass of Ea, Eb and C[0].  Capture c lies behind the onset exactly when the node has one by the end of this fold and
    // c >= it: the onset is the FIRST capture that reached the threshold
    if (on != kInterauralNone) {
        uint32_t held = kInterauralNone;  // the bin whose sums e holds; none yet
        double e[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < T; ++j) {
            if (j < t) {
                const uint32_t c = first + (uint32_t)j;
                if (c >= on) {
                    const uint32_t k = interaural_bin(c - on, edges.e, n_bins);
                    if (k != held) {
                        if (held != kInterauralNone) {
                            sums[((uint64_t)held * planes) * nodes] = e[0], sums[((uint64_t)held * planes + 1) * nodes] = e[1];
                            sums[((uint64_t)held * planes + 2 + L) * nodes] = e[2];
                        }
                        held = k;
                        e[0] = sums[((uint64_t)held * planes) * nodes], e[1] = sums[((uint64_t)held * planes + 1) * nodes];
                        e[2] = sums[((uint64_t)held * planes + 2 + L) * nodes];
                    }
                    const double va = (double)xa[LMAX + j], vb = (double)xb[LMAX + j];
                    e[0] = e[0] + va * va;
                    e[1] = e[1] + vb * vb;
                    e[2] = e[2] + va * vb;
                }
            }
        }
        if (held != kInterauralNone) {
            sums[((uint64_t)held * planes) * nodes] = e[0], sums[((uint64_t)held * planes + 1) * nodes] = e[1];
            sums[((uint64_t)held * planes + 2 + L) * nodes] = e[2];
        }
    }
    // ---- the passes of the lags l0 .. l0 + CH - 1 on either side
    if constexpr (LMAX > 0) {
#pragma unroll
        for (int l0 = 1; l0 <= LMAX; l0 += CH) {
            if ((uint32_t)l0 <= L && on != kInterauralNone) {
                uint32_t held = kInterauralNone;
                double cp[CH], cm[CH];  // C[w][L + l], C[w][L - l]
#pragma unroll
                for (int j = 0; j < T; ++j) {
                    if (j < t) {
                        const uint32_t c = first + (uint32_t)j;
                        if (c >= on) {
                            const uint32_t k = interaural_bin(c - on, edges.e, n_bins);
                            if (k != held) {
                                if (held != kInterauralNone) {
#pragma unroll
                                    for (int ll = 0; ll < CH; ++ll) {
                                        if ((uint32_t)(l0 + ll) <= L) {
                                            sums[((uint64_t)held * planes + 2 + L + (uint32_t)(l0 + ll)) * nodes] = cp[ll];
                                            sums[((uint64_t)held * planes + 2 + L - (uint32_t)(l0 + ll)) * nodes] = cm[ll];
                                        }
                                    }
                                }
                                held = k;
#pragma unroll
                                for (int ll = 0; ll < CH; ++ll) {
                                    if ((uint32_t)(l0 + ll) <= L) {
                                        cp[ll] = sums[((uint64_t)held * planes + 2 + L + (uint32_t)(l0 + ll)) * nodes];
                                        cm[ll] = sums[((uint64_t)held * planes + 2 + L - (uint32_t)(l0 + ll)) * nodes];
                                    }
                                }
                            }
                            const double va = (double)xa[LMAX + j], vb = (double)xb[LMAX + j];
#pragma unroll
                            for (int ll = 0; ll < CH; ++ll) {
                                if ((uint32_t)(l0 + ll) <= L) {
                                    cp[ll] = cp[ll] + (double)xa[LMAX + j - (l0 + ll)] * vb;  // a earlier, b later: tau = +l
                                    cm[ll] = cm[ll] + (double)xb[LMAX + j - (l0 + ll)] * va;
                                }
                            }
                        }
                    }
                }
                if (held != kInterauralNone) {
#pragma unroll
                    for (int ll = 0; ll < CH; ++ll) {
                        if ((uint32_t)(l0 + ll) <= L) {
                            sums[((uint64_t)held * planes + 2 + L + (uint32_t)(l0 + ll)) * nodes] = cp[ll];
                            sums[((uint64_t)held * planes + 2 + L - (uint32_t)(l0 + ll)) * nodes] = cm[ll];
                        }
                    }
                }
            }
        }
        // ---- the history: the fold's last min(t, L) samples into their slots (capture first + t - m lies m slots before capture first + t's)
        const uint32_t end = (first + (uint32_t)t) % L;
#pragma unroll
        for (int j = 0; j < T; ++j) {
            if (j < t && (uint32_t)(t - j) <= L) {
                const uint32_t m = (uint32_t)(t - j);
                const uint32_t slot = end >= m ? end - m : end + L - m;
                history[(uint64_t)slot * nodes + node] = (double)xa[LMAX + j];
                history[((uint64_t)L + slot) * nodes + node] = (double)xb[LMAX + j];
            }
        }
    }
}

}  // namespace wv

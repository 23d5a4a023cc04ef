// fold_parts.hip.h -- the pieces more than one fold kernel of the accumulating plans has, each the ONE copy of its arithmetic.  A
// kernel's header keeps the formula block of its own plan (the contract a NumPy loop reproduces bit for bit).  Built with
// -ffp-contract=off: every product and every sum is rounded on its own.  Every piece is forced inline and its loops are unrolled:
// what a lane keeps lives in registers.  Only pieces with which every kernel's assembly is the hand-written body's are here
// (HISTORY.md: the cascade, the held bins and the Fourier sum are not).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// (the tests/cpp/*_kernel_host.cpp programs compile the kernels' text for the host behind a stand-in for the HIP runtime that knows
// neither word)
#ifdef __HIPCC__
#define WV_FOLD_PART __device__ __forceinline__
#else
#define WV_FOLD_PART inline
#endif

namespace wv {

typedef float FoldFloat2 __attribute__((vector_size(8)));
typedef double FoldDouble2 __attribute__((vector_size(16)));

// A lane's N nodes of one dense plane, N = 1, or 2 in one access (the caller sees to the alignment: an even B and an even node).
template <int N, typename Pair, typename T>
WV_FOLD_PART void plane_load(const T* src, T (&v)[N]) {
    if (N == 2) {
        const Pair pair = *reinterpret_cast<const Pair*>(src);
        v[0] = pair[0], v[N - 1] = pair[1];
    } else {
        v[0] = src[0];
    }
}
template <int N, typename Pair, typename T>
WV_FOLD_PART void plane_store(T* dst, const T (&v)[N]) {
    if (N == 2)
        *reinterpret_cast<Pair*>(dst) = Pair{v[0], v[N - 1]};
    else
        dst[0] = v[0];
}

// The first t of the stage's SLOTS captures float[SLOTS][B] -> p, read once and kept in registers as T (float: half the registers, the
// conversion at each use is exact).  The loop is unrolled over all slots behind a wave-uniform `j < t`: a slot's index is a constant.
template <typename T, int N, int SLOTS>
WV_FOLD_PART void stage_read(const float* __restrict__ stage, const uint64_t nodes, const uint64_t node, const int32_t t, T (&p)[SLOTS][N]) {
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) {
        if (j < t) {
            float v[N];
            plane_load<N, FoldFloat2>(stage + (uint64_t)j * nodes + node, v);
#pragma unroll
            for (int n = 0; n < N; ++n) p[j][n] = (T)v[n];
        }
    }
}

// One step of the reference's directional_receiver integrator on one axis: k = ambient_density * sample_rate, an IEEE division, never
// a multiplication by 1 / k.
WV_FOLD_PART double integrate(const double v, const float g, const double k) {
    const double m = (double)g * 0.5;
    return v - m / k;
}

// The onset of a node is the first capture c whose magnitude a reaches the threshold (false for a NaN); `none`: no onset yet.
WV_FOLD_PART uint32_t onset_update(uint32_t on, const float a, const float thr, const uint32_t c, const uint32_t none) {
    if (on == none && a >= thr) on = c;
    return on;
}

}  // namespace wv

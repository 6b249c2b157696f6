// pvx_select.h -- device functions: order statistics of a short float64 series held in LDS, one wave64 per series, and the
// small wave-wide reductions the segmenter kernels share (k_segment.hip).  Design: SEGMENT.md.
//
// Selection is by rank counting: lane l owns the elements l, l + 64, ..; it counts, for each of its elements, the elements
// that sort before it -- smaller, or equal with a lower index -- and so knows that element's place in the sorted series.
// Ranks are a permutation of 0 .. m - 1, so each wanted place has exactly one writer and ties need no second pass.  The
// series is read through LDS broadcasts (every lane reads the same v[j]), four owned elements per read; m^2 / 64 comparisons
// per lane: 1024 at the 256 points of a side of pvx_seg_refine, 262144 at the 4096 of pvx_seg_transitions.  No lane
// writes the series, no barrier is needed between the passes, and the result does not depend on the data's order beyond
// the ties' indices, which an LDS bitonic sort (log^2 m barriers, padding to a power of two, a second copy of the series
// when the original order is still needed for the crossing scan) would not give for free.
// The callers test for NaN first: a series with a NaN has no order here.
#pragma once
#include <math.h>

#include <hip/hip_runtime.h>

namespace pvxsel {

__device__ __forceinline__ void lds_sync() {                         // LDS hand-off inside one wave (as pvx_roots.h)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// the lowest (key, idx) pair of the wave in lexicographic order; key NaN never wins (the callers give +inf for "none")
__device__ __forceinline__ void wave_argmin(double& key, int& idx) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double ok = __shfl_xor(key, d, 64);
        const int oi = __shfl_xor(idx, d, 64);
        if (ok < key || (ok == key && oi < idx)) { key = ok; idx = oi; }
    }
}

// np.min / np.max of v[0 .. m) for a series without NaN: (+inf, -inf) for m = 0
__device__ __forceinline__ void wave_minmax(const double* v, int m, int lane, double* mn, double* mx) {
    double lo = INFINITY, hi = -INFINITY;
    for (int j = lane; j < m; j += 64) { const double x = v[j]; lo = x < lo ? x : lo; hi = x > hi ? x : hi; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double ol = __shfl_xor(lo, d, 64), oh = __shfl_xor(hi, d, 64);
        lo = ol < lo ? ol : lo; hi = oh > hi ? oh : hi;
    }
    *mn = lo; *mx = hi;
}

__device__ __forceinline__ bool wave_any_nan(const double* v, int m, int lane) {
    bool nan = false;
    for (int j = lane; j < m; j += 64) { const double x = v[j]; nan |= x != x; }
    return __ballot(nan) != 0ull;
}

// out[q] = the element of v[0 .. m) at place want[q] of the sorted series, q < NW; a place outside 0 .. m - 1 leaves out[q]
// as it is.  v and out are LDS of the calling wave; the caller synchronises (lds_sync) before it reads out.
template <int NW> __device__ __forceinline__ void select_ranks(const double* v, int m, const int (&want)[NW], double* out, int lane) {
    for (int i0 = lane; i0 < m; i0 += 256) {                         // (the lanes' trip counts differ: nothing below is wave-wide)
        double own[4];
        int at[4], rank[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            at[q] = i0 + 64 * q;
            own[q] = at[q] < m ? v[at[q]] : 0.0;
            rank[q] = 0;
        }
        for (int j = 0; j < m; j++) {
            const double x = v[j];
#pragma unroll
            for (int q = 0; q < 4; q++) rank[q] += (x < own[q] || (x == own[q] && j < at[q])) ? 1 : 0;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (at[q] >= m) continue;
#pragma unroll
            for (int w = 0; w < NW; w++)
                if (rank[q] == want[w]) out[w] = own[q];
        }
    }
}

// np.median of a series without NaN from its two middle places lo = out[(m-1)/2], hi = out[m/2]: np.mean of the two (of the
// one, counted twice, for an odd m -- (x + x) / 2 is x, infinities included); m = 0: NaN
__device__ __forceinline__ double median_of(double lo, double hi, int m) { return m == 0 ? NAN : (m & 1 ? lo : (lo + hi) / 2.0); }

}  // namespace pvxsel

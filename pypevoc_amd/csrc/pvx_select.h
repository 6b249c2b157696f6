// pvx_select.h -- device functions: order statistics of a short float64 series held in LDS, one wave64 per series, and the
// small wave-wide reductions, np.sum's summation order and np.percentile's linear rule that the segmenter and the jump
// kernels share (k_segment.hip, k_jumps.hip).  Design: SEGMENT.md.
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


// ---- np.sum's order -----------------------------------------------------------------------------------------------------
// numpy adds a contiguous float64 run of n < 8 values one by one from 0.0; 8 <= n <= 128 into eight accumulators by index % 8
// up to n - n % 8, ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the rest one by one; a longer run as the sum of its
// two halves, the first of n / 2 rounded down to a multiple of 8.  np.sum and np.mean start from 0.0 + that.
template <class F> __device__ __forceinline__ double np_block_sum(F a, int lo, int n) {   // n <= 128
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; i++) res += a(lo + i);
        return res;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = a(lo + j);
    const int n8 = n - n % 8;
    for (int i = 8; i < n8; i += 8) {
#pragma unroll
        for (int j = 0; j < 8; j++) r[j] += a(lo + i + j);
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (int i = n8; i < n; i++) res += a(lo + i);
    return res;
}

// the recursion over halves as a post-order walk with an explicit stack: a run longer than 128 becomes (join, right half, left
// half); the blocks' sums come in index order and a join adds the two sums below it, left + right
constexpr int kNpSumMaxRun = 4096;                                   // the longest run np_sum's stacks hold; its callers assert their limits
template <class F> __device__ __forceinline__ double np_sum(F a, int n) {
    struct Item { int lo, n, join; };
    Item todo[24];                                                   // kNpSumMaxRun: five levels, two items a level
    double sums[8];
    int nt = 0, ns = 0;
    todo[nt++] = {0, n, 0};
    while (nt > 0) {
        const Item s = todo[--nt];
        if (s.join) {
            const double right = sums[--ns], left = sums[--ns];
            sums[ns++] = left + right;
        } else if (s.n <= 128) {
            sums[ns++] = np_block_sum(a, s.lo, s.n);
        } else {
            int n2 = s.n / 2;
            n2 -= n2 % 8;
            todo[nt++] = {0, 0, 1};
            todo[nt++] = {s.lo + n2, s.n - n2, 0};
            todo[nt++] = {s.lo, n2, 0};
        }
    }
    return 0.0 + sums[0];
}

// np.percentile(side, q100), method 'linear', from the sorted side's places: which two places it reads (plan), and its value
struct PctPlan { int prev, next; double t; };
__device__ __forceinline__ PctPlan pct_plan(int m, double q100) {
    const double q = q100 / 100.0;
    const double virt = (double)m * q + (1.0 + q * (1.0 - 1.0 - 1.0)) - 1.0;
    double prev = floor(virt), next = prev + 1.0, gprev = prev;
    if (virt >= (double)(m - 1)) { prev = next = (double)(m - 1); gprev = -1.0; }   // numpy writes -1 (the last) and keeps it for gamma
    if (virt < 0.0) { prev = next = 0.0; gprev = 0.0; }
    PctPlan pl;
    pl.prev = (int)prev; pl.next = (int)next; pl.t = virt - gprev;
    return pl;
}
__device__ __forceinline__ double pct_value(double a, double b, double t) {
    const double diff = b - a;
    return t >= 0.5 ? b - diff * (1.0 - t) : a + diff * t;
}

}  // namespace pvxsel

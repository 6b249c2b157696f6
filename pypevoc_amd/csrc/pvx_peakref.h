// pvx_peakref.h -- device functions: PeakFinder's scan with the default thresholds (pypevoc/PeakFinder.py:155-194) and its
// three-point refinement (refine :331-372, fun=None, rad=1) on one row per wave64, float64.  Design: ENVELOPE.md.
//
// A row is a callable y(k) whose value depends on k alone (a table in memory, or a function evaluated on the spot: the same
// bits whichever lane asks), an axis a callable x(k).  Lane l owns the points l B .. l B + B - 1, B = ceil(npts / 64), so
// ascending index order is lane order.
//   scan_block   the lane walks its block once with a three-point window, stores its own points (optional) and sets one
//                bit per peak -- index i in 1 .. npts - 2 with y[i-1] < y[i] and y[i] >= y[i+1]; comparisons with NaN are
//                false -- in its words of the wave's mask; returns the lane's count
//   wave_excl    exclusive prefix of the lanes' counts and their total
//   emit_block   the lane's peaks, refined, at list positions prefix, prefix + 1, .. (left-packed, ascending); positions
//                from maxpk on are not written
//   refine3      c = s1, b = (s2 - s0) / 2, a = (s2 + s0) / 2 - c, lpos = -b / 2 / a, fpos = i + lpos,
//                fval = a lpos lpos + b lpos + c when `fit`, else (refine's else branch) fpos = i, fval = s1;
//                pos = np.interp(fpos, arange(npts), x).  No fused multiply-add: numpy's operations in numpy's order.
#pragma once
#include <math.h>

#include <hip/hip_runtime.h>

namespace pvxpk {

constexpr int kRowOk = 0, kRowOverflow = 1, kRowBadIndex = 2, kRowLeadZero = 3;   // a row's status
constexpr int kMaxBlock = 256;                                       // points per lane at PVX_ENV_MAX_NPTS
constexpr int kMaskWords = kMaxBlock / 32;                           // mask words per lane: word w of lane l at m[w * 64 + l]

struct AxisArange {
    __device__ double operator()(int k) const { return (double)k; }
};
struct AxisTable {
    const double* x;
    __device__ double operator()(int k) const { return x[k]; }
};
struct AxisFreq {                                                    // x_k = k fs / (2 npts)
    double fs, two_n;
    __device__ double operator()(int k) const { return (double)k * fs / two_n; }
};

// np.interp(fpos, arange(n), x): x[0] at or below 0, x[n-1] at or above n - 1, NaN for NaN, x[j] at an integer j, else
// slope (fpos - j) + x[j] with slope = x[j+1] - x[j], j = floor(fpos).  Reads x inside 0 .. n - 1 whatever fpos is.
template <class X> __device__ __forceinline__ double interp_axis(double fpos, int n, X x) {
    if (fpos != fpos) return fpos;
    if (fpos <= 0.0) return x(0);
    if (fpos >= (double)(n - 1)) return x(n - 1);
    const int j = (int)fpos;                                         // 0 < fpos < n - 1: j in 0 .. n - 2
    const double xj = x(j), t = fpos - (double)j;
    if (t == 0.0) return xj;
    const double slope = x(j + 1) - xj;
    return slope * t + xj;
}

template <class X>
__device__ __forceinline__ void refine3(double s0, double s1, double s2, int i, int n, X x, bool fit, double* pos, double* val) {
    double fpos = (double)i, fval = s1;
    if (fit) {
        const double c = s1;
        const double b = (s2 - s0) / 2.0;
        const double a = (s2 + s0) / 2.0 - c;
        const double lpos = -(b / 2.0 / a);
        fpos = (double)i + lpos;
        fval = a * lpos * lpos + b * lpos + c;
    }
    *pos = interp_axis(fpos, n, x);
    *val = fval;
}

template <class Y>
__device__ __forceinline__ int scan_block(Y y, int k0, int k1, int npts, double* own, unsigned* m, int lane) {
    int cnt = 0;
    if (k0 >= k1) return 0;
    double prev = k0 > 0 ? y(k0 - 1) : 0.0, cur = y(k0);
    unsigned bits = 0;
    for (int k = k0; k < k1; k++) {
        const double next = k + 1 < npts ? y(k + 1) : cur;
        if (own) own[k] = cur;
        const bool pk = k >= 1 && k <= npts - 2 && prev < cur && cur >= next;
        const int b = (k - k0) & 31;
        bits |= pk ? 1u << b : 0u;
        cnt += pk ? 1 : 0;
        if (b == 31 || k + 1 == k1) { m[((k - k0) >> 5) * 64 + lane] = bits; bits = 0; }
        prev = cur; cur = next;
    }
    return cnt;
}

__device__ __forceinline__ int wave_excl(int cnt, int lane, int* total) {
    int incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    *total = __shfl(incl, 63, 64);
    return incl - cnt;
}

template <class Y, class X>
__device__ __forceinline__ void emit_block(Y y, X x, int k0, int k1, int npts, const unsigned* m, int lane, int p, int maxpk, int* idx,
                                           double* pos, double* val) {
    for (int w = 0; k0 + 32 * w < k1; w++) {
        unsigned bits = m[w * 64 + lane];
        while (bits != 0u && p < maxpk) {
            const int i = k0 + 32 * w + __ffs((int)bits) - 1;
            bits &= bits - 1u;
            double fp, fv;
            refine3(y(i - 1), y(i), y(i + 1), i, npts, x, true, &fp, &fv);
            if (idx) idx[p] = i;
            if (pos) pos[p] = fp;
            if (val) val[p] = fv;
            p++;
        }
    }
}

// slots from `from` on: idx -1, pos / val NaN
__device__ __forceinline__ void pad_row(int from, int maxpk, int lane, int* idx, double* pos, double* val) {
    for (int t = from + lane; t < maxpk; t += 64) {
        if (idx) idx[t] = -1;
        if (pos) pos[t] = NAN;
        if (val) val[t] = NAN;
    }
}

// scan, count, pack, refine and pad one row; returns the row's status.  idx / pos / val point at the row's maxpk slots.
template <class Y, class X>
__device__ __forceinline__ int row_peaks(Y y, X x, int npts, double* own, unsigned* m, int lane, int maxpk, int* npk, int* idx, double* pos,
                                         double* val) {
    const int B = (npts + 63) >> 6;
    const int k0 = lane * B < npts ? lane * B : npts, k1 = k0 + B < npts ? k0 + B : npts;
    const int cnt = scan_block(y, k0, k1, npts, own, m, lane);
    int total;
    const int p = wave_excl(cnt, lane, &total);
    const bool lists = idx || pos || val;
    if (lists) {
        emit_block(y, x, k0, k1, npts, m, lane, p, maxpk, idx, pos, val);
        pad_row(total < maxpk ? total : maxpk, maxpk, lane, idx, pos, val);
    }
    if (lane == 0 && npk) *npk = total;
    return lists && total > maxpk ? kRowOverflow : kRowOk;
}

}  // namespace pvxpk

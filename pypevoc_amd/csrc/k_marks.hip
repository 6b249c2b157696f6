// k_marks.hip -- period marks: the reference's period_marks_corr (pypevoc/Periodicity.py:573-618) and period_marks_peak
// (:621-709), as MARKS.md states them.  Both are walks: a step decides where the next one starts.  A walk is sequential,
// the work inside a step and the walks of a call are not.
//
// k_marks_corr: one 256-thread workgroup per row (persistent: a workgroup walks rows r, r + grid, ...).  Per step
//   1. thread 0 evaluates the loop test, the two int() truncations and the status cases (MARKS.md, "Row status");
//   2. the stretch x[s : s + P + W] goes to LDS (float64): src = xs[0 : W], tgt = xs[P : P + W];
//   3. lanes own lags: ring j holds the lags |k| in [128 j, 128 j + 127], nearest to 0 first; a thread sums
//      xc[k] = sum_n src[n + k] * tgt[n] over ascending n into LDS.  After a ring every lag with |k| <= 128 j + 126 has both
//      neighbours: the local maxima among the new ones are searched (block minimum of 2 |k| + (k > 0): the nearest one, the
//      lower index on equal distance) and the rings stop at the first that has one, or at |k| = W - 1;
//   4. thread 0 runs the parabola, delay_t, the mark and next_t in the statements' own operation order, then np.interp.
// k_marks_peak: one wave per row (four rows per workgroup, no LDS): first arg-max / arg-min over at most P samples as a strided
//   scan and a butterfly in the order (value, index); the least-squares parabola by the closed-form normal equations.
// float64 throughout.  A lag's sum has one order (ascending n, one fma per term), so a row's result does not depend on the ring
// count, the workgroup, the grid, the other rows or the launch.  Every loop is bounded by max_steps, W or the row length.
// No atomics, no global scratch.
#include <float.h>
#include <math.h>
#include <string.h>

#include <map>
#include <mutex>
#include <vector>

#include "pvx_block.h"
#include "pvx_internal.h"
#include "pvx_mem.h"

namespace {

using namespace pvxb;

constexpr int kThreads = kBlock;
constexpr int kHalf = kThreads / 2;                                  // lags of one sign per ring
constexpr int kGridMax = 1024;
constexpr int kHeadRed = (sizeof(Red) + 7) / 8;
constexpr double kTwo31 = 2147483648.0;

enum { kEnd = 0, kCorr = 1, kSkip = 2 };

// the walk's state: written by thread 0, read by all after a barrier
struct Walk {
    double next_t, f0, delay_t;
    long long P, s;
    int act, have, stop, status, cnt, pad;
};
constexpr int kHead = (kHeadRed + (int)((sizeof(Walk) + 7) / 8) + 1) / 2 * 2;

// np.interp(xv, xp, fp) for one value (numpy/core/src/multiarray/compiled_base.c: arr_interp), xp strictly increasing
__device__ double interp_np(double xv, const double* __restrict__ xp, const double* __restrict__ fp, int n) {
    if (n == 1) return fp[0];
    if (xv != xv) return xv;
    if (xv < xp[0]) return fp[0];
    if (xv > xp[n - 1]) return fp[n - 1];
    int lo = 0, hi = n;                                              // xp[lo] <= xv < xp[hi] (hi == n: no such knot)
    for (int it = 0; it < 32 && hi - lo > 1; it++) {
        const int mid = (lo + hi) >> 1;
        if (xv >= xp[mid]) lo = mid; else hi = mid;
    }
    const int j = lo;
    if (j == n - 1 || xp[j] == xv) return fp[j];
    const double slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]);
    double r = slope * (xv - xp[j]) + fp[j];
    if (r != r) {                                                    // NaN from one side: try the other
        r = slope * (xv - xp[j + 1]) + fp[j + 1];
        if (r != r && fp[j] == fp[j + 1]) r = fp[j];
    }
    return r;
}

// P = int(sr / f0), or -1 where the reference cannot go on: f0 <= 0, NaN, P < 1 or P beyond int32
__device__ long long period_of(double sr, double f0) {
    if (!(f0 > 0.0)) return -1;
    const double q = sr / f0;
    if (!(q >= 1.0 && q < kTwo31)) return -1;
    return (long long)q;
}

__global__ __launch_bounds__(kThreads) void k_marks_corr(MarksCorrParams p) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    Red& red = *(Red*)lds;
    Walk& wk = *(Walk*)(lds + kHeadRed);
    double* xs = lds + kHead;                                        // [cap]: the stretch
    double* xc = xs + p.cap;                                         // [2 W - 1]: xc[k + W - 1]
    const int t = threadIdx.x, W = p.W;
    const bool neg = t < kHalf;
    const int tm = neg ? kHalf - 1 - t : t - kHalf;                  // 0 .. 127: |k| inside a ring
    const int nring = (W + kHalf - 1) / kHalf;
    for (int64_t r = blockIdx.x; r < p.nrows; r += gridDim.x) {
        const int64_t a = p.row_start[r];
        const int64_t L = p.row_stop[r] - a;                         // the entry point checked 0 <= a <= stop <= nsamp
        const double* x = p.x + a;
        const double toff = p.toff ? p.toff[r] : 0.0;
        double* out = p.marks + r * (int64_t)p.max_marks;
        if (t == 0) {
            const double t0 = p.t0[r];
            wk.status = 0; wk.cnt = 1; wk.have = 0; wk.stop = 0; wk.delay_t = 0.0; wk.s = 0;
            out[0] = t0;
            wk.next_t = t0;
            double f0 = interp_np(toff + t0, p.tf, p.f, p.ntf);
            if (f0 != f0) f0 = p.f_fallback;
            wk.f0 = f0;
            wk.P = period_of(p.sr, f0);
            if (!(t0 >= 0.0) || wk.P < 0) { wk.status = PVX_MARKS_BAD_F0; wk.stop = 1; }
        }
        for (int64_t it = 0; it <= p.max_steps; it++) {
            if (t == 0) {
                int act = kEnd;
                if (wk.stop || !(wk.next_t * p.sr < (double)(L - wk.P - W))) {
                    act = kEnd;
                } else if (it == p.max_steps) {
                    wk.status |= PVX_MARKS_STEPS;
                } else if (wk.f0 != wk.f0) {
                    if (!wk.have || !(wk.delay_t > 0.0)) {
                        wk.status |= PVX_MARKS_NO_ADVANCE;
                    } else {
                        wk.next_t = wk.next_t + wk.delay_t;
                        wk.f0 = interp_np(toff + wk.next_t, p.tf, p.f, p.ntf);
                        act = kSkip;
                    }
                } else {
                    const long long P = period_of(p.sr, wk.f0);
                    const double sd = wk.next_t * p.sr;              // < L - P - W: inside int64
                    const long long s = (long long)sd;
                    if (P < 0 || !(sd >= 0.0) || P + W > p.cap) {
                        wk.status |= PVX_MARKS_BAD_F0;
                    } else if (s + P + W > L) {
                        wk.status |= PVX_MARKS_PAST_END;
                    } else {
                        wk.P = P; wk.s = s;
                        act = kCorr;
                    }
                }
                wk.act = act;
            }
            __syncthreads();
            const int act = wk.act;
            const int P = (int)wk.P;
            const int64_t s = wk.s;
            __syncthreads();                                         // everyone has read the step before thread 0 moves on
            if (act == kEnd) break;
            if (act == kSkip) continue;
            for (int i = t; i < P + W; i += kThreads) xs[i] = x[s + i];
            __syncthreads();
            const double* tgt = xs + P;
            int best = INT_MAX;
            for (int j = 0; j < nring; j++) {
                const int m = kHalf * j + tm;                        // this thread's |k|
                if (m <= W - 1) {
                    const int k = neg ? -m : m;
                    const int n0 = k < 0 ? -k : 0, n1 = k < 0 ? W : W - k;
                    const double* src = xs + k;
                    double acc = 0.0;
#pragma unroll 4
                    for (int n = n0; n < n1; n++) acc = fma(src[n], tgt[n], acc);
                    xc[k + W - 1] = acc;
                }
                __syncthreads();
                int key = INT_MAX;
                if (m >= 1 && m <= W - 1) {                          // the lag one nearer to 0 now has both neighbours
                    const int cm = m - 1;
                    const int i = (neg ? -cm : cm) + W - 1;
                    if (xc[i - 1] < xc[i] && xc[i] >= xc[i + 1]) key = 2 * cm + (neg || cm == 0 ? 0 : 1);
                }
                best = block_imin(key, red);
                if (best != INT_MAX) break;                          // block-uniform
            }
            if (t == 0) {
                if (best == INT_MAX) {
                    wk.status |= PVX_MARKS_NO_PEAK;
                    wk.stop = 1;
                } else {
                    const int cm = best >> 1;
                    const int pos = ((best & 1) ? cm : -cm) + W - 1;
                    const double s0 = xc[pos - 1], s1 = xc[pos], s2 = xc[pos + 1];
                    const double c = s1;                             // PeakFinder.py:353-359
                    const double b = (s2 - s0) / 2.0;
                    const double aa = (s2 + s0) / 2.0 - c;
                    const double lpos = -b / 2.0 / aa;
                    double fpos = (double)pos + lpos;
                    if (fpos < 0.0) fpos = 0.0;                      // :372, np.interp over arange(2 W - 1) clamps
                    if (fpos > (double)(2 * W - 2)) fpos = (double)(2 * W - 2);
                    const double delay_samp = fpos - (double)(W - 1);
                    const double delay_t = (-delay_samp + (double)P) / p.sr;
                    wk.delay_t = delay_t; wk.have = 1;
                    if (delay_t > p.min_per) {
                        if (wk.cnt == p.max_marks) {
                            wk.status |= PVX_MARKS_CAPACITY;
                            wk.stop = 1;
                        } else {
                            out[wk.cnt++] = wk.next_t + ((double)W + (double)P / 2.0) / p.sr;
                            wk.next_t = wk.next_t + delay_t;
                        }
                    } else {
                        wk.next_t = wk.next_t + 1.0 / wk.f0;
                    }
                    if (!wk.stop) wk.f0 = interp_np(toff + wk.next_t, p.tf, p.f, p.ntf);
                }
            }
            // thread 0 read xc; the next step's first barrier comes before anything overwrites it
        }
        if (t == 0) { p.count[r] = wk.cnt; p.status[r] = wk.status; }
        __syncthreads();
    }
}

// ---- the peak walk ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool np_gt(double v, double b) { return v > b || (v != v && b == b); }   // np.argmax: a NaN wins
__device__ __forceinline__ bool np_lt(double v, double b) { return v < b || (v != v && b == b); }   // np.argmin: a NaN wins
__device__ __forceinline__ bool np_same(double v, double b) { return v == b || (v != v && b != b); }

// the first arg-max (kMax) or arg-min of x[lo : hi], lo < hi, over the wave; every lane gets the index and the value
template <bool kMax> __device__ int64_t wave_first_arg(const double* __restrict__ x, int64_t lo, int64_t hi, int lane, double* val) {
    double bv = 0.0;
    long long bi = -1;
    for (int64_t i = lo + lane; i < hi; i += 64) {
        const double v = x[i];
        if (bi < 0 || (kMax ? np_gt(v, bv) : np_lt(v, bv))) { bv = v; bi = i; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o);
        const long long oi = __shfl_xor(bi, o);
        if (oi >= 0 && (bi < 0 || (kMax ? np_gt(ov, bv) : np_lt(ov, bv)) || (np_same(ov, bv) && oi < bi))) { bv = ov; bi = oi; }
    }
    *val = bv;
    return bi;
}

__device__ __forceinline__ double peak_f_at(const MarksPeakParams& p, int64_t a, double toff, int64_t i) {
    if (p.fmode == 0) return p.f[0];
    if (p.fmode == 1) return p.f[a + i];
    return interp_np(toff + (double)i / p.sr, p.tf, p.f, p.ntf);
}

__global__ __launch_bounds__(kThreads) void k_marks_peak(MarksPeakParams p) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t stride = (int64_t)gridDim.x * (kThreads / 64);
    for (int64_t r = (int64_t)blockIdx.x * (kThreads / 64) + wv; r < p.nrows; r += stride) {
        const int64_t a = p.row_start[r];
        const int64_t L = p.row_stop[r] - a;
        const double* x = p.x + a;
        const double toff = p.toff ? p.toff[r] : 0.0;
        double* om = p.marks + r * (int64_t)p.max_marks;
        double* ov = p.vals + r * (int64_t)p.max_marks;
        int status = 0, cnt = 0, prev_short = 0;
        // the first finite sample of f
        int64_t idx0 = -1;
        for (int64_t base = 0; base < L; base += 64) {
            const int64_t i = base + lane;
            const bool fin = i < L && isfinite(peak_f_at(p, a, toff, i));
            const unsigned long long mask = __ballot(fin);
            if (mask) { idx0 = base + (__ffsll((long long)mask) - 1); break; }
        }
        long long P = idx0 < 0 ? -1 : period_of(p.sr, peak_f_at(p, a, toff, idx0));
        if (P < 0) {
            status = PVX_MARKS_BAD_F0;
        } else {
            double v;
            int64_t idx_start = wave_first_arg<false>(x, idx0, min((int64_t)(idx0 + P), L), lane, &v);
            for (int64_t it = 0; idx_start < L; it++) {
                if (it == p.max_steps) { status |= PVX_MARKS_STEPS; break; }
                double xm;
                const int64_t idx_max = wave_first_arg<true>(x, idx_start, min((int64_t)(idx_start + P), L), lane, &xm);
                const int m = (int)min((int64_t)p.fit_points, L - idx_max - 1);
                double t_max = (double)idx_max / p.sr, v_max = xm;
                const int shortfit = m < 2;
                if (!shortfit) {
                    // least squares of p0 u^2 + p1 u + p2 over (u, x[idx_max + i] - x[idx_max]), u = i - m / 2, i = 0 .. m: about the
                    // middle the odd sums vanish and the normal equations fall apart into p1 = T1 / S2 and a 2 x 2 system
                    const double c = 0.5 * (double)m;
                    double S2 = 0, S4 = 0, T0 = 0, T1 = 0, T2 = 0;
                    for (int i = 0; i <= m; i++) {
                        const double u = (double)i - c, u2 = u * u, y = x[idx_max + i] - xm;
                        S2 += u2; S4 += u2 * u2;
                        T0 += y; T1 += u * y; T2 += u2 * y;
                    }
                    const double S0 = (double)(m + 1);
                    const double D = S4 * S0 - S2 * S2;
                    const double p0 = (T2 * S0 - S2 * T0) / D, p1 = T1 / S2, p2 = (S4 * T0 - S2 * T2) / D;
                    const double uu = -p1 / p0 / 2.0;                // the vertex, from the middle
                    const double rel = c + uu;
                    if (fabs(rel) <= (double)p.fit_points) {
                        t_max = ((double)idx_max + rel) / p.sr;
                        v_max = ((p0 * uu + p1) * uu + p2) + xm;
                    }
                }
                const double f0 = peak_f_at(p, a, toff, idx_max);
                if (isfinite(f0)) {
                    P = period_of(p.sr, f0);
                    if (P < 0) { status |= PVX_MARKS_BAD_F0; break; }
                    if (cnt == p.max_marks) { status |= PVX_MARKS_CAPACITY; break; }
                    if (prev_short) status |= PVX_MARKS_SHORT_FIT;
                    prev_short = shortfit;
                    if (lane == 0) { om[cnt] = t_max; ov[cnt] = v_max; }
                    cnt++;
                }
                const int64_t am = wave_first_arg<false>(x, idx_max, min((int64_t)(idx_max + P), L), lane, &v);
                idx_start = am > idx_max ? am : idx_max + 1;
            }
        }
        if (lane == 0) { p.count[r] = cnt > 0 ? cnt - 1 : 0; p.status[r] = status; }   // the last mark is dropped (:708)
    }
}

// the row lists and the track of a call, kept per device for the process (grow-only; calls on one device take turns)
struct MarksWs {
    std::mutex mu;
    DevMem buf;
};
std::mutex g_ws_mu;
std::map<int, MarksWs*> g_ws;                                        // device -> workspace (never erased)

int workspace(MarksWs** w) {
    int dev = 0;
    PVX_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_ws_mu);
    MarksWs*& e = g_ws[dev];
    if (!e) e = new MarksWs();
    *w = e;
    return PVX_OK;
}

// one block of 8-byte words: [row_start][row_stop][t0][toff][tf][f]; absent lists take no room
struct Pack {
    std::vector<int64_t> words;
    size_t add(const void* src, size_t n) {
        const size_t at = words.size();
        if (src && n) { words.resize(at + n); memcpy(words.data() + at, src, n * 8); }
        return at;
    }
};

}  // namespace

int pvx_marks_corr_run(MarksCorrParams p, const MarksRows& h, hipStream_t s, const char** kernels) {
    *kernels = "";
    if (p.nrows <= 0) return PVX_OK;
    MarksWs* w;
    int rc;
    if ((rc = workspace(&w)) != PVX_OK) return rc;
    std::lock_guard<std::mutex> lk(w->mu);
    Pack pk;
    const size_t o_st = pk.add(h.row_start, p.nrows), o_sp = pk.add(h.row_stop, p.nrows), o_t0 = pk.add(h.t0, p.nrows);
    const size_t o_to = pk.add(h.toff, p.nrows), o_tf = pk.add(h.tf, h.ntf), o_f = pk.add(h.f, h.nf);
    if ((rc = w->buf.grow(pk.words.size() * 8, Sizing::headroom)) != PVX_OK) return rc;
    PVX_HIP_CHECK(hipMemcpyAsync(w->buf.get(), pk.words.data(), pk.words.size() * 8, hipMemcpyHostToDevice, s));
    const int64_t* base = w->buf.as<const int64_t>();
    p.row_start = base + o_st; p.row_stop = base + o_sp;
    p.t0 = (const double*)(base + o_t0);
    p.toff = h.toff ? (const double*)(base + o_to) : nullptr;
    p.tf = (const double*)(base + o_tf); p.f = (const double*)(base + o_f);
    p.ntf = (int)h.ntf;
    const size_t lds = ((size_t)kHead + (size_t)p.cap + (size_t)(2 * p.W)) * 8;   // <= 64 KiB by PVX_MARKS_CORR_MAX_LDS
    const unsigned grid = (unsigned)(p.nrows < kGridMax ? p.nrows : kGridMax);
    hipLaunchKernelGGL(k_marks_corr, dim3(grid), dim3(kThreads), lds, s, p);
    PVX_HIP_CHECK(hipGetLastError());
    PVX_HIP_CHECK(hipStreamSynchronize(s));                          // the workspace is free for the next call from here on
    *kernels = "k_marks_corr";
    return PVX_OK;
}

int pvx_marks_peak_run(MarksPeakParams p, const MarksRows& h, hipStream_t s, const char** kernels) {
    *kernels = "";
    if (p.nrows <= 0) return PVX_OK;
    MarksWs* w;
    int rc;
    if ((rc = workspace(&w)) != PVX_OK) return rc;
    std::lock_guard<std::mutex> lk(w->mu);
    Pack pk;
    const size_t o_st = pk.add(h.row_start, p.nrows), o_sp = pk.add(h.row_stop, p.nrows);
    const size_t o_to = pk.add(h.toff, p.nrows), o_tf = pk.add(h.tf, h.ntf), o_f = pk.add(h.f, h.nf);
    if ((rc = w->buf.grow(pk.words.size() * 8, Sizing::headroom)) != PVX_OK) return rc;
    PVX_HIP_CHECK(hipMemcpyAsync(w->buf.get(), pk.words.data(), pk.words.size() * 8, hipMemcpyHostToDevice, s));
    const int64_t* base = w->buf.as<const int64_t>();
    p.row_start = base + o_st; p.row_stop = base + o_sp;
    p.toff = h.toff ? (const double*)(base + o_to) : nullptr;
    p.tf = h.tf ? (const double*)(base + o_tf) : nullptr; p.f = (const double*)(base + o_f);
    p.ntf = (int)h.ntf;
    p.fmode = h.tf ? 2 : (h.nf == 1 ? 0 : 1);
    const int64_t nblk = (p.nrows + kThreads / 64 - 1) / (kThreads / 64);
    const unsigned grid = (unsigned)(nblk < kGridMax ? nblk : kGridMax);
    hipLaunchKernelGGL(k_marks_peak, dim3(grid), dim3(kThreads), 0, s, p);
    PVX_HIP_CHECK(hipGetLastError());
    PVX_HIP_CHECK(hipStreamSynchronize(s));
    *kernels = "k_marks_peak";
    return PVX_OK;
}

// k_jumps.hip -- the device half of pypevoc/speech/PitchJumps.py: frame selection by magnitude (detect_jumps :179-183), the
// windowed statistics zscore_wind :50-64, linreg_err :67-84 and linreg2_err :87-121, the strict-extremum pick (:190-200) and
// the per-jump line fits (calc_jump_params :209-242), on rows of tracks padded to nmax with a length per row.  float64
// throughout, no fused multiply-add (the library is built with -ffp-contract=off), no atomics.  Design: JUMPS.md.
//
// k_jump_select: one workgroup per row.  Pass 1: a thread per frame takes m = sqrt(sum_k mag[k]^2) in np.sum's order of a
//   contiguous run (pvx_select.h) and the workgroup the row's maximum (a NaN magnitude makes it NaN: nothing is selected, as
//   with np.max).  Pass 2 walks the row in ordered tiles of the workgroup's width: m > max * mag_threshold (strict), a ballot
//   per wave and the waves' counts as a prefix in LDS, so the selected (t, f0) pairs are left-packed in ascending order and
//   the count of the tiles before is a register.
// k_winstat: one wave64 per (row, index), lanes over the window's points; a workgroup of four waves takes four consecutive
//   indices and loads their shared stretch of t and x into LDS once (when four indices' stretch does not fit -- a large hop --
//   a workgroup takes one index).  Every sum is a lane's partial sum over the points lane, lane + 64, .. in ascending order
//   followed by the __shfl_xor butterfly 32, 16, .., 1: a fixed order, so a result does not depend on the grid, the row's
//   place in the batch or the other rows.  Means and sums of squares are two-pass.  The medians and percentiles of kind
//   ZMEDIAN are order statistics by rank counting (pvx_select.h) with np.percentile's linear rule.
// k_jump_pick: one workgroup per row.  The strict interior extrema of zs beyond +-t_threshold in ordered tiles, up- and
//   down-jumps merged in one ascending list (dir says which); then a wave per jump fits the lines of up to nsl points before
//   and after it (read from global memory, lanes over the points) and evaluates both at the jump.  Without zs the lists are
//   the caller's and only the fits run (calc_jump_params on indices set by hand).
// Reads are clamped to the rows whatever len holds.
#include <math.h>
#include <stdint.h>

#include "pvx_internal.h"
#include "pvx_select.h"

namespace {

using namespace pvxsel;

constexpr int kRowThreads = 256, kRowWaves = kRowThreads / 64;
static_assert(PVX_JUMP_MAX_K <= kNpSumMaxRun, "np_sum's stacks (pvx_select.h) are sized for runs of up to kNpSumMaxRun terms");

__device__ __forceinline__ int row_len(const int* len, int64_t r, int nmax) {
    const int n = len ? len[r] : nmax;
    return n < 0 ? 0 : (n > nmax ? nmax : n);
}

// sum over j < n of f(j): lane l adds its points l, l + 64, .. in ascending order from 0.0, then the butterfly
template <class F> __device__ __forceinline__ double wsum(int n, int lane, F f) {
    double s = 0.0;
    for (int j = lane; j < n; j += 64) s += f(j);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    return s;
}

// the least-squares line through n points, centred: b = sum((t - tm)(x - xm)) / sum((t - tm)^2), a = xm - b tm
struct Line { double a, b; };
__device__ __forceinline__ Line fit_line(const double* t, const double* x, int n, int lane) {
    const double tm = wsum(n, lane, [t](int j) { return t[j]; }) / (double)n;
    const double xm = wsum(n, lane, [x](int j) { return x[j]; }) / (double)n;
    const double sxy = wsum(n, lane, [t, x, tm, xm](int j) { return (t[j] - tm) * (x[j] - xm); });
    const double sxx = wsum(n, lane, [t, tm](int j) { const double d = t[j] - tm; return d * d; });
    Line l;
    l.b = sxy / sxx;
    l.a = xm - l.b * tm;
    return l;
}
__device__ __forceinline__ double line_at(const Line& l, double t) { return l.b * t + l.a; }

// mean and sum of squares about the mean of the residuals x - line(t) of n points
__device__ __forceinline__ void resid_stats(const Line& l, const double* t, const double* x, int n, int lane, double* mean, double* ss) {
    const double m = wsum(n, lane, [&l, t, x](int j) { return x[j] - line_at(l, t[j]); }) / (double)n;
    *ss = wsum(n, lane, [&l, t, x, m](int j) { const double d = (x[j] - line_at(l, t[j])) - m; return d * d; });
    *mean = m;
}

// scipy.stats.ttest_ind(equal_var=True) of the residuals about `l` of side 1 against those of side 2
__device__ __forceinline__ double pooled_t(const Line& l, const double* t1, const double* x1, int n1, const double* t2, const double* x2, int n2,
                                           int lane) {
    double m1, s1, m2, s2;
    resid_stats(l, t1, x1, n1, lane, &m1, &s1);
    resid_stats(l, t2, x2, n2, lane, &m2, &s2);
    const double v1 = s1 / (double)(n1 - 1), v2 = s2 / (double)(n2 - 1);
    const double df = (double)(n1 + n2 - 2);
    const double sp = ((double)(n1 - 1) * v1 + (double)(n2 - 1) * v2) / df;
    return (m1 - m2) / sqrt(sp * (1.0 / (double)n1 + 1.0 / (double)n2));
}

// ---- k_jump_select ------------------------------------------------------------------------------------------------------
struct SelectParams {
    const double* mag;          // [rows][nmax][K]
    const double *f0, *t;       // [rows][nmax]
    const int* len;             // [rows], or null: every row holds nmax frames
    int nmax, K;
    double thr;                 // mag_threshold
    double* m;                  // [rows][nmax], 0.0 from len on
    int* isel;                  // [rows][nmax], 0 from len on
    double *tsel, *fsel;        // [rows][nmax], 0.0 from nsel on
    int *nsel, *status;         // [rows]
};

__global__ __launch_bounds__(kRowThreads) void k_jump_select(SelectParams p) {
    __shared__ double wmax[kRowWaves];
    __shared__ int wflag[kRowWaves], wcnt[kRowWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, K = p.K, nmax = p.nmax;
    const int64_t r = blockIdx.x;
    const int n = row_len(p.len, r, nmax);
    const double* mag = p.mag + r * nmax * K;
    const double* t = p.t + r * nmax;
    const double* f0 = p.f0 + r * nmax;
    double* m = p.m + r * nmax;
    int* isel = p.isel + r * nmax;
    double* tsel = p.tsel + r * nmax;
    double* fsel = p.fsel + r * nmax;
    // pass 1: the magnitudes and their maximum
    double mx = -INFINITY;
    bool nan = false;
    for (int i = tid; i < nmax; i += kRowThreads) {
        double v = 0.0;
        if (i < n) {
            const double* row = mag + (int64_t)i * K;
            auto sq = [row](int k) { const double a = row[k]; return a * a; };
            v = sqrt(K <= 128 ? 0.0 + np_block_sum(sq, 0, K) : np_sum(sq, K));
            nan |= v != v;
            mx = v > mx ? v : mx;
        }
        m[i] = v;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const double o = __shfl_xor(mx, d, 64); mx = o > mx ? o : mx; }
    const bool wnan = __ballot(nan) != 0ull;
    if (lane == 0) { wmax[wave] = mx; wflag[wave] = wnan ? 1 : 0; }
    __syncthreads();
    double gmax = wmax[0];
    bool gnan = wflag[0] != 0;
#pragma unroll
    for (int w = 1; w < kRowWaves; w++) { gmax = wmax[w] > gmax ? wmax[w] : gmax; gnan |= wflag[w] != 0; }
    const double level = gnan ? NAN : gmax * p.thr;
    __syncthreads();                                                 // wflag is written again below
    // pass 2: ordered tiles (thread tid tests the frames it wrote in pass 1)
    int base = 0;
    bool badsel = false;
    for (int i0 = 0; i0 < nmax; i0 += kRowThreads) {
        const int i = i0 + tid;
        const bool sel = i < n && m[i] > level;
        double tv = 0.0, fv = 0.0;
        if (i < nmax) isel[i] = sel ? 1 : 0;
        if (sel) { tv = t[i]; fv = f0[i]; badsel |= tv != tv || fv != fv; }
        const unsigned long long bal = __ballot(sel);
        if (lane == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        int before = base, total = 0;
#pragma unroll
        for (int w = 0; w < kRowWaves; w++) {
            const int cw = wcnt[w];
            before += w < wave ? cw : 0;
            total += cw;
        }
        if (sel) {
            const int at = before + __popcll(bal & ((1ull << lane) - 1ull));   // at <= i < nmax
            tsel[at] = tv;
            fsel[at] = fv;
        }
        base += total;
        __syncthreads();
    }
    for (int i = base + tid; i < nmax; i += kRowThreads) { tsel[i] = 0.0; fsel[i] = 0.0; }
    const bool wbad = __ballot(badsel) != 0ull;
    if (lane == 0) wflag[wave] = wbad ? 1 : 0;
    __syncthreads();
    if (tid == 0) {
        bool bad = gnan;
#pragma unroll
        for (int w = 0; w < kRowWaves; w++) bad |= wflag[w] != 0;
        p.nsel[r] = base;
        p.status[r] = bad ? PVX_JUMP_NAN : 0;
    }
}

// ---- k_winstat ----------------------------------------------------------------------------------------------------------
constexpr int kWinStretch = 2 * PVX_JUMP_MAX_SIDE + 3;               // four consecutive indices' windows at hop 1

struct WinParams {
    const double *t, *x;        // [rows][nmax]
    const int* len;             // [rows] or null
    int nmax, kind, wl, wr, hop, flags;
    int per;                    // indices per workgroup: kRowWaves, or 1 when four indices' stretch is longer than the buffer
    int groups;                 // workgroups per row
    double* out;                // [rows][nmax], zeroed before the launch
};

__global__ __launch_bounds__(kRowThreads) void k_winstat(WinParams p) {
    __shared__ double st[kWinStretch], sx[kWinStretch];
    __shared__ double places[kRowWaves][6];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wl = p.wl, wr = p.wr;
    const int64_t r = blockIdx.x / p.groups;
    const int g = blockIdx.x % p.groups;
    const int n = row_len(p.len, r, p.nmax);
    const int last = n - wr;                                         // the indices are wl, wl + hop, .. < last
    const int i0 = wl + g * p.per * p.hop;                           // (groups is sized from nmax: no overflow)
    if (i0 >= last) return;                                          // (the whole workgroup)
    const double* t = p.t + r * p.nmax;
    const double* x = p.x + r * p.nmax;
    const int s0 = i0 - wl;
    const int slen = wl + (wr > 1 ? wr : 1) + (p.per - 1) * p.hop;   // <= kWinStretch (the host chose per so); the index itself
    for (int k = tid; k < slen; k += kRowThreads) {                  // is inside even when wr = 0
        const int j = s0 + k;
        st[k] = j < n ? t[j] : 0.0;
        sx[k] = j < n ? x[j] : 0.0;
    }
    __syncthreads();
    const int i = i0 + wave * p.hop;
    if (wave >= p.per || i >= last) return;                          // (a whole wave; no barrier below)
    const double* wt = st + wave * p.hop;                            // the window [i - wl, i + wr) is wt[0 .. wl + wr), the index wt[wl]
    const double* wx = sx + wave * p.hop;
    const int W = wl + wr;
    const double xi = wx[wl], ti = wt[wl];
    double res = NAN;
    if (p.kind == PVX_WIN_ZMEAN) {
        const double mean = wsum(W, lane, [wx](int j) { return wx[j]; }) / (double)W;
        const double ss = wsum(W, lane, [wx, mean](int j) { const double d = wx[j] - mean; return d * d; });
        res = (xi - mean) / sqrt(ss / (double)W);
    } else if (p.kind == PVX_WIN_ZMEDIAN) {
        if (!wave_any_nan(wx, W, lane)) {
            const PctPlan hi = pct_plan(W, 75.0), lo = pct_plan(W, 25.0);
            const int want[6] = {(W - 1) / 2, W / 2, hi.prev, hi.next, lo.prev, lo.next};
            select_ranks(wx, W, want, places[wave], lane);
            lds_sync();
            const double* q = places[wave];
            const double med = median_of(q[0], q[1], W);
            res = (xi - med) / (pct_value(q[2], q[3], hi.t) - pct_value(q[4], q[5], lo.t));
        }
    } else if (p.kind == PVX_WIN_LINREG) {
        const Line l = fit_line(wt, wx, W, lane);
        double mr, ss;
        resid_stats(l, wt, wx, W, lane, &mr, &ss);
        res = (xi - line_at(l, ti)) / sqrt(ss / (double)W);
    } else {
        const double* tr = wt + wl;
        const double* xr = wx + wl;
        double ttl = 0.0, ttr = 0.0;
        if (p.flags & PVX_WIN_USE_L) ttl = pooled_t(fit_line(wt, wx, wl, lane), wt, wx, wl, tr, xr, wr, lane);
        if (p.flags & PVX_WIN_USE_R) ttr = pooled_t(fit_line(tr, xr, wr, lane), tr, xr, wr, wt, wx, wl, lane);
        const int both = PVX_WIN_USE_L | PVX_WIN_USE_R;
        if ((p.flags & both) == both) res = (ttl + -ttr) / 2.0;
        else if (p.flags & PVX_WIN_USE_L) res = ttl;
        else if (p.flags & PVX_WIN_USE_R) res = -ttr;                // (neither: np.mean([]) is NaN)
    }
    if (lane == 0) p.out[r * p.nmax + i] = res;
}

// ---- k_jump_pick --------------------------------------------------------------------------------------------------------
struct PickParams {
    const double *zs, *t, *x;   // [rows][nmax]; zs null: idx and njump are the caller's and only the fits run
    const int* len;             // [rows] or null
    int nmax, nsl, maxjump;
    double thr;
    int *idx, *dir;             // [rows][maxjump]: ascending indices, +1 up / -1 down
    int* njump;                 // [rows]: the full count
    double *intcpts, *sumres;   // [rows][maxjump][2]
    int* status;                // [rows][maxjump]
};

// one side of calc_jump_params: the line through cnt points from `first` on, evaluated at ti, and sqrt(sum(res^2) / div)
__device__ __forceinline__ int jump_side(const double* t, const double* x, int first, int cnt, double ti, int div, int lane, double* at,
                                         double* rs) {
    if (cnt < 2) { *at = NAN; *rs = NAN; return PVX_JUMP_SHORT_SIDE; }
    const double* ts = t + first;
    const double* xs = x + first;
    const Line l = fit_line(ts, xs, cnt, lane);
    const double ss = wsum(cnt, lane, [&l, ts, xs](int j) { const double d = xs[j] - line_at(l, ts[j]); return d * d; });
    *at = line_at(l, ti);
    *rs = sqrt(ss / (double)div);
    return (*at != *at || *rs != *rs) ? PVX_JUMP_NAN : 0;
}

__global__ __launch_bounds__(kRowThreads) void k_jump_pick(PickParams p) {
    __shared__ int wcnt[kRowWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nmax = p.nmax;
    const int64_t r = blockIdx.x;
    const int n = row_len(p.len, r, nmax);
    const double* zs = p.zs + r * nmax;
    const double* t = p.t + r * nmax;
    const double* x = p.x + r * nmax;
    int* idx = p.idx + r * p.maxjump;
    int* dir = p.dir + r * p.maxjump;
    int base = 0;
    if (!p.zs) base = p.njump[r] < 0 ? 0 : p.njump[r];               // the caller's lists: only the fits run
    for (int i0 = 0; p.zs && i0 < n; i0 += kRowThreads) {            // (n is the workgroup's)
        const int i = i0 + tid;
        int d = 0;
        if (i >= 1 && i <= n - 2) {
            const double z = zs[i], zl = zs[i - 1], zr = zs[i + 1];
            if (z > zl && z > zr && z > p.thr) d = 1;
            else if (z < zl && z < zr && z < -p.thr) d = -1;
        }
        const unsigned long long bal = __ballot(d != 0);
        if (lane == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        int before = base, total = 0;
#pragma unroll
        for (int w = 0; w < kRowWaves; w++) {
            const int cw = wcnt[w];
            before += w < wave ? cw : 0;
            total += cw;
        }
        if (d != 0) {
            const int at = before + __popcll(bal & ((1ull << lane) - 1ull));
            if (at < p.maxjump) { idx[at] = i; dir[at] = d; }
        }
        base += total;
        __syncthreads();
    }
    __syncthreads();                                                 // the workgroup's idx writes are visible to its waves
    if (tid == 0 && p.zs) p.njump[r] = base;
    const int cnt = base < p.maxjump ? base : p.maxjump;
    for (int j = wave; j < cnt; j += kRowWaves) {
        const int i = idx[j];
        if (i < 0 || i >= n) {                                       // (a caller's index outside the row)
            if (lane == 0) {
                const int64_t o = (r * p.maxjump + j) * 2;
                p.intcpts[o] = p.intcpts[o + 1] = p.sumres[o] = p.sumres[o + 1] = NAN;
                p.status[r * p.maxjump + j] = PVX_JUMP_SHORT_SIDE;
            }
            continue;
        }
        const int il = i - p.nsl > 0 ? i - p.nsl : 0;
        const int ir = (int64_t)i + p.nsl < n ? i + p.nsl : n;
        const double ti = t[i];
        double al, rl, ar, rr;
        int st = jump_side(t, x, il, i - il, ti, i - il, lane, &al, &rl);
        st |= jump_side(t, x, i + 1, ir - i - 1, ti, ir - i, lane, &ar, &rr);
        if (lane == 0) {
            const int64_t o = (r * p.maxjump + j) * 2;
            p.intcpts[o] = al; p.intcpts[o + 1] = ar;
            p.sumres[o] = rl; p.sumres[o + 1] = rr;
            p.status[r * p.maxjump + j] = st;
        }
    }
}

}  // namespace

// ---- host side: launches on device rows -------------------------------------------------------------------------------------
int pvx_jump_select_run(const double* d_mag, const double* d_f0, const double* d_t, const int* d_len, int64_t rows, int nmax, int K, double thr,
                        double* d_m, int* d_isel, double* d_tsel, double* d_fsel, int* d_nsel, int* d_status, hipStream_t s,
                        const char** kernels) {
    if (rows <= 0) return PVX_OK;
    SelectParams p = {};
    p.mag = d_mag; p.f0 = d_f0; p.t = d_t; p.len = d_len; p.nmax = nmax; p.K = K; p.thr = thr;
    p.m = d_m; p.isel = d_isel; p.tsel = d_tsel; p.fsel = d_fsel; p.nsel = d_nsel; p.status = d_status;
    hipLaunchKernelGGL(k_jump_select, dim3((unsigned)rows), dim3(kRowThreads), 0, s, p);
    PVX_HIP_CHECK(hipGetLastError());
    *kernels = "k_jump_select";
    PVX_HIP_CHECK(hipStreamSynchronize(s));
    return PVX_OK;
}

int pvx_winstat_run(const double* d_t, const double* d_x, const int* d_len, int64_t rows, int nmax, int kind, int wl, int wr, int hop, int flags,
                    double* d_out, hipStream_t s, const char** kernels) {
    if (rows <= 0 || nmax <= 0) return PVX_OK;
    PVX_HIP_CHECK(hipMemsetAsync(d_out, 0, (size_t)rows * nmax * 8, s));
    const int64_t count = nmax - wr > wl ? ((int64_t)(nmax - wr - wl) + hop - 1) / hop : 0;   // the indices of a full row
    if (count > 0) {
        WinParams p = {};
        p.t = d_t; p.x = d_x; p.len = d_len; p.nmax = nmax; p.kind = kind; p.wl = wl; p.wr = wr; p.hop = hop; p.flags = flags; p.out = d_out;
        p.per = (int64_t)wl + (wr > 1 ? wr : 1) + (int64_t)(kRowWaves - 1) * hop <= kWinStretch ? kRowWaves : 1;
        p.groups = (int)((count + p.per - 1) / p.per);
        if (rows * p.groups > 0x7fffffffLL) { pvx_set_error("pvx_winstat: %lld rows of %d workgroups exceed a launch's grid", (long long)rows, p.groups); return PVX_ERR_UNSUPPORTED; }
        hipLaunchKernelGGL(k_winstat, dim3((unsigned)(rows * p.groups)), dim3(kRowThreads), 0, s, p);
        PVX_HIP_CHECK(hipGetLastError());
        *kernels = "k_winstat";
    }
    PVX_HIP_CHECK(hipStreamSynchronize(s));
    return PVX_OK;
}

int pvx_jump_pick_run(const double* d_zs, const double* d_t, const double* d_x, const int* d_len, int64_t rows, int nmax, double thr, int nsl,
                      int maxjump, int* d_idx, int* d_dir, int* d_njump, double* d_intcpts, double* d_sumres, int* d_status, hipStream_t s,
                      const char** kernels) {
    if (rows <= 0) return PVX_OK;
    PickParams p = {};
    p.zs = d_zs; p.t = d_t; p.x = d_x; p.len = d_len; p.nmax = nmax; p.nsl = nsl; p.maxjump = maxjump; p.thr = thr;
    p.idx = d_idx; p.dir = d_dir; p.njump = d_njump; p.intcpts = d_intcpts; p.sumres = d_sumres; p.status = d_status;
    hipLaunchKernelGGL(k_jump_pick, dim3((unsigned)rows), dim3(kRowThreads), 0, s, p);
    PVX_HIP_CHECK(hipGetLastError());
    *kernels = "k_jump_pick";
    PVX_HIP_CHECK(hipStreamSynchronize(s));
    return PVX_OK;
}

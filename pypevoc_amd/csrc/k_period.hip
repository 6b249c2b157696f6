// k_period.hip -- time-domain periodicity (pypevoc/Periodicity.py:98-236): PeriodSeries' per-frame
// similarity function (xcorr or amdf), its normalisation, voicing test, candidate peaks with quadratic
// refinement, the choice of the preferred candidate and the sort by strength.  Design: PERIODICITY.md.
//
// One 256-thread workgroup per frame (persistent: a workgroup walks frames fr, fr + grid, ...).
//   1. the windowed frame xw = (xs - mean(xs)) * wind (:104-111) goes to LDS (nwind <= kLdsMax) or to
//      the workgroup's slice of a global scratch (larger windows; read back through L1 / L2);
//   2. lanes own lags: a thread computes kR neighbouring lags over a sliding register window (two
//      memory reads per kR float64 FMAs / absolute differences), only over the lag ranges the frame
//      reads -- lo[0..1) and lo[1..2) given by the caller (the slices of :122-146 in numpy's clipping);
//   3. normaliser, first negative lag (xcorr), voicing, PeakFinder(minval, npeaks) (PeakFinder.py:
//      155-194) as ncand rounds of a block arg-max over the order (score desc, index asc), refinement
//      with the 3-point parabola (PeakFinder.py:331-372);
//   4. cand_method 'min' / 'similar' / other: preferred + sort_strength (:223-236) here; 'fft': the
//      caller runs a batched rocFFT of the frames written to `xw_out` and k_period_fft finishes.
// float64 throughout.  Outputs per frame: cand_period / cand_strength [ncand] (NaN beyond the count),
// ncands, preferred (-1: the reference's `preferred = []`).
#include <float.h>
#include <math.h>

#include <map>
#include <mutex>
#include <tuple>

#include "pvx_block.h"
#include "pvx_internal.h"
#include "pvx_mem.h"

namespace {

constexpr int kThreads = 256;
constexpr int kR = 4;              // lags per thread per pass
constexpr int kLdsMax = 6144;      // windows up to 48 KB of float64 stay in LDS

// block reductions in a fixed order (results do not depend on which workgroup runs a frame): pvx_block.h
using namespace pvxb;
static_assert(kThreads == kBlock, "the block reductions are written for 256 threads");

// PeakFinder(y, minval=..., npeaks=np).findpos() (PeakFinder.py:155-194) on y[0..m): pkmskamp[k] = y[k] - miny at
// interior maxima y[k-1] < y[k] >= y[k+1], 0 elsewhere; rounds take the best (score, index) below the previous pick
// while its score > th -- the reference's arg-max / overwrite loop without the overwrite.  out[] ascending, returns
// the count (block-uniform).  th = minamp - miny.
template <typename Y>
__device__ int select_peaks(Y y, int m, double miny, double th, int npeaks, int* out, Red& r) {
    int cnt = 0;
    double ps = INFINITY;
    int pk = -1;
    for (int round = 0; round < npeaks; round++) {
        double bs = -INFINITY;
        int bk = INT_MAX;
        for (int k = 1 + (int)threadIdx.x; k < m - 1; k += kThreads) {
            const double a = y(k - 1), b = y(k), c = y(k + 1);
            const double s = (a < b && b >= c) ? b - miny : 0.0;
            if ((s < ps || (s == ps && k > pk)) && better(s, k, bs, bk)) { bs = s; bk = k; }
        }
        block_argmax(bs, bk, r);
        if (!(bs > th) || bk == INT_MAX) break;
        if (threadIdx.x == 0) out[cnt] = bk;
        cnt++;
        ps = bs; pk = bk;
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                          // np.sort(pos)
        for (int a = 1; a < cnt; a++) {
            const int v = out[a];
            int b = a - 1;
            while (b >= 0 && out[b] > v) { out[b + 1] = out[b]; b--; }
            out[b + 1] = v;
        }
    }
    __syncthreads();
    return cnt;
}

// sort_strength (Periodicity.py:223-236): order = argsort(strength)[::-1] (ties: the higher index first), preferred
// follows its candidate.  Thread 0; writes the frame's outputs.  ord: LDS scratch of PVX_PERIOD_MAX_NCAND entries.
__device__ void finish_frame(const PeriodParams& p, int64_t fr, const double* per, const double* str, int cnt, int pref, int* ord) {
    for (int a = 0; a < cnt; a++) ord[a] = a;
    for (int a = 1; a < cnt; a++) {                                  // stable ascending by strength, then reversed
        const int v = ord[a];
        int b = a - 1;
        while (b >= 0 && str[ord[b]] > str[v]) { ord[b + 1] = ord[b]; b--; }
        ord[b + 1] = v;
    }
    double* op = p.cand_period + fr * p.ncand;
    double* os = p.cand_strength + fr * p.ncand;
    int np_ = -1;
    for (int a = 0; a < cnt; a++) {
        const int src = ord[cnt - 1 - a];
        op[a] = per[src];
        os[a] = str[src];
        if (src == pref) np_ = a;
    }
    for (int a = cnt; a < p.ncand; a++) { op[a] = NAN; os[a] = NAN; }
    p.ncands[fr] = cnt;
    p.preferred[fr] = cnt > 0 ? np_ : -1;
}

// similarity of lags [l0, l0 + kR) (clipped to lend): xcorr sum_i xw[i] * xw[i+l] / wnorm[l]; amdf
// sum_i |xw[i] - xw[i+l]| / (n - l) (Periodicity.py:38-50: every lag, divisor n - i)
template <bool AMDF>
__device__ void lag_block(const double* xw, int n, int l0, int lend, const double* wnorm, double* sim) {
    double acc[kR], b[kR];
#pragma unroll
    for (int j = 0; j < kR; j++) { acc[j] = 0.0; b[j] = (l0 + j < n) ? xw[l0 + j] : 0.0; }
    const int ifull = n - l0 - kR;                                   // i <= ifull: all kR lags have a partner
    int i = 0;
    for (; i <= ifull; i++) {
        const double a = xw[i];
#pragma unroll
        for (int j = 0; j < kR; j++) acc[j] = AMDF ? acc[j] + fabs(a - b[j]) : fma(a, b[j], acc[j]);
#pragma unroll
        for (int j = 0; j < kR - 1; j++) b[j] = b[j + 1];
        b[kR - 1] = (i + l0 + kR < n) ? xw[i + l0 + kR] : 0.0;
    }
    for (; i < n - l0; i++) {                                        // tail: the lags whose sums end earlier
        const double a = xw[i];
#pragma unroll
        for (int j = 0; j < kR; j++)
            if (i + l0 + j < n) { const double c = xw[i + l0 + j]; acc[j] = AMDF ? acc[j] + fabs(a - c) : fma(a, c, acc[j]); }
    }
#pragma unroll
    for (int j = 0; j < kR; j++) {
        const int l = l0 + j;
        if (l < lend && l < n) sim[l] = AMDF ? acc[j] / (double)(n - l) : acc[j] / wnorm[l];
    }
}

template <bool AMDF>
__device__ void lag_range(const double* xw, int n, int a, int e, const double* wnorm, double* sim) {
    for (int l0 = a + (int)threadIdx.x * kR; l0 < e; l0 += kThreads * kR) lag_block<AMDF>(xw, n, l0, e, wnorm, sim);
}

template <bool AMDF, bool INLDS>
__global__ __launch_bounds__(kThreads) void k_period(PeriodParams p) {
    extern __shared__ double lds[];
    __shared__ Red red;
    __shared__ int pk[PVX_PERIOD_MAX_NCAND], ord[PVX_PERIOD_MAX_NCAND];
    __shared__ double cper[PVX_PERIOD_MAX_NCAND], cstr[PVX_PERIOD_MAX_NCAND];
    const int n = p.nwind;
    double* sim = p.scratch + (size_t)blockIdx.x * (size_t)(INLDS ? n : 2 * n + kR);   // sim[n] (+ xw[n + kR] beyond LDS)
    double* xw = INLDS ? lds : sim + n;
    const int nwl = n / 2;                                           // floor(nwind / 2) (:104)
    for (int64_t fr = blockIdx.x; fr < p.nfr; fr += gridDim.x) {
        const int64_t st = p.idx[fr] - nwl;
        if (st < 0 || st + n > p.nsamp) {                            // the entry point checked this; never read outside x
            if (threadIdx.x == 0) { atomicOr(p.err, 1); p.ncands[fr] = 0; p.preferred[fr] = -1; }
            continue;
        }
        const double* xs = p.x + st;
        double s = 0.0;
        for (int i = threadIdx.x; i < n; i += kThreads) s += xs[i];
        const double mean = block_sum(s, red) / (double)n;
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const double v = (xs[i] - mean) * p.wind[i];
            xw[i] = v;
            if (p.xw_out) p.xw_out[fr * (int64_t)n + i] = v;
        }
        __syncthreads();
        lag_range<AMDF>(xw, n, p.lo[0], p.hi[0], p.wnorm, sim);
        lag_range<AMDF>(xw, n, p.lo[1], p.hi[1], p.wnorm, sim);
        __syncthreads();

        // normaliser: builtin max() over the slice [ns, ne) -- NaN when its first element is, else the max of the rest's numbers
        auto nval = [&](int j) { return AMDF ? sim[j] : sim[j >= n - 1 ? j - (n - 1) : (n - 1) - j]; };
        double v = -INFINITY;
        for (int j = p.ns + (int)threadIdx.x; j < p.ne; j += kThreads) v = fmax(v, nval(j));
        double norm = block_fmax(v, red);
        if (p.ns >= p.ne) norm = NAN;                                 // (the entry point refuses an empty slice)
        else if (nval(p.ns) != nval(p.ns)) norm = NAN;

        int imin;
        if (AMDF) {
            imin = p.mindelay;
        } else {                                                     // first lag >= 0 with xc < 0, over every lag (:136-141)
            int fn = INT_MAX;
            for (int l = threadIdx.x; l < p.hi[0]; l += kThreads) if (sim[l] < 0.0) fn = min(fn, l);
            fn = block_imin(fn, red);
            int done = p.hi[0];
            while (fn == INT_MAX && done < n) {                      // rare: continue past the lags read
                const int e = min(n, done + kThreads * kR);
                __syncthreads();
                lag_range<false>(xw, n, done, e, p.wnorm, sim);
                __syncthreads();
                for (int l = done + (int)threadIdx.x; l < e; l += kThreads) if (sim[l] < 0.0) fn = min(fn, l);
                fn = block_imin(fn, red);
                done = e;
            }
            imin = max(fn == INT_MAX ? p.mindelay : fn, p.mindelay);
        }
        const int pend = min(p.maxdelay, n);
        const int m = pend > imin ? pend - imin : 0;
        auto y = [&](int k) {
            const double c = sim[imin + k];
            return AMDF ? (norm - c) / norm : c / norm;
        };
        // voicing: len(xcpos) > 0 and max(xcpos) > vthresh (builtin max: NaN first element -> NaN)
        double ymax = -INFINITY, ymin = INFINITY;
        bool ynan = false;
        for (int k = threadIdx.x; k < m; k += kThreads) { const double t = y(k); ymax = fmax(ymax, t); ynan |= (t != t); ymin = t < ymin ? t : ymin; }
        ymax = block_fmax(ymax, red);
        const double miny = block_nanmin(ynan ? NAN : ymin, red);
        const bool voiced = m > 0 && y(0) == y(0) && ymax > p.vthresh;
        int cnt = 0;
        if (voiced && m < 3) {                                       // PeakFinder on 1-2 values: the reference raises ValueError
            if (threadIdx.x == 0) atomicOr(p.err, 2);
        } else if (voiced && miny == miny) {
            const double minamp = p.threshold != 0.0 ? p.threshold : miny;   // `if not self.minamp` (PeakFinder.py:69)
            cnt = select_peaks(y, m, miny, minamp - miny, p.ncand, pk, red);
            if (threadIdx.x == 0) {
                for (int q = 0; q < cnt; q++) {                      // refine() (PeakFinder.py:344-372)
                    const int ps = pk[q];
                    const double s0 = y(ps - 1), s1 = y(ps), s2 = y(ps + 1);
                    double fpos = (double)ps, fval = s1;
                    if (s1 > s0 && s1 >= s2) {
                        const double c = s1, b = (s2 - s0) / 2, a = (s2 + s0) / 2 - c;
                        const double lpos = -b / 2 / a;
                        fpos = (double)ps + lpos;
                        fval = a * lpos * lpos + b * lpos + c;
                    }
                    fpos = fpos < 0.0 ? 0.0 : (fpos > (double)(m - 1) ? (double)(m - 1) : fpos);   // np.interp on arange(m)
                    cper[q] = fpos + (double)imin;
                    cstr[q] = fval;
                }
            }
        }
        if (threadIdx.x == 0) {
            if (p.cand_method == PVX_CAND_FFT) {                     // k_period_fft finishes the frame
                double* op = p.cand_period + fr * p.ncand;
                double* os = p.cand_strength + fr * p.ncand;
                for (int q = 0; q < p.ncand; q++) { op[q] = q < cnt ? cper[q] : NAN; os[q] = q < cnt ? cstr[q] : NAN; }
                p.ncands[fr] = cnt;
                p.preferred[fr] = cnt > 0 ? 0 : -1;
            } else {
                int pref = 0;
                for (int q = 1; q < cnt; q++) {
                    if (p.cand_method == PVX_CAND_MIN && cper[q] < cper[pref]) pref = q;          // np.argmin
                    if (p.cand_method == PVX_CAND_SIMILAR && cstr[q] > cstr[pref]) pref = q;      // np.argmax
                }
                finish_frame(p, fr, cper, cstr, cnt, pref, ord);
            }
        }
        __syncthreads();
    }
}

// cand_method 'fft' (Periodicity.py:169-188): |FFT(xw)| over bins 0 .. nwind/2 - 1, its top ncand peaks (PeakFinder
// defaults: threshold min(y), integer positions), the bins with fval > max(fval * fftthresh), their periods nwind / fpos;
// preferred = the candidate nearest to one of them.  Then sort_strength.  spec: [frames of the chunk][nwind/2 + 1].
__global__ __launch_bounds__(kThreads) void k_period_fft(PeriodParams p, const double2* spec, int64_t nfr_chunk) {
    __shared__ Red red;
    __shared__ int pk[PVX_PERIOD_MAX_NCAND], ord[PVX_PERIOD_MAX_NCAND];
    __shared__ double cper[PVX_PERIOD_MAX_NCAND], cstr[PVX_PERIOD_MAX_NCAND];
    const int n = p.nwind, m = n / 2, ldo = n / 2 + 1;
    for (int64_t q = blockIdx.x; q < nfr_chunk; q += gridDim.x) {
        const int64_t fr = q;
        const int cnt = p.ncands[fr];
        if (cnt == 0) continue;                                      // block-uniform; k_period wrote the frame
        const double2* row = spec + q * ldo;
        auto y = [&](int k) { return hypot(row[k].x, row[k].y); };
        double mn = INFINITY;
        bool nan = false;
        for (int k = threadIdx.x; k < m; k += kThreads) { const double t = y(k); nan |= (t != t); mn = t < mn ? t : mn; }
        const double miny = block_nanmin(nan ? NAN : mn, red);
        const int nf = miny == miny ? select_peaks(y, m, miny, 0.0, p.ncand, pk, red) : 0;
        if (threadIdx.x == 0) {
            const double* ip = p.cand_period + fr * p.ncand;
            const double* is = p.cand_strength + fr * p.ncand;
            for (int a = 0; a < cnt; a++) { cper[a] = ip[a]; cstr[a] = is[a]; }
            double thr = -INFINITY;
            for (int a = 0; a < nf; a++) thr = fmax(thr, y(pk[a]) * p.fftthresh);
            int pref = 0;
            double best = INFINITY;
            bool any = false;
            for (int c = 0; c < cnt; c++) {
                double d = INFINITY;
                for (int a = 0; a < nf; a++) {
                    if (!(y(pk[a]) > thr)) continue;
                    any = true;
                    d = fmin(d, fabs((double)n / (double)pk[a] - cper[c]));
                }
                if (d < best) { best = d; pref = c; }
            }
            if (!any) pref = 0;
            finish_frame(p, fr, cper, cstr, cnt, pref, ord);
        }
        __syncthreads();
    }
}

// wnorm = np.correlate(w, w, "full") at lags 0 .. nwind-1 (Periodicity.py:334-344)
__global__ __launch_bounds__(kThreads) void k_window_acf(const double* w, int n, double* out) {
    const int l = blockIdx.x * kThreads + threadIdx.x;
    if (l >= n) return;
    double s = 0.0;
    for (int i = 0; i + l < n; i++) s = fma(w[i], w[i + l], s);
    out[l] = s;
}

// Per-device workspace of pvx_period_run, kept for the process and reused by every call: grow-only buffers and ONE rocFFT
// plan (the nwind of the last 'fft' request, with a fixed batch: a call transforms whole chunks, its own frames first).
// Memory therefore stays flat across calls on signals of any length; a new nwind replaces the plan.  The workspace's mutex
// is held for a whole call, execution and the final synchronisation included: two threads on one device take turns.
struct PeriodWs {
    std::mutex mu;
    int fft_nwind = 0;
    int64_t fft_batch = 0;
    RealFft fft;
    DevMem work;                                                     // rocFFT's work buffer: kept when a new nwind replaces the plan
    DevMem wind, wnorm, idx, scratch, frames, spec, err;
};
std::mutex g_ws_mu;
std::map<int, PeriodWs*> g_ws;                                       // device -> workspace (never erased)


// frames per 'fft' chunk: the rocFFT input / output of a chunk stay near 64 MB each
int64_t fft_chunk(int nwind) {
    const int64_t c = ((int64_t)64 << 20) / ((int64_t)nwind * 8);
    return c < 1 ? 1 : c;
}

// (the buffers are exactly as large as the largest request so far; no work is pending when one is replaced: every call ends
// synchronised)
int ensure_fft(PeriodWs& w, int nwind) {
    if (w.fft && w.fft_nwind == nwind) return PVX_OK;
    w.fft_nwind = 0; w.fft_batch = 0;
    const int64_t batch = fft_chunk(nwind);
    rocfft_status st;
    switch (w.fft.create((size_t)nwind, (size_t)batch, rocfft_precision_double, rocfft_placement_notinplace, (size_t)nwind, (size_t)(nwind / 2 + 1), &st)) {
        case RealFft::done: break;
        case RealFft::describe: pvx_set_error("rocfft_plan_description_create failed: rocfft_status %d", (int)st); return PVX_ERR_HIP;
        case RealFft::plan: pvx_set_error("rocfft_plan_create(nwind=%d, batch=%lld) failed: %d", nwind, (long long)batch, (int)st); return PVX_ERR_HIP;
        case RealFft::info: pvx_set_error("rocfft execution setup (nwind=%d) failed", nwind); return PVX_ERR_HIP;
    }
    if (const size_t wb = w.fft.work_bytes()) {
        int rc;
        if ((rc = w.work.grow(wb, Sizing::exact)) != PVX_OK) { w.fft.reset(); return rc; }
        if (w.fft.set_work(w.work.get(), wb) != rocfft_status_success) {
            w.fft.reset();
            pvx_set_error("rocfft set_work_buffer failed");
            return PVX_ERR_HIP;
        }
    }
    w.fft_nwind = nwind;
    w.fft_batch = batch;
    return PVX_OK;
}

int run_locked(PeriodWs& w, PeriodParams p, const double* h_wind, const int64_t* h_idx, hipStream_t s) {
    const int n = p.nwind;
    const bool inlds = n <= kLdsMax;
    const bool fft = p.cand_method == PVX_CAND_FFT;
    int rc;
    if ((rc = w.wind.grow((size_t)n * 8, Sizing::exact)) != PVX_OK || (rc = w.idx.grow((size_t)p.nfr * 8, Sizing::exact)) != PVX_OK ||
        (rc = w.err.grow(4, Sizing::exact)) != PVX_OK) return rc;
    PVX_HIP_CHECK(hipMemcpyAsync(w.wind.get(), h_wind, (size_t)n * 8, hipMemcpyHostToDevice, s));
    PVX_HIP_CHECK(hipMemcpyAsync(w.idx.get(), h_idx, (size_t)p.nfr * 8, hipMemcpyHostToDevice, s));
    PVX_HIP_CHECK(hipMemsetAsync(w.err.get(), 0, 4, s));
    p.wind = w.wind.as<const double>();
    p.idx = w.idx.as<const int64_t>();
    p.err = w.err.as<int>();
    if (!p.amdf) {
        if ((rc = w.wnorm.grow((size_t)n * 8, Sizing::exact)) != PVX_OK) return rc;
        hipLaunchKernelGGL(k_window_acf, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, s, p.wind, n, w.wnorm.as<double>());
        PVX_HIP_CHECK(hipGetLastError());
        p.wnorm = w.wnorm.as<const double>();
    }
    int64_t chunk = p.nfr;
    if (fft) {
        if ((rc = ensure_fft(w, n)) != PVX_OK) return rc;
        chunk = w.fft_batch < p.nfr ? w.fft_batch : p.nfr;
        // the plan transforms fft_batch rows: rows beyond a call's frames hold zeros or an earlier call's frames, never read
        const bool fresh = w.frames.cap() < (size_t)w.fft_batch * n * 8;
        if ((rc = w.frames.grow((size_t)w.fft_batch * n * 8, Sizing::exact)) != PVX_OK ||
            (rc = w.spec.grow((size_t)w.fft_batch * (n / 2 + 1) * 16, Sizing::exact)) != PVX_OK) return rc;
        if (fresh) PVX_HIP_CHECK(hipMemsetAsync(w.frames.get(), 0, w.frames.cap(), s));
    }
    const int64_t gmax = inlds ? 1024 : 512;
    const int64_t grid = chunk < gmax ? chunk : gmax;
    if ((rc = w.scratch.grow((size_t)grid * (size_t)(inlds ? n : 2 * n + kR) * 8, Sizing::exact)) != PVX_OK) return rc;
    p.scratch = w.scratch.as<double>();
    const size_t lds = inlds ? (size_t)n * 8 : 0;
    PeriodParams q = p;
    for (int64_t f0 = 0; f0 < p.nfr; f0 += chunk) {
        const int64_t nf = p.nfr - f0 < chunk ? p.nfr - f0 : chunk;
        // the kernels index frames from the chunk's first: shift the inputs and outputs to it
        q.nfr = nf;
        q.idx = p.idx + f0;
        q.cand_period = p.cand_period + f0 * p.ncand;
        q.cand_strength = p.cand_strength + f0 * p.ncand;
        q.ncands = p.ncands + f0;
        q.preferred = p.preferred + f0;
        q.xw_out = fft ? w.frames.as<double>() : nullptr;
        const unsigned g = (unsigned)(nf < grid ? nf : grid);
        if (p.amdf) {
            if (inlds) hipLaunchKernelGGL((k_period<true, true>), dim3(g), dim3(kThreads), lds, s, q);
            else hipLaunchKernelGGL((k_period<true, false>), dim3(g), dim3(kThreads), 0, s, q);
        } else {
            if (inlds) hipLaunchKernelGGL((k_period<false, true>), dim3(g), dim3(kThreads), lds, s, q);
            else hipLaunchKernelGGL((k_period<false, false>), dim3(g), dim3(kThreads), 0, s, q);
        }
        PVX_HIP_CHECK(hipGetLastError());
        if (fft) {
            PVX_FFT_CHECK(w.fft.execute(w.frames.get(), w.spec.get(), s));
            hipLaunchKernelGGL(k_period_fft, dim3(g), dim3(kThreads), 0, s, q, w.spec.as<const double2>(), nf);
            PVX_HIP_CHECK(hipGetLastError());
        }
    }
    int herr = 0;
    PVX_HIP_CHECK(hipMemcpyAsync(&herr, w.err.get(), 4, hipMemcpyDeviceToHost, s));
    PVX_HIP_CHECK(hipStreamSynchronize(s));                          // the workspace is free for the next call from here on
    if (herr & 1) { pvx_set_error("pvx_periodicity: a frame centre leaves the signal"); return PVX_ERR_INVALID; }
    if (herr & 2) {
        pvx_set_error("pvx_periodicity: a voiced frame has fewer than 3 similarity values to pick peaks from (the reference raises ValueError)");
        return PVX_ERR_INVALID;
    }
    return PVX_OK;
}

}  // namespace

// Runs the whole periodicity request on `s`: p.x and the outputs are device pointers, h_wind [nwind] and h_idx [nfr] host
// arrays; the lag ranges, the normaliser slice and the scalars filled in by the entry point.  Synchronises `s`.
int pvx_period_run(PeriodParams p, const double* h_wind, const int64_t* h_idx, hipStream_t s) {
    if (p.nfr <= 0) return PVX_OK;
    int dev = 0;
    PVX_HIP_CHECK(hipGetDevice(&dev));
    PeriodWs* w;
    {
        std::lock_guard<std::mutex> lk(g_ws_mu);
        PeriodWs*& e = g_ws[dev];
        if (!e) e = new PeriodWs();
        w = e;
    }
    std::lock_guard<std::mutex> lk(w->mu);
    return run_locked(*w, p, h_wind, h_idx, s);
}

// k_xcorr.hip -- full cross-correlations of two signals and their peaks, block by block: the device half of determineDelay,
// block_delay and maxdelwind (pypevoc/TransferFunctions.py:80-109, :188-196, :199-244).  float64 throughout.  Design and
// numbers: DELAY.md.
// Block b of a call reads a[b * delta : .. + la] and v[b * delta : .. + lv]:
//   a', v'  the block detrended on its own (none / mean / least-squares line, closed form), then times its window
//   c[k] = sum_m a'[m + k - (lv-1)] v'[m],  k = 0 .. la + lv - 2                  (numpy's correlate(a', v', "full"))
//   lag = the k of the largest c[k] (or |c[k]|), the lowest k of an exact tie; peak = c[lag]
//
// Two routes, chosen once per call:
//   direct  max(la, lv) <= PVX_XCORR_DIRECT_MAX: k_xcorr_direct, a workgroup per block (persistent over the blocks), both
//           prepared blocks in LDS (at most 32 KB), a lag per lane: lane t of a wave reads a'[m + k_t - (lv-1)] -- 8-byte
//           words at consecutive addresses, all 64 banks of a 32-lane half once -- and v'[m], one address for the wave (a
//           broadcast).  A lag is one lane's sum in ascending m.
//   fft     everything else (PVX_XCORR_FFT in the environment: every length): k_xcorr_prep writes a' and the reversed v'
//           zero-padded to P doubles, P the smallest power of two >= la + lv - 1 (never below 16); two batched real rocFFTs,
//           k_xcorr_mul (A V per bin), the inverse real rocFFT, k_xcorr_peak (scales by 1/P, exact for a power of two).
// Every kernel works per block, with XC_THREADS threads whatever the sizes, and adds in a fixed order (a thread its strided
// elements in ascending index, then a tree over the threads): no atomics, and the bits depend neither on the grid nor on how a
// call was cut into batches or chunks.  The arg-max is a workgroup reduction in the order (value descending, index ascending).
#include <math.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <vector>

#include "pvx_internal.h"
#include "pvx_mem.h"
#include "pvx_host.h"

namespace {

constexpr int XC_THREADS = 256;
constexpr int XC_MIN_P = 16;
constexpr int XC_NO_LAG = 0x7fffffff;

struct XcParams {
    const void* a;            // first sample of block 0 ...
    const void* v;            // ... of the second signal
    int64_t delta;            // samples between block starts
    int64_t nblk;             // blocks of this launch
    int la, lv, nlag;         // nlag = la + lv - 1
    int detrend, use_abs;
    const double* win_a;      // [la] device, null: ones
    const double* win_v;      // [lv]
    int32_t* lag;             // [nblk]
    double* peak;             // [nblk]
    double* corr;             // [nblk][nlag], nullable
    double* ta;               // fft route: [..][P] a' zero padded; after the inverse transform P * c[k]
    double* tv;               // fft route: [..][P] reversed v' zero padded
    double2* sa;              // fft route: [..][P/2 + 1] half spectra of ta ...
    const double2* sv;        // ... and of tv
    int P;
};

// the sum of the workgroup's `part`s, the same value in every thread: a tree over the threads in a fixed order
__device__ __forceinline__ double xc_sum(double part, double* red) {
    const int t = threadIdx.x;
    __syncthreads();                                                  // red may still be read from the call before
    red[t] = part;
    __syncthreads();
    for (int s = XC_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}

// mean and slope (against the centred index i - (n-1)/2) of the least-squares line through ld(0 .. n-1); what `mode` does not
// remove is 0.  sum (i - c)^2 = n (n^2 - 1) / 12
template <class Load> __device__ __forceinline__ void xc_trend(Load ld, int n, int mode, double* red, double& mean, double& slope) {
    mean = 0.0; slope = 0.0;
    if (mode == PVX_DETREND_NONE) return;
    double part = 0.0;
    for (int i = threadIdx.x; i < n; i += XC_THREADS) part += ld(i);
    mean = xc_sum(part, red) / (double)n;
    if (mode != PVX_DETREND_LINEAR || n < 2) return;
    const double c = 0.5 * (double)(n - 1);
    part = 0.0;
    for (int i = threadIdx.x; i < n; i += XC_THREADS) part += ((double)i - c) * (ld(i) - mean);
    slope = xc_sum(part, red) / ((double)n * ((double)n * (double)n - 1.0) / 12.0);
}

__device__ __forceinline__ double xc_prepared(double x, int i, int n, int mode, double mean, double slope, const double* win) {
    double y = x;
    if (mode != PVX_DETREND_NONE) y = (x - mean) - slope * ((double)i - 0.5 * (double)(n - 1));
    return win ? y * win[i] : y;
}

// a thread's best lag so far, then the workgroup's: value descending, index ascending; thread 0 writes the block's result
struct XcBest {
    double key, val;
    int idx;
};
__device__ __forceinline__ void xc_take(XcBest& b, double c, int k, int use_abs) {
    const double key = use_abs ? fabs(c) : c;
    if (b.idx == XC_NO_LAG || key > b.key) { b.key = key; b.val = c; b.idx = k; }      // ascending k: strict > keeps the lowest
}
__device__ __forceinline__ void xc_best_out(XcBest b, double* rkey, double* rval, int* ridx, int32_t* lag, double* peak) {
    const int t = threadIdx.x;
    __syncthreads();
    rkey[t] = b.key; rval[t] = b.val; ridx[t] = b.idx;
    __syncthreads();
    for (int s = XC_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            const int i2 = ridx[t + s], i1 = ridx[t];
            const double k2 = rkey[t + s], k1 = rkey[t];
            if (i2 != XC_NO_LAG && (i1 == XC_NO_LAG || k2 > k1 || (k2 == k1 && i2 < i1))) { rkey[t] = k2; rval[t] = rval[t + s]; ridx[t] = i2; }
        }
        __syncthreads();
    }
    if (t == 0) {
        *lag = ridx[0] == XC_NO_LAG ? 0 : ridx[0];
        *peak = rval[0] + 0.0;                                        // (a silent block's -0.0 becomes +0.0)
    }
}

// ---- direct route ----------------------------------------------------------------------------------------------------
// LDS: a' [la] | v' [lv] | the reductions' 3 x XC_THREADS words
template <typename InT> __global__ __launch_bounds__(XC_THREADS) void k_xcorr_direct(XcParams p) {
    extern __shared__ __attribute__((aligned(16))) double xc_lds[];
    double* const A = xc_lds;
    double* const V = A + p.la;
    double* const red = V + p.lv;
    double* const rval = red + XC_THREADS;
    int* const ridx = (int*)(rval + XC_THREADS);
    const int t = threadIdx.x;
    const int la = p.la, lv = p.lv;
    for (int64_t b = blockIdx.x; b < p.nblk; b += gridDim.x) {
        const InT* const xa = (const InT*)p.a + b * p.delta;
        const InT* const xv = (const InT*)p.v + b * p.delta;
        __syncthreads();                                              // the block before is done with A and V
        for (int i = t; i < la; i += XC_THREADS) A[i] = (double)xa[i];
        for (int i = t; i < lv; i += XC_THREADS) V[i] = (double)xv[i];
        __syncthreads();
        double mean, slope;
        xc_trend([&](int i) { return A[i]; }, la, p.detrend, red, mean, slope);
        for (int i = t; i < la; i += XC_THREADS) A[i] = xc_prepared(A[i], i, la, p.detrend, mean, slope, p.win_a);
        xc_trend([&](int i) { return V[i]; }, lv, p.detrend, red, mean, slope);
        for (int i = t; i < lv; i += XC_THREADS) V[i] = xc_prepared(V[i], i, lv, p.detrend, mean, slope, p.win_v);
        __syncthreads();
        XcBest best = {0.0, 0.0, XC_NO_LAG};
        double* const co = p.corr ? p.corr + b * (int64_t)p.nlag : nullptr;
        for (int k = t; k < p.nlag; k += XC_THREADS) {
            const int off = k - (lv - 1);                             // a' index = m + off, inside 0 .. la - 1
            const int mlo = off < 0 ? -off : 0;
            const int mhi = la - 1 - off < lv - 1 ? la - 1 - off : lv - 1;
            double s = 0.0;
            for (int m = mlo; m <= mhi; m++) s += A[m + off] * V[m];
            if (co) co[k] = s;
            xc_take(best, s, k, p.use_abs);
        }
        xc_best_out(best, red, rval, ridx, p.lag + b, p.peak + b);
    }
}

// ---- fft route -------------------------------------------------------------------------------------------------------
// blockIdx.y = 0: a' into ta[b][0 .. la), zeros up to P; 1: v' reversed into tv[b][0 .. lv), zeros up to P
template <typename InT> __global__ __launch_bounds__(XC_THREADS) void k_xcorr_prep(XcParams p) {
    __shared__ double red[XC_THREADS];
    const bool second = blockIdx.y != 0;
    const int64_t b = blockIdx.x;
    const int n = second ? p.lv : p.la;
    const InT* const x = (const InT*)(second ? p.v : p.a) + b * p.delta;
    const double* const win = second ? p.win_v : p.win_a;
    double* const out = (second ? p.tv : p.ta) + b * (int64_t)p.P;
    double mean, slope;
    xc_trend([&](int i) { return (double)x[i]; }, n, p.detrend, red, mean, slope);
    for (int j = threadIdx.x; j < p.P; j += XC_THREADS) {
        const int i = second ? n - 1 - j : j;
        out[j] = j < n ? xc_prepared((double)x[i], i, n, p.detrend, mean, slope, win) : 0.0;
    }
}

// sa[i] *= sv[i] over the half spectra of the launch's blocks
__global__ __launch_bounds__(XC_THREADS) void k_xcorr_mul(double2* sa, const double2* sv, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * XC_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * XC_THREADS) {
        const double2 x = sa[i], y = sv[i];
        sa[i] = make_double2(x.x * y.x - x.y * y.y, x.x * y.y + x.y * y.x);
    }
}

// a workgroup per block: c[k] = ta[b][k] / P, the optional copy, the arg-max
__global__ __launch_bounds__(XC_THREADS) void k_xcorr_peak(XcParams p) {
    __shared__ double rkey[XC_THREADS];
    __shared__ double rval[XC_THREADS];
    __shared__ int ridx[XC_THREADS];
    const int64_t b = blockIdx.x;
    const double* const c = p.ta + b * (int64_t)p.P;
    const double inv = 1.0 / (double)p.P;
    double* const co = p.corr ? p.corr + b * (int64_t)p.nlag : nullptr;
    XcBest best = {0.0, 0.0, XC_NO_LAG};
    for (int k = threadIdx.x; k < p.nlag; k += XC_THREADS) {
        const double s = c[k] * inv;
        if (co) co[k] = s;
        xc_take(best, s, k, p.use_abs);
    }
    xc_best_out(best, rkey, rval, ridx, p.lag + b, p.peak + b);
}

// ---- per-device workspace: the windows of the call, the fft route's buffers and its plans (kept for the process, grow-only,
// held for a whole call, the final synchronisation included: callers on one device take turns)
struct XcPlan {
    RealFft fwd, inv;                                                 // each with its own work buffer
    int64_t batch = 0;                                                // blocks per execution: fixed per P
};
struct XcorrWs {
    std::mutex mu;
    std::vector<double> h_win;                                        // host image of `win` (alive until the call's copy is done)
    DevMem win, ta, tv, sa, sv;
    std::map<int, XcPlan> plans;                                      // P -> the forward and the inverse plan
};
std::mutex g_xc_mu;
std::map<int, XcorrWs*> g_xc;                                         // device -> workspace (never erased)
constexpr size_t kMaxPlans = 8;                                      // padded lengths with live plans

int workspace(XcorrWs** ws) {
    int dev = 0;
    PVX_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_xc_mu);
    XcorrWs*& e = g_xc[dev];
    if (!e) e = new XcorrWs();
    *ws = e;
    return PVX_OK;
}

// blocks per rocFFT execution: a padded buffer stays near 32 MB.  Fixed per P, whatever the call's block count or chunking: a
// block's transform is the work of one plan
int64_t plan_batch(int P) {
    const int64_t c = ((int64_t)32 << 20) / ((int64_t)P * 8);
    return c < 1 ? 1 : c;
}

int own_work(RealFft& f) {
    if (const size_t wb = f.work_bytes()) {
        if (f.work.alloc(wb) != PVX_OK) { pvx_set_error("hipMalloc(rocfft work, %zu) failed", wb); return PVX_ERR_ALLOC; }
        if (f.set_work(f.work.get(), wb) != rocfft_status_success) { pvx_set_error("rocfft set_work_buffer failed"); return PVX_ERR_HIP; }
    }
    return PVX_OK;
}

int ensure_plan(XcorrWs& w, int P, XcPlan** out) {
    auto it = w.plans.find(P);
    if (it != w.plans.end()) { *out = &it->second; return PVX_OK; }
    if (w.plans.size() >= kMaxPlans) w.plans.clear();
    XcPlan xp;
    xp.batch = plan_batch(P);
    const size_t nh = (size_t)P / 2 + 1;
    rocfft_status st;
    RealFft::Step step = xp.fwd.create((size_t)P, (size_t)xp.batch, rocfft_precision_double, rocfft_placement_notinplace, (size_t)P, nh, &st);
    if (step == RealFft::done)
        step = xp.inv.create_inverse((size_t)P, (size_t)xp.batch, rocfft_precision_double, rocfft_placement_notinplace, nh, (size_t)P, &st);
    if (step != RealFft::done) {
        pvx_set_error("pvx_xcorr_peak: rocFFT plan (P=%d, batch=%lld) failed at step %d: rocfft_status %d", P, (long long)xp.batch, (int)step, (int)st);
        return PVX_ERR_HIP;
    }
    int rc;
    if ((rc = own_work(xp.fwd)) != PVX_OK || (rc = own_work(xp.inv)) != PVX_OK) return rc;
    *out = &(w.plans[P] = std::move(xp));
    return PVX_OK;
}

int ncus() {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) return v;
    return 256;
}

size_t device_limit() { return pvx_device_bytes_limit((size_t)2 << 30); }   // per buffer

int run_locked(XcorrWs& w, XcParams p, int x_dtype, const double* h_win_a, const double* h_win_v, hipStream_t s, const char** kernels) {
    int rc;
    // the windows of the call: [win_a | win_v], either may be missing
    std::vector<double>& hw = w.h_win;
    hw.clear();
    if (h_win_a) hw.insert(hw.end(), h_win_a, h_win_a + p.la);
    if (h_win_v) hw.insert(hw.end(), h_win_v, h_win_v + p.lv);
    if (!hw.empty()) {
        if ((rc = w.win.grow(hw.size() * 8, Sizing::exact)) != PVX_OK) return rc;
        PVX_HIP_CHECK(hipMemcpyAsync(w.win.get(), hw.data(), hw.size() * 8, hipMemcpyHostToDevice, s));
        p.win_a = h_win_a ? w.win.as<const double>() : nullptr;
        p.win_v = h_win_v ? w.win.as<const double>() + (h_win_a ? p.la : 0) : nullptr;
    }
    if (!pvx_xcorr_fft_route(p.la, p.lv)) {
        const void* fn = nullptr;
        switch (x_dtype) {
            case PVX_F32: fn = (const void*)k_xcorr_direct<float>; break;
            case PVX_F64: fn = (const void*)k_xcorr_direct<double>; break;
            default: fn = (const void*)k_xcorr_direct<int16_t>; break;
        }
        const size_t lds = (size_t)(p.la + p.lv) * 8 + (size_t)XC_THREADS * (8 + 8 + 4);
        int per_cu = pvx_resident_blocks(fn, XC_THREADS, lds);
        if (per_cu < 1) per_cu = 4;
        const int64_t grid = std::min<int64_t>(p.nblk, (int64_t)ncus() * per_cu);
        void* args[] = {&p};
        PVX_HIP_CHECK(hipLaunchKernel(fn, dim3((unsigned)grid), dim3(XC_THREADS), args, lds, s));
        *kernels = "k_xcorr_direct";
    } else {
        const int P = pvx_xcorr_padded(p.la, p.lv);
        XcPlan* xp = nullptr;
        if ((rc = ensure_plan(w, P, &xp)) != PVX_OK) return rc;
        const int64_t nh = P / 2 + 1;
        const int64_t B = xp->batch;
        if ((rc = w.ta.grow((size_t)(B * P) * 8, Sizing::exact)) != PVX_OK || (rc = w.tv.grow((size_t)(B * P) * 8, Sizing::exact)) != PVX_OK ||
            (rc = w.sa.grow((size_t)(B * nh) * 16, Sizing::exact)) != PVX_OK || (rc = w.sv.grow((size_t)(B * nh) * 16, Sizing::exact)) != PVX_OK) return rc;
        // blocks of a pass: what the plan holds, and no more than fill PVX_MAX_DEVICE_BYTES of a buffer (at least one)
        const int64_t fit = std::max<int64_t>(1, (int64_t)(device_limit() / ((size_t)nh * 16)));
        const int64_t per = std::min(B, fit);
        const size_t es = x_dtype == PVX_F64 ? 8 : (x_dtype == PVX_F32 ? 4 : 2);
        const char* const a0 = (const char*)p.a;
        const char* const v0 = (const char*)p.v;
        int32_t* const lag0 = p.lag;
        double* const peak0 = p.peak;
        double* const corr0 = p.corr;
        const int64_t total = p.nblk;
        p.P = P; p.ta = w.ta.as<double>(); p.tv = w.tv.as<double>(); p.sa = w.sa.as<double2>(); p.sv = w.sv.as<const double2>();
        const int mulgrid = ncus() * 8;
        for (int64_t c0 = 0; c0 < total; c0 += per) {
            const int64_t cnt = std::min(per, total - c0);
            p.nblk = cnt;
            p.a = a0 + (size_t)(c0 * p.delta) * es; p.v = v0 + (size_t)(c0 * p.delta) * es;
            p.lag = lag0 + c0; p.peak = peak0 + c0; p.corr = corr0 ? corr0 + c0 * p.nlag : nullptr;
            switch (x_dtype) {
                case PVX_F32: hipLaunchKernelGGL(k_xcorr_prep<float>, dim3((unsigned)cnt, 2), dim3(XC_THREADS), 0, s, p); break;
                case PVX_F64: hipLaunchKernelGGL(k_xcorr_prep<double>, dim3((unsigned)cnt, 2), dim3(XC_THREADS), 0, s, p); break;
                default: hipLaunchKernelGGL(k_xcorr_prep<int16_t>, dim3((unsigned)cnt, 2), dim3(XC_THREADS), 0, s, p); break;
            }
            PVX_HIP_CHECK(hipGetLastError());
            // the whole batch each time: the rows beyond `cnt` hold what an earlier pass left and are not read afterwards
            PVX_FFT_CHECK(xp->fwd.execute(w.ta.get(), w.sa.get(), s));
            PVX_FFT_CHECK(xp->fwd.execute(w.tv.get(), w.sv.get(), s));
            const int64_t nbin = cnt * nh;
            hipLaunchKernelGGL(k_xcorr_mul, dim3((unsigned)std::min<int64_t>(mulgrid, (nbin + XC_THREADS - 1) / XC_THREADS)), dim3(XC_THREADS), 0, s,
                               p.sa, p.sv, nbin);
            PVX_HIP_CHECK(hipGetLastError());
            PVX_FFT_CHECK(xp->inv.execute(w.sa.get(), w.ta.get(), s));
            hipLaunchKernelGGL(k_xcorr_peak, dim3((unsigned)cnt), dim3(XC_THREADS), 0, s, p);
            PVX_HIP_CHECK(hipGetLastError());
        }
        *kernels = "k_xcorr_prep+rocfft+k_xcorr_mul+rocfft+k_xcorr_peak";
    }
    PVX_HIP_CHECK(hipStreamSynchronize(s));
    return PVX_OK;
}

}  // namespace

bool pvx_xcorr_fft_route(int la, int lv) {
    return std::max(la, lv) > PVX_XCORR_DIRECT_MAX || getenv("PVX_XCORR_FFT") != nullptr;
}

int pvx_xcorr_padded(int la, int lv) {
    const int64_t nlag = (int64_t)la + lv - 1;
    int64_t P = XC_MIN_P;
    while (P < nlag) P <<= 1;
    return P > (int64_t)PVX_XCORR_MAX_P ? 0 : (int)P;
}

int pvx_xcorr_run(const void* d_a, const void* d_v, int x_dtype, int la, int lv, int64_t delta, int64_t nblk, int detrend, const double* h_win_a,
                  const double* h_win_v, int use_abs, int32_t* d_lag, double* d_peak, double* d_corr, hipStream_t s, const char** kernels) {
    if (nblk <= 0) return PVX_OK;
    XcParams p = {};
    p.a = d_a; p.v = d_v; p.delta = delta; p.nblk = nblk; p.la = la; p.lv = lv; p.nlag = la + lv - 1;
    p.detrend = detrend; p.use_abs = use_abs ? 1 : 0; p.lag = d_lag; p.peak = d_peak; p.corr = d_corr;
    XcorrWs* w;
    int rc;
    if ((rc = workspace(&w)) != PVX_OK) return rc;
    std::lock_guard<std::mutex> lk(w->mu);
    return run_locked(*w, p, x_dtype, h_win_a, h_win_v, s, kernels);
}

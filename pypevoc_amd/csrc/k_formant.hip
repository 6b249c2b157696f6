// k_formant.hip -- formant tracking (pypevoc/speech/SpeechAnalysis.py: Formants :220-319, lpc2form :186-209; glottal.py:
// lpcc2pole :249-272) on the device functions of pvx_lpc.h and pvx_roots.h.  Design: FORMANTS.md.
//
// k_preemph_decim: one thread per sample of the decimated signal, float64.  d[i] = x[i] - x[i+1] (the last sample as it
//   is; pre == 0: d = x), samples widened on load; y[m] = sum_k h[L-1-k] dz[m down + k - half], dz the zero extension of d,
//   the taps k in ascending order with fma; down == 1: y[m] = d[m].  A sample's bits depend on m and the signal alone.
// k_formant_frames: one 256-thread workgroup per frame (persistent: fr, fr + grid, ...): the frame of the decimated signal
//   times the window in LDS, pvx_lpc.h's autocorrelation and Levinson recursion, pvx_roots.h on wave 0 over [1, a_1 .. a_p],
//   then per kept root (imag >= 0, ascending angle) freq = atan2(im, re) Fs / 2 pi and bw = -0.5 (Fs / 2 pi) log |z|.
//   Rows per frame: nkept, freq / bw [order] (NaN beyond nkept), re / im [order], the LPC row [order + 1]; each nullable.
// k_polyroots: one wave per polynomial, four per workgroup, rows [n][order + 1]: the same device function on the row divided
//   by its leading coefficient (the roots' bits do not depend on a power-of-two scale of the row).
#include <math.h>

#include <map>
#include <mutex>
#include <vector>

#include "pvx_internal.h"
#include "pvx_lpc.h"
#include "pvx_mem.h"
#include "pvx_roots.h"

namespace {

using pvxlpc::kThreads;
using pvxlpc::Work;

constexpr int kFrameSingular = 1;                                    // beside pvxroots::kNoConv, kLeadZero

struct DecimParams {
    const void* x;              // x[i - x0] is sample i of the signal
    int64_t x0, n;              // n: the length of the whole signal
    int pre, down, ntaps;
    const double* h;            // [ntaps], ntaps = 2 half + 1 (unused at down 1)
    int64_t m0, cnt;            // decimated samples m0 .. m0 + cnt - 1 go to y[0 .. cnt)
    double* y;
};

template <typename T>
__global__ __launch_bounds__(kThreads) void k_preemph_decim(DecimParams p) {
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= p.cnt) return;
    const T* x = (const T*)p.x;
    auto d = [&](int64_t i) -> double {
        const double a = (double)x[i - p.x0];
        return p.pre && i + 1 < p.n ? a - (double)x[i + 1 - p.x0] : a;
    };
    const int64_t m = p.m0 + q;
    if (p.down == 1) { p.y[q] = d(m); return; }
    const int L = p.ntaps;
    const int64_t base = m * p.down - (L - 1) / 2;
    double s = 0.0;
    for (int k = 0; k < L; k++) {
        const int64_t i = base + k;
        if (i >= 0 && i < p.n) s = fma(p.h[L - 1 - k], d(i), s);
    }
    p.y[q] = s;
}

struct FormantParams {
    const double* y;            // the decimated signal; frame fr starts at y[fr * hop]
    int64_t nfr;
    int nwind, hop, order;
    double fs;
    const double* wind;         // [nwind]
    int* nkept;                 // [nfr]
    double *freq, *bw, *re, *im;   // [nfr][order]
    double* lpc;                // [nfr][order + 1]
    int* status;                // [nfr] 0, kFrameSingular, kNoConv
};

__global__ __launch_bounds__(kThreads) void k_formant_frames(FormantParams p) {
    extern __shared__ double lds[];
    __shared__ Work w;
    __shared__ double sre[PVX_ROOTS_MAX_ORDER], sim[PVX_ROOTS_MAX_ORDER];
    const int n = p.nwind, P = p.order;
    const double scale = p.fs / (2.0 * M_PI);
    for (int64_t fr = blockIdx.x; fr < p.nfr; fr += gridDim.x) {
        __syncthreads();                                             // the frame before is done with LDS
        const double* ys = p.y + fr * (int64_t)p.hop;
        for (int i = threadIdx.x; i < n; i += kThreads) lds[i] = ys[i] * p.wind[i];
        __syncthreads();
        pvxlpc::lpc_autocorr(lds, n, P, w);
        if (pvxlpc::lpc_levinson(w, P) != 0) {                       // (block-uniform)
            if (threadIdx.x == 0) p.status[fr] = kFrameSingular;
            continue;
        }
        if (p.lpc)
            for (int k = threadIdx.x; k <= P; k += kThreads) p.lpc[fr * (P + 1) + k] = w.a[k];
        if (threadIdx.x < 64) {                                      // w.a[0] = 1: the leading coefficient is never 0
            int nk = 0;
            const int st = pvxroots::wave_roots(w.a, P, sre, sim, &nk);
            const int k = threadIdx.x;
            if (k == 0) { p.status[fr] = st; if (p.nkept) p.nkept[fr] = nk; }
            if (k < P) {
                const double re = sre[k], im = sim[k];
                if (p.re) p.re[fr * P + k] = re;
                if (p.im) p.im[fr * P + k] = im;
                if (p.freq) p.freq[fr * P + k] = k < nk ? atan2(im, re) * scale : NAN;
                if (p.bw) p.bw[fr * P + k] = k < nk ? (-0.5 * scale) * log(hypot(re, im)) : NAN;
            }
        }
    }
}

struct RootsParams {
    const double* coef;         // [n][order + 1]
    int64_t n;
    int order;
    double *re, *im;            // [n][order]
    int* nkept;                 // [n]
    int* status;                // [n] 0, kNoConv, kLeadZero
};

constexpr int kWaves = kThreads / 64;

__global__ __launch_bounds__(kThreads) void k_polyroots(RootsParams p) {
    __shared__ double c[kWaves][PVX_ROOTS_MAX_ORDER + 1], sre[kWaves][PVX_ROOTS_MAX_ORDER], sim[kWaves][PVX_ROOTS_MAX_ORDER];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, P = p.order;
    const int64_t row = (int64_t)blockIdx.x * kWaves + wave;
    if (row >= p.n) return;                                          // (a whole wave: nothing below synchronises the workgroup)
    const double* cr = p.coef + row * (P + 1);
    // the monic polynomial is iterated: |p'|^2 and the stop test then do not depend on the row's scale (c / 1.0 is c itself,
    // a power of two changes no significand)
    const double lead = cr[0];
    c[wave][lane] = lane <= P ? cr[lane] / lead : 0.0;
    if (lane == 0 && P == 64) c[wave][64] = cr[64] / lead;
    pvxroots::lds_sync();
    int nk = 0, st = pvxroots::kLeadZero;
    if (lead != 0.0) st = pvxroots::wave_roots(c[wave], P, sre[wave], sim[wave], &nk);         // (wave-uniform)
    if (lane == 0) { p.status[row] = st; if (p.nkept) p.nkept[row] = nk; }
    if (lane < P) {
        const bool ok = st != pvxroots::kLeadZero;
        if (p.re) p.re[row * P + lane] = ok ? sre[wave][lane] : NAN;
        if (p.im) p.im[row * P + lane] = ok ? sim[wave][lane] : NAN;
    }
}

// Per-device tables of the calls, kept for the process (grow-only); a call holds the mutex until its stream is synchronised.
struct FormantWs {
    std::mutex mu;
    DevMem tab, status;
    std::vector<double> h_tab;
    std::vector<int> h_status;
};
std::mutex g_ws_mu;
std::map<int, FormantWs*> g_ws;                                      // device -> workspace (never erased)

int workspace(FormantWs** out) {
    int dev = 0;
    PVX_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_ws_mu);
    FormantWs*& e = g_ws[dev];
    if (!e) e = new FormantWs();
    *out = e;
    return PVX_OK;
}

unsigned frames_grid(const void* fn, size_t lds, int64_t nf) {
    int dev = 0, ncu = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ncu = v;
    }
    int per_cu = (int)((160 * 1024) / (lds + 8192));
    if (per_cu < 1) per_cu = 1;
    if (per_cu > 4) per_cu = 4;
    { const int nb = pvx_resident_blocks(fn, kThreads, lds); if (nb >= 1 && nb < per_cu) per_cu = nb; }
    const int64_t g = (int64_t)ncu * per_cu;
    return (unsigned)(nf < g ? nf : g);
}

// the first row of each status, or -1.  Synchronises the stream: the workspace is free for the next call from here on.
int first_status(FormantWs& w, int64_t nf, int64_t* singular, int64_t* noconv, int64_t* leadzero, hipStream_t s) {
    w.h_status.resize((size_t)nf);
    PVX_HIP_CHECK(hipMemcpyAsync(w.h_status.data(), w.status.get(), (size_t)nf * 4, hipMemcpyDeviceToHost, s));
    PVX_HIP_CHECK(hipStreamSynchronize(s));
    *singular = *noconv = *leadzero = -1;
    for (int64_t i = nf - 1; i >= 0; i--) {
        const int st = w.h_status[(size_t)i];
        if (st == kFrameSingular) *singular = i;
        if (st == pvxroots::kNoConv) *noconv = i;
        if (st == pvxroots::kLeadZero) *leadzero = i;
    }
    return PVX_OK;
}

}  // namespace

int pvx_formants_run(const FormantCall& c, const void* d_x, int64_t x0, int64_t f0, int64_t nf, double* d_y, const FormantRows& out,
                     int64_t* singular, int64_t* noconv, hipStream_t s, const char** kernels) {
    *singular = *noconv = -1;
    if (nf <= 0) return PVX_OK;
    FormantWs* wp;
    int rc;
    if ((rc = workspace(&wp)) != PVX_OK) return rc;
    FormantWs& w = *wp;
    std::lock_guard<std::mutex> lk(w.mu);
    std::vector<double>& t = w.h_tab;
    t.assign(c.h_wind, c.h_wind + c.nwind);
    if (c.down > 1) t.insert(t.end(), c.h_taps, c.h_taps + c.ntaps);
    if ((rc = w.tab.grow(t.size() * 8, Sizing::exact)) != PVX_OK || (rc = w.status.grow((size_t)nf * 4, Sizing::headroom)) != PVX_OK) return rc;
    PVX_HIP_CHECK(hipMemcpyAsync(w.tab.get(), t.data(), t.size() * 8, hipMemcpyHostToDevice, s));
    DecimParams d = {};
    d.x = d_x; d.x0 = x0; d.n = c.n; d.pre = c.preemph; d.down = c.down; d.ntaps = c.ntaps;
    d.h = w.tab.as<const double>() + c.nwind;
    d.m0 = f0 * c.hop; d.cnt = (nf - 1) * c.hop + c.nwind; d.y = d_y;
    const void* dfn = c.x_dtype == PVX_F32 ? (const void*)k_preemph_decim<float>
                                           : (c.x_dtype == PVX_F64 ? (const void*)k_preemph_decim<double>
                                                                   : (c.x_dtype == PVX_I16 ? (const void*)k_preemph_decim<int16_t> : nullptr));
    if (!dfn) { pvx_set_error("bad x_dtype %d", c.x_dtype); return PVX_ERR_INVALID; }
    void* dargs[] = {&d};
    PVX_HIP_CHECK(hipLaunchKernel(dfn, dim3((unsigned)((d.cnt + kThreads - 1) / kThreads)), dim3(kThreads), dargs, 0, s));
    FormantParams p = {};
    p.y = d_y; p.nfr = nf; p.nwind = c.nwind; p.hop = c.hop; p.order = c.order; p.fs = c.fs;
    p.wind = w.tab.as<const double>();
    p.nkept = out.nkept; p.freq = out.freq; p.bw = out.bw; p.re = out.re; p.im = out.im; p.lpc = out.lpc;
    p.status = w.status.as<int>();
    const size_t lds = (size_t)c.nwind * 8;
    const void* fn = (const void*)k_formant_frames;
    if (lds > 48 * 1024) PVX_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    void* args[] = {&p};
    PVX_HIP_CHECK(hipLaunchKernel(fn, dim3(frames_grid(fn, lds, nf)), dim3(kThreads), args, lds, s));
    *kernels = "k_preemph_decim+k_formant_frames";
    int64_t lead;
    return first_status(w, nf, singular, noconv, &lead, s);
}

int pvx_polyroots_run(const double* d_coef, int64_t n, int order, double* d_re, double* d_im, int* d_nkept, int* d_status, int64_t* noconv,
                      int64_t* leadzero, hipStream_t s, const char** kernels) {
    *noconv = *leadzero = -1;
    if (n <= 0) return PVX_OK;
    FormantWs* wp;
    int rc;
    if ((rc = workspace(&wp)) != PVX_OK) return rc;
    FormantWs& w = *wp;
    std::lock_guard<std::mutex> lk(w.mu);
    if ((rc = w.status.grow((size_t)n * 4, Sizing::headroom)) != PVX_OK) return rc;
    RootsParams p = {};
    p.coef = d_coef; p.n = n; p.order = order; p.re = d_re; p.im = d_im; p.nkept = d_nkept; p.status = w.status.as<int>();
    hipLaunchKernelGGL(k_polyroots, dim3((unsigned)((n + kWaves - 1) / kWaves)), dim3(kThreads), 0, s, p);
    PVX_HIP_CHECK(hipGetLastError());
    *kernels = "k_polyroots";
    if (d_status) PVX_HIP_CHECK(hipMemcpyAsync(d_status, w.status.get(), (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    int64_t sing;
    return first_status(w, n, &sing, noconv, leadzero, s);
}

// k_iaif.hip -- glottal inverse filtering (pypevoc/speech/glottal.py: InverseFilter.apply :190-234, iaif_ola :36-84)
// and frame-wise linear prediction (SpeechAnalysis.py:9-24) on the device functions of pvx_lpc.h.  Design: GLOTTAL.md.
//
// k_iaif_frames: one 256-thread workgroup per frame (persistent: a workgroup walks frames fr, fr + grid, ...), float64:
//   1. the frame, widened, goes to LDS; y[i] = sum_k b[k] xz[i + hp - k] (the high-pass FIR with its delay removed; xz
//      the frame followed by zeros), one output per thread per pass, the taps in index order;
//   2. u = [linspace(-y[0], y[0], P), y], P = tract_order + 1: what every later FIR filters;
//   3. Hg = lpc(y * hw, 1), y = fir(Hg, u)[P:]; n_it rounds of Hvt = lpc(y * hw, pt), g = integ(fir(Hvt, u))[P:],
//      Hg = lpc(g * hw, pg), y = integ(fir(Hg, u))[P:]; then Hvt = lpc(y * hw, pt), dg = fir(Hvt, u)[P:],
//      g = integ(fir(Hvt, u))[P:];
//   4. g and dg go to the workspace rows of the frame, Hvt, Hg and a status to their per-frame outputs.
// LDS (doubles): b [L] | the frame, later the windowed vector [n] | u [P + n] | work [P + n] | leak powers, block ends
// and carries of the integrator.  integ (v[j] += leak v[j-1] over the padded length) is a blocked scan with one shape
// per length: thread t owns the B = ceil(len / 256) samples from t B on, runs them from a zero carry, thread 0 chains the
// 256 block ends, and every thread adds leak^(j - t B + 1) times its block's carry.
// k_lpc_frames: the windowed frame in LDS, pvx_lpc.h, one row of coefficients.
// k_iaif_ola: one thread per output sample adds g * wind, dg * wind and wind of the frames that cover it in ascending
// frame order (no atomics: the reference's accumulation order), and divides where the window sum is > 0.
#include <math.h>

#include <map>
#include <mutex>
#include <vector>

#include "pvx_internal.h"
#include "pvx_lpc.h"
#include "pvx_mem.h"

namespace {

using pvxlpc::kThreads;
using pvxlpc::Work;

constexpr int kMaxPad = PVX_LPC_MAX_ORDER + 1;
constexpr int kMaxBlock = (PVX_IAIF_MAX_NWIND + kMaxPad + kThreads - 1) / kThreads;   // integrator samples per thread

struct IaifParams {
    const void* x;              // samples; frame fr starts at x[fr * hop]
    int64_t nfr;
    int nwind, hop, ntaps, hp, pt, pg, n_it;
    double leak;
    const double* b;            // [ntaps]
    const double* hw;           // [nwind] the window of the LPCs
    double *g, *dg;             // [nfr][nwind]
    double* vt;                 // [nfr][pt + 1]
    double* gc;                 // [nfr][(n_it ? pg : 1) + 1]
    int* status;                // [nfr] 0, or 1 + the number of the LPC that was singular
};

// out[j] = sum_k h[k] u[j - k] (zeros before u), j in [j0, m)
__device__ void fir(const double* h, int p, const double* u, int j0, int m, double* out) {
    for (int j = j0 + (int)threadIdx.x; j < m; j += kThreads) {
        const int ke = j < p ? j : p;
        double s = 0.0;
        for (int k = 0; k <= ke; k++) s = fma(h[k], u[j - k], s);
        out[j] = s;
    }
}

// v[j] += leak * v[j-1], j in [0, m), as a blocked scan (see above); pw[q] = leak^q.  Ends with a barrier.
__device__ void integ(double* v, int m, double leak, const double* pw, double* ends, double* carry) {
    const int B = (m + kThreads - 1) / kThreads;
    const int s = (int)threadIdx.x * B, e = s + B < m ? s + B : m;
    double prev = 0.0;
    for (int j = s; j < e; j++) { prev = v[j] + leak * prev; v[j] = prev; }
    ends[threadIdx.x] = prev;
    __syncthreads();
    if (threadIdx.x == 0) {
        double c = 0.0;
        for (int q = 0; q < kThreads; q++) {
            carry[q] = c;
            const int len = m - q * B < B ? m - q * B : B;
            if (len > 0) c = ends[q] + pw[len] * c;
        }
    }
    __syncthreads();
    if (threadIdx.x > 0) {
        const double c = carry[threadIdx.x];
        for (int j = s; j < e; j++) v[j] = v[j] + pw[j - s + 1] * c;
    }
    __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_iaif_frames(IaifParams p) {
    extern __shared__ double lds[];
    __shared__ Work w;
    __shared__ double pw[kMaxBlock + 1], ends[kThreads], carry[kThreads];
    const int n = p.nwind, L = p.ntaps, hp = p.hp, P = p.pt + 1, M = P + n;
    const int pgc = p.n_it > 0 ? p.pg : 1;
    double* b = lds;
    double* fv = b + L;
    double* u = fv + n;
    double* wk = u + M;
    for (int k = threadIdx.x; k < L; k += kThreads) b[k] = p.b[k];
    if (threadIdx.x == 0) {
        double q = 1.0;
        for (int k = 0; k <= kMaxBlock; k++) { pw[k] = q; q = q * p.leak; }
    }
    // lpc(wk[P:] * hw, order); false: singular, the frame's status is written
    auto window_lpc = [&](int order, int which, int64_t fr) -> bool {
        for (int i = threadIdx.x; i < n; i += kThreads) fv[i] = wk[P + i] * p.hw[i];
        __syncthreads();
        pvxlpc::lpc_autocorr(fv, n, order, w);
        if (pvxlpc::lpc_levinson(w, order) != 0) {
            if (threadIdx.x == 0) p.status[fr] = which;
            return false;
        }
        return true;
    };
    auto put = [&](double* rows, int order, int64_t fr) {
        for (int k = threadIdx.x; k <= order; k += kThreads) rows[fr * (order + 1) + k] = w.a[k];
    };
    for (int64_t fr = blockIdx.x; fr < p.nfr; fr += gridDim.x) {
        __syncthreads();                                             // the frame before is done with LDS (and b, pw are written)
        const T* xs = (const T*)p.x + fr * (int64_t)p.hop;
        for (int i = threadIdx.x; i < n; i += kThreads) fv[i] = (double)xs[i];
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const int top = i + hp;                                  // xz index of tap 0
            const int klo = top > n - 1 ? top - (n - 1) : 0, khi = top < L - 1 ? top : L - 1;
            double s = 0.0;
            for (int k = klo; k <= khi; k++) s = fma(b[k], fv[top - k], s);
            wk[P + i] = s;
            u[P + i] = s;
        }
        __syncthreads();
        if ((int)threadIdx.x < P) {                                  // np.linspace(-y0, y0, P)
            const double y0 = u[P], start = -y0;
            double v = start;
            if (P > 1) {
                const double step = (y0 - start) / (double)(P - 1);
                v = (int)threadIdx.x == P - 1 ? y0 : (double)threadIdx.x * step + start;
            }
            u[threadIdx.x] = v;
        }
        if (threadIdx.x == 0) p.status[fr] = 0;
        int nl = 1;                                                  // the number of the LPC at hand
        if (!window_lpc(1, nl++, fr)) continue;                      // (block-uniform)
        if (p.n_it == 0) put(p.gc, 1, fr);
        fir(w.a, 1, u, P, M, wk);
        __syncthreads();
        bool ok = true;
        for (int it = 0; it < p.n_it && ok; it++) {
            if (!(ok = window_lpc(p.pt, nl++, fr))) break;
            fir(w.a, p.pt, u, 0, M, wk);
            __syncthreads();
            integ(wk, M, p.leak, pw, ends, carry);
            if (!(ok = window_lpc(p.pg, nl++, fr))) break;
            put(p.gc, pgc, fr);
            fir(w.a, p.pg, u, 0, M, wk);
            __syncthreads();
            integ(wk, M, p.leak, pw, ends, carry);
        }
        if (!ok) continue;
        if (!window_lpc(p.pt, nl++, fr)) continue;
        put(p.vt, p.pt, fr);
        fir(w.a, p.pt, u, 0, M, wk);
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += kThreads) p.dg[fr * (int64_t)n + i] = wk[P + i];
        __syncthreads();
        integ(wk, M, p.leak, pw, ends, carry);
        for (int i = threadIdx.x; i < n; i += kThreads) p.g[fr * (int64_t)n + i] = wk[P + i];
    }
}

struct LpcParams {
    const void* x;
    int64_t nfr;
    int nwind, hop, order;
    const double* wind;         // [nwind] or null
    double* coef;               // [nfr][order + 1]
    int* status;                // [nfr]
};

template <typename T>
__global__ __launch_bounds__(kThreads) void k_lpc_frames(LpcParams p) {
    extern __shared__ double lds[];
    __shared__ Work w;
    const int n = p.nwind;
    for (int64_t fr = blockIdx.x; fr < p.nfr; fr += gridDim.x) {
        __syncthreads();
        const T* xs = (const T*)p.x + fr * (int64_t)p.hop;
        for (int i = threadIdx.x; i < n; i += kThreads) lds[i] = p.wind ? (double)xs[i] * p.wind[i] : (double)xs[i];
        __syncthreads();
        pvxlpc::lpc_autocorr(lds, n, p.order, w);
        const int st = pvxlpc::lpc_levinson(w, p.order);
        if (threadIdx.x == 0) p.status[fr] = st != 0 ? 1 : 0;
        if (st == 0)
            for (int k = threadIdx.x; k <= p.order; k += kThreads) p.coef[fr * (p.order + 1) + k] = w.a[k];
    }
}

// Workspace rows 0 .. nf - 1 hold frames f0 .. f0 + nf - 1 of the signal; thread per sample s0 .. s0 + ns - 1, written to
// glot[0 .. ns) / dglot[0 .. ns).
__global__ __launch_bounds__(kThreads) void k_iaif_ola(const double* g, const double* dg, const double* wind, int nwind, int hop, int64_t f0,
                                                       int64_t nf, int64_t s0, int64_t ns, double* glot, double* dglot) {
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= ns) return;
    const int64_t s = s0 + q;
    const int64_t lo = s - nwind + 1;
    int64_t fa = lo <= 0 ? 0 : (lo + hop - 1) / hop, fb = s / hop;
    if (fa < f0) fa = f0;                                            // (the caller's rows cover every frame of its samples)
    if (fb > f0 + nf - 1) fb = f0 + nf - 1;
    double a = 0.0, d = 0.0, ws = 0.0;
    for (int64_t f = fa; f <= fb; f++) {
        const int64_t j = s - f * hop;                               // 0 <= j < nwind
        const double wv = wind[j];
        const int64_t at = (f - f0) * nwind + j;
        a = a + g[at] * wv;
        d = d + dg[at] * wv;
        ws = ws + wv;
    }
    if (ws > 0.0) { a = a / ws; d = d / ws; }
    if (glot) glot[q] = a;
    if (dglot) dglot[q] = d;
}

// Per-device tables of the calls, kept for the process (grow-only); a call holds the mutex until its stream is synchronised.
struct IaifWs {
    std::mutex mu;
    DevMem tab, status;
    std::vector<double> h_tab;
};
std::mutex g_ws_mu;
std::map<int, IaifWs*> g_ws;                                         // device -> workspace (never erased)

int workspace(IaifWs** out) {
    int dev = 0;
    PVX_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_ws_mu);
    IaifWs*& e = g_ws[dev];
    if (!e) e = new IaifWs();
    *out = e;
    return PVX_OK;
}

unsigned frames_grid(const void* fn, size_t lds, int64_t nf) {
    int dev = 0, ncu = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ncu = v;
    }
    int per_cu = (int)((160 * 1024) / (lds + 4096));
    if (per_cu < 1) per_cu = 1;
    if (per_cu > 4) per_cu = 4;
    { const int nb = pvx_resident_blocks(fn, kThreads, lds); if (nb >= 1 && nb < per_cu) per_cu = nb; }
    const int64_t g = (int64_t)ncu * per_cu;
    return (unsigned)(nf < g ? nf : g);
}

template <typename P> const void* pick(int x_dtype, void (*f32)(P), void (*f64)(P), void (*i16)(P)) {
    return x_dtype == PVX_F32 ? (const void*)f32 : (x_dtype == PVX_F64 ? (const void*)f64 : (x_dtype == PVX_I16 ? (const void*)i16 : nullptr));
}

// the first frame with a status, or -1
int first_singular(IaifWs& w, int64_t nf, int64_t* which, hipStream_t s) {
    std::vector<int> h((size_t)nf);
    PVX_HIP_CHECK(hipMemcpyAsync(h.data(), w.status.get(), (size_t)nf * 4, hipMemcpyDeviceToHost, s));
    PVX_HIP_CHECK(hipStreamSynchronize(s));                          // the workspace is free for the next call from here on
    *which = -1;
    for (int64_t i = 0; i < nf; i++) if (h[(size_t)i] != 0) { *which = i; break; }
    return PVX_OK;
}

// dynamic LDS of k_iaif_frames: b | frame | u | work
size_t iaif_lds_bytes(int nwind, int ntaps, int tract_order) {
    return ((size_t)ntaps + (size_t)nwind + 2 * ((size_t)nwind + (size_t)tract_order + 1)) * 8;
}

}  // namespace

int pvx_iaif_run(const IaifCall& c, const void* d_x, int64_t f0, int64_t nf, double* d_g, double* d_dg, double* d_vt, double* d_gc, int64_t s0,
                 int64_t ns, double* d_glot, double* d_dglot, int64_t* singular, hipStream_t s, const char** kernels) {
    *singular = -1;
    if (nf <= 0) return PVX_OK;
    IaifWs* wp;
    int rc;
    if ((rc = workspace(&wp)) != PVX_OK) return rc;
    IaifWs& w = *wp;
    std::lock_guard<std::mutex> lk(w.mu);
    const bool ola = (d_glot || d_dglot) && ns > 0;
    std::vector<double>& t = w.h_tab;
    t.assign(c.h_b, c.h_b + c.ntaps);
    t.insert(t.end(), c.h_hw, c.h_hw + c.nwind);
    if (ola) t.insert(t.end(), c.h_ow, c.h_ow + c.nwind);
    if ((rc = w.tab.grow(t.size() * 8, Sizing::exact)) != PVX_OK || (rc = w.status.grow((size_t)nf * 4, Sizing::headroom)) != PVX_OK) return rc;
    PVX_HIP_CHECK(hipMemcpyAsync(w.tab.get(), t.data(), t.size() * 8, hipMemcpyHostToDevice, s));
    IaifParams p = {};
    p.x = d_x; p.nfr = nf; p.nwind = c.nwind; p.hop = c.hop; p.ntaps = c.ntaps; p.pt = c.pt; p.pg = c.pg; p.n_it = c.n_it; p.leak = c.leak;
    p.hp = (int)nearbyint((double)c.ntaps / 2.0 - 1.0);              // int(np.round(L/2 - 1)): half to even
    if (p.hp < 0) p.hp = 0;
    p.b = w.tab.as<const double>(); p.hw = p.b + c.ntaps;
    p.g = d_g; p.dg = d_dg; p.vt = d_vt; p.gc = d_gc; p.status = w.status.as<int>();
    const size_t lds = iaif_lds_bytes(c.nwind, c.ntaps, c.pt);
    const void* fn = pick<IaifParams>(c.x_dtype, k_iaif_frames<float>, k_iaif_frames<double>, k_iaif_frames<int16_t>);
    if (!fn) { pvx_set_error("bad x_dtype %d", c.x_dtype); return PVX_ERR_INVALID; }
    if (lds > 64 * 1024) PVX_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    void* args[] = {&p};
    PVX_HIP_CHECK(hipLaunchKernel(fn, dim3(frames_grid(fn, lds, nf)), dim3(kThreads), args, lds, s));
    *kernels = "k_iaif_frames";
    if (ola) {
        hipLaunchKernelGGL(k_iaif_ola, dim3((unsigned)((ns + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, d_g, d_dg, p.hw + c.nwind, c.nwind,
                           c.hop, f0, nf, s0, ns, d_glot, d_dglot);
        PVX_HIP_CHECK(hipGetLastError());
        *kernels = "k_iaif_frames+k_iaif_ola";
    }
    return first_singular(w, nf, singular, s);
}

int pvx_lpc_run(const void* d_x, int x_dtype, int64_t nf, const double* h_wind, int nwind, int hop, int order, double* d_coef, int64_t* singular,
                hipStream_t s, const char** kernels) {
    *singular = -1;
    if (nf <= 0) return PVX_OK;
    IaifWs* wp;
    int rc;
    if ((rc = workspace(&wp)) != PVX_OK) return rc;
    IaifWs& w = *wp;
    std::lock_guard<std::mutex> lk(w.mu);
    if ((rc = w.tab.grow((size_t)nwind * 8, Sizing::exact)) != PVX_OK || (rc = w.status.grow((size_t)nf * 4, Sizing::headroom)) != PVX_OK) return rc;
    if (h_wind) PVX_HIP_CHECK(hipMemcpyAsync(w.tab.get(), h_wind, (size_t)nwind * 8, hipMemcpyHostToDevice, s));
    LpcParams p = {};
    p.x = d_x; p.nfr = nf; p.nwind = nwind; p.hop = hop; p.order = order;
    p.wind = h_wind ? w.tab.as<const double>() : nullptr;
    p.coef = d_coef; p.status = w.status.as<int>();
    const size_t lds = (size_t)nwind * 8;
    const void* fn = pick<LpcParams>(x_dtype, k_lpc_frames<float>, k_lpc_frames<double>, k_lpc_frames<int16_t>);
    if (!fn) { pvx_set_error("bad x_dtype %d", x_dtype); return PVX_ERR_INVALID; }
    if (lds > 64 * 1024) PVX_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    void* args[] = {&p};
    PVX_HIP_CHECK(hipLaunchKernel(fn, dim3(frames_grid(fn, lds, nf)), dim3(kThreads), args, lds, s));
    *kernels = "k_lpc_frames";
    return first_singular(w, nf, singular, s);
}

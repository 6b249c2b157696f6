// k_lpcenv.hip -- the LPC spectral envelope and its refined peaks (pypevoc/speech/SpeechAnalysis.py: lpc2form_full :211-218)
// and PeakFinder's refine_all on plain rows (pypevoc/PeakFinder.py:331-413), on the device functions of pvx_peakref.h.
// Design: ENVELOPE.md.
//
// k_lpc_envelope: one wave per coefficient row c[0 .. p], four per workgroup.  Point k < npts: z_k = exp(-i pi k / npts) from
//   sincospi(k / npts), A_k = sum_j c_j z_k^j by Horner from c_p down in fma complex arithmetic, y_k = 1 / |A_k|: what
//   abs(freqz([1], c, worN=npts)[1]) computes.  A point's value depends on (row, k) alone -- no running rotation --, so the
//   lanes that need a neighbour's point evaluate it themselves and get the neighbour's bits.  Then pvx_peakref.h's scan,
//   count, pack and refinement on the axis x_k = k fs / (2 npts).  Nothing keeps a row in LDS: a wave holds its coefficients
//   and one mask bit per point there.  A root on the unit circle at a grid point gives inf, as in scipy: not handled.
// k_peaks_refine: the same scan and refinement on rows y[n][npts] in memory with the axis x[npts] (null: arange); with sel
//   [n][maxpk] (-1 padded) the scan is skipped and those indices are refined, refine's own test s1 > s0 and s1 >= s2 choosing
//   between the fit and its else branch.
#include <math.h>

#include <map>
#include <mutex>
#include <vector>

#include "pvx_internal.h"
#include "pvx_mem.h"
#include "pvx_peakref.h"

namespace {

using namespace pvxpk;

constexpr int kThreads = 256, kWaves = kThreads / 64;

struct EnvParams {
    const double* coef;         // [n][order + 1]
    int64_t n;
    int order, npts, maxpk;
    double fs;
    double* env;                // [n][npts]
    int* npk;                   // [n]
    int* idx;                   // [n][maxpk]
    double *pos, *val;          // [n][maxpk]
    int* status;                // [n]
};

struct EnvRow {                 // y_k of one coefficient row (in LDS)
    const double* c;
    int P;
    double n;
    __device__ double operator()(int k) const {
        double s, co;
        sincospi((double)k / n, &s, &co);
        const double zr = co, zi = -s;
        double ar = c[P], ai = 0.0;
        for (int j = P - 1; j >= 0; j--) {                           // a = a z + c_j
            const double nr = fma(ar, zr, fma(-ai, zi, c[j]));
            ai = fma(ar, zi, ai * zr);
            ar = nr;
        }
        return 1.0 / hypot(ar, ai);
    }
};

struct MemRow {
    const double* y;
    __device__ double operator()(int k) const { return y[k]; }
};

__global__ __launch_bounds__(kThreads) void k_lpc_envelope(EnvParams p) {
    __shared__ double c[kWaves][PVX_ROOTS_MAX_ORDER + 1];
    __shared__ unsigned mask[kWaves][kMaskWords * 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, P = p.order;
    const int64_t row = (int64_t)blockIdx.x * kWaves + wave;
    if (row >= p.n) return;                                          // (a whole wave: nothing below synchronises the workgroup)
    const double* cr = p.coef + row * (P + 1);
    c[wave][lane] = lane <= P ? cr[lane] : 0.0;
    if (lane == 0 && P == 64) c[wave][64] = cr[64];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");               // LDS hand-off inside one wave (as pvx_roots.h: lds_sync)
    __builtin_amdgcn_wave_barrier();
    if (c[wave][0] == 0.0) {                                         // (wave-uniform)
        if (lane == 0) { p.status[row] = kRowLeadZero; if (p.npk) p.npk[row] = 0; }
        return;
    }
    const EnvRow y = {c[wave], P, (double)p.npts};
    const AxisFreq x = {p.fs, 2.0 * (double)p.npts};
    const int64_t o = row * p.maxpk;
    const int st = row_peaks(y, x, p.npts, p.env ? p.env + row * p.npts : nullptr, mask[wave], lane, p.maxpk, p.npk ? p.npk + row : nullptr,
                             p.idx ? p.idx + o : nullptr, p.pos ? p.pos + o : nullptr, p.val ? p.val + o : nullptr);
    if (lane == 0) p.status[row] = st;
}

struct RefineParams {
    const double* y;            // [n][npts]
    int64_t n;
    int npts, maxpk;
    const double* x;            // [npts] or null
    const int* sel;             // [n][maxpk] or null
    int* npk;
    int* idx;
    double *pos, *val;
    int* status;
};

template <class X>
__device__ __forceinline__ int sel_row(MemRow y, X x, int npts, const int* sel, int maxpk, int lane, int* npk, int* idx, double* pos,
                                       double* val) {
    int cnt = 0, bad = 0;
    for (int t0 = 0; t0 < maxpk; t0 += 64) {                         // (wave-uniform trip count)
        const int t = t0 + lane;
        const int i = t < maxpk ? sel[t] : -1;
        const bool given = i != -1, ok = i >= 1 && i <= npts - 2;
        bad |= given && !ok ? 1 : 0;
        cnt += given ? 1 : 0;
        if (t < maxpk) {
            double fp = NAN, fv = NAN;
            if (ok) {
                const double s0 = y(i - 1), s1 = y(i), s2 = y(i + 1);
                refine3(s0, s1, s2, i, npts, x, s1 > s0 && s1 >= s2, &fp, &fv);
            }
            if (idx) idx[t] = ok ? i : -1;
            if (pos) pos[t] = fp;
            if (val) val[t] = fv;
        }
    }
    int total;
    wave_excl(cnt, lane, &total);
    if (lane == 0 && npk) *npk = total;
    return __ballot(bad != 0) != 0ull ? kRowBadIndex : kRowOk;
}

template <class X> __device__ __forceinline__ void refine_row(const RefineParams& p, X x, unsigned* m, int lane, int64_t row) {
    const MemRow y = {p.y + row * p.npts};
    const int64_t o = row * p.maxpk;
    int* npk = p.npk ? p.npk + row : nullptr;
    int* idx = p.idx ? p.idx + o : nullptr;
    double* pos = p.pos ? p.pos + o : nullptr;
    double* val = p.val ? p.val + o : nullptr;
    const int st = p.sel ? sel_row(y, x, p.npts, p.sel + o, p.maxpk, lane, npk, idx, pos, val)
                         : row_peaks(y, x, p.npts, nullptr, m, lane, p.maxpk, npk, idx, pos, val);
    if (lane == 0) p.status[row] = st;
}

__global__ __launch_bounds__(kThreads) void k_peaks_refine(RefineParams p) {
    __shared__ unsigned mask[kWaves][kMaskWords * 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kWaves + wave;
    if (row >= p.n) return;                                          // (a whole wave)
    if (p.x) refine_row(p, AxisTable{p.x}, mask[wave], lane, row);
    else refine_row(p, AxisArange{}, mask[wave], lane, row);
}

// Per-device status rows of the calls, kept for the process (grow-only); a call holds the mutex until its stream is synchronised.
struct EnvWs {
    std::mutex mu;
    DevMem status;
    std::vector<int> h_status;
};
std::mutex g_ws_mu;
std::map<int, EnvWs*> g_ws;                                          // device -> workspace (never erased)

int workspace(EnvWs** out) {
    int dev = 0;
    PVX_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_ws_mu);
    EnvWs*& e = g_ws[dev];
    if (!e) e = new EnvWs();
    *out = e;
    return PVX_OK;
}

// the first row of each status, or -1.  Synchronises the stream.
int first_status(EnvWs& w, int64_t n, int64_t* overflow, int64_t* invalid, hipStream_t s) {
    w.h_status.resize((size_t)n);
    PVX_HIP_CHECK(hipMemcpyAsync(w.h_status.data(), w.status.get(), (size_t)n * 4, hipMemcpyDeviceToHost, s));
    PVX_HIP_CHECK(hipStreamSynchronize(s));
    *overflow = *invalid = -1;
    for (int64_t i = n - 1; i >= 0; i--) {
        const int st = w.h_status[(size_t)i];
        if (st == kRowOverflow) *overflow = i;
        if (st == kRowBadIndex || st == kRowLeadZero) *invalid = i;
    }
    return PVX_OK;
}

}  // namespace

int pvx_lpcenv_run(const double* d_coef, int64_t n, int order, int npts, double fs, int maxpk, double* d_env, int* d_npk, int* d_idx,
                   double* d_pos, double* d_val, int64_t* overflow, int64_t* invalid, hipStream_t s, const char** kernels) {
    *overflow = *invalid = -1;
    if (n <= 0) return PVX_OK;
    EnvWs* wp;
    int rc;
    if ((rc = workspace(&wp)) != PVX_OK) return rc;
    EnvWs& w = *wp;
    std::lock_guard<std::mutex> lk(w.mu);
    if ((rc = w.status.grow((size_t)n * 4, Sizing::headroom)) != PVX_OK) return rc;
    EnvParams p = {};
    p.coef = d_coef; p.n = n; p.order = order; p.npts = npts; p.maxpk = maxpk; p.fs = fs;
    p.env = d_env; p.npk = d_npk; p.idx = d_idx; p.pos = d_pos; p.val = d_val; p.status = w.status.as<int>();
    hipLaunchKernelGGL(k_lpc_envelope, dim3((unsigned)((n + kWaves - 1) / kWaves)), dim3(kThreads), 0, s, p);
    PVX_HIP_CHECK(hipGetLastError());
    *kernels = "k_lpc_envelope";
    return first_status(w, n, overflow, invalid, s);
}

int pvx_peaks_refine_run(const double* d_y, int64_t n, int npts, const double* d_x, int maxpk, const int* d_sel, int* d_npk, int* d_idx,
                         double* d_pos, double* d_val, int64_t* overflow, int64_t* invalid, hipStream_t s, const char** kernels) {
    *overflow = *invalid = -1;
    if (n <= 0) return PVX_OK;
    EnvWs* wp;
    int rc;
    if ((rc = workspace(&wp)) != PVX_OK) return rc;
    EnvWs& w = *wp;
    std::lock_guard<std::mutex> lk(w.mu);
    if ((rc = w.status.grow((size_t)n * 4, Sizing::headroom)) != PVX_OK) return rc;
    RefineParams p = {};
    p.y = d_y; p.n = n; p.npts = npts; p.maxpk = maxpk; p.x = d_x; p.sel = d_sel;
    p.npk = d_npk; p.idx = d_idx; p.pos = d_pos; p.val = d_val; p.status = w.status.as<int>();
    hipLaunchKernelGGL(k_peaks_refine, dim3((unsigned)((n + kWaves - 1) / kWaves)), dim3(kThreads), 0, s, p);
    PVX_HIP_CHECK(hipGetLastError());
    *kernels = "k_peaks_refine";
    return first_status(w, n, overflow, invalid, s);
}

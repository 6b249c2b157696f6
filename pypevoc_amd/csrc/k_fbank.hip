// k_fbank.hip -- FFT filter banks (pypevoc/FFTFilters.py): FilterBank.specout (:274-292) for every frame of a call,
//   spec[i][b] = sum_k |fft(w[i*hop : i*hop+nwind] * wind)[k]|^2 * fb[b][k]
// and, when asked, MelFilterBank.mfcc's cepstral step on log(spec) (:352-374): DCT type 1..4 (scipy.fftpack, norm=None)
// or np.fft.ifft across the bands.  float64 throughout.  Design and numbers: FILTERBANK.md.
//
// The reference's weights fb[b][0..nwind) cover the FULL spectrum of the real frame; |X[nwind-k]|^2 = |X[k]|^2, so the host folds
// them onto the half spectrum (bins 0 .. nwind/2) and packs, per band, only the bins between its first and last non-zero
// folded weight: a band costs its own bins.
//
// Two routes (fbank_route()):
//   fused  nwind 512 / 1024 / 2048: k_fbank_fused, one launch, a wave64 per frame -- load + window, the single-wave transform
//          of pvx_stft.h (as k_stft.hip runs it), |X|^2 of the untangled bins into the wave's own LDS buffer (the transform's
//          exchange buffer, free by then), band sums, log, cepstral matrix.  No spectrum row reaches global memory.
//   rows   any other nwind: k_frames (windowed frames) + a batched real rocFFT into the workspace, then k_fbank_rows, a wave
//          per half-spectrum row with the same band / cepstrum tail.
// A frame is the work of one wave with a fixed summation order: results do not depend on the grid, on the chunking of a
// long signal or on where the samples came from.
#include <math.h>

#include <map>
#include <mutex>
#include <vector>

#include "pvx_fbank_ws.h"
#include "pvx_internal.h"
#include "pvx_mem.h"
#include "pvx_stft.h"
#include "pvx_wave.h"

using namespace pvxw;
using namespace pvxf;
using namespace pvxs;

namespace {

struct FbankParams {
    const void* x;            // samples of frame 0 (fused) ...
    const void* rows;         // ... or complex double [nfr][ldo] half-spectrum rows (rows route)
    int64_t ldo;
    int64_t nfr;              // frames of this launch
    int hop, nband, cep_mode;
    const double* win;        // [nwind] the bare window (FFTFilters.py:283: no 1/wfact)
    const void* twiddle;      // complex double [nwind] W_nwind^j (fused)
    const int* band_lo;       // [nband] first half-spectrum bin of the band's packed weights
    const int* band_n;        // [nband] how many (0: the band's row of fb is all zero)
    const int* band_off;      // [nband] where they start in wf
    const double* wf;         // folded weights, band after band
    const double* cre;        // [nband][nband] cepstral matrix: cep[c] = sum_n log(spec[n]) * cre[n][c]
    const double* cim;        // the imaginary one (IFFT)
    const double* silent;     // [nband] or [nband][2]: the reference's row for a frame whose band energies are all 0
    double* spec;             // [nfr][nband] or nullptr
    double* cep;              // [nfr][nband] or [nfr][nband][2] (IFFT), or nullptr
};

// Band sums, log and cepstral step of frame `fr` by one wave.  pw(k) = |X[k]|^2 of half-spectrum bin k; le: nband doubles
// of the wave's own LDS.  Lanes stride over a band's bins, wave_sum joins them: the order is fixed.
template <typename PW>
__device__ __forceinline__ void fbank_tail(const FbankParams& p, int64_t fr, int lane, double* le, PW pw) {
    const int nband = p.nband;
    double e0 = 0.0, e1 = 0.0;                                        // energy of band `lane` / `lane + 64`
    for (int b = 0; b < nband; b++) {
        const int lo = p.band_lo[b], n = p.band_n[b];
        const double* w = p.wf + p.band_off[b];
        double acc = 0.0;
        for (int k = lane; k < n; k += 64) acc += pw(lo + k) * w[k];
        const double e = wave_sum(acc);
        if (b < 64) { if (lane == b) e0 = e; }
        else if (lane == b - 64) e1 = e;
    }
    const bool h0 = lane < nband, h1 = lane + 64 < nband;
    if (p.spec) {
        double* so = p.spec + fr * nband;
        if (h0) so[lane] = e0;
        if (h1) so[lane + 64] = e1;
    }
    if (p.cep_mode == 0) return;
    const int cpx = p.cep_mode == 5 ? 2 : 1;
    double* co = p.cep + fr * (int64_t)(nband * cpx);
    // silence: every band energy exactly 0, every log -inf.  What scipy's and numpy's FFT-based transforms make of such a
    // row is not what a matrix product makes of it; the host built the reference's row (FILTERBANK.md)
    if (__ballot((h0 && e0 != 0.0) || (h1 && e1 != 0.0)) == 0ull) {
        for (int i = lane; i < nband * cpx; i += 64) co[i] = p.silent[i];
        return;
    }
    if (h0) le[lane] = log(e0);                                       // FFTFilters.py:354: no floor, log(0) = -inf
    if (h1) le[lane + 64] = log(e1);
    wave_sync();
    for (int c = lane; c < nband; c += 64) {
        double ar = 0.0, ai = 0.0;
        const double* mr = p.cre + c;
        if (cpx == 2) {
            const double* mi = p.cim + c;
            for (int n = 0; n < nband; n++) { const double l = le[n]; ar += l * mr[n * nband]; ai += l * mi[n * nband]; }
            co[2 * c] = ar; co[2 * c + 1] = ai;
        } else {
            for (int n = 0; n < nband; n++) ar += le[n] * mr[n * nband];
            co[c] = ar;
        }
    }
    wave_sync();                                                      // le is free for the wave's next frame
}

// ---- fused route -----------------------------------------------------------------------------------------------------
// The transform is k_stft.hip's, stage for stage (same tables, same arithmetic); the untangle keeps |X[k]|^2 instead of
// storing X[k], and includes the Nyquist bin nwind/2 that the analysis rows leave out.
template <int R, typename InT>
__global__ __launch_bounds__(384) void k_fbank_fused(FbankParams p) {
    using T = double;
    using G = StftGeo<R, T>;
    constexpr int M = G::M, P = G::P, PITCH = G::PITCH;
    static_assert(M + 8 + PVX_FBANK_MAX_NBAND <= 2 * G::BUFC, "|X|^2 of bins 0..M and the log energies share the wave's exchange buffer");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nw = blockDim.x >> 6;
    T* const winL = (T*)(smem + G::OFF_WIN);
    cx<T>* const t1L = (cx<T>*)(smem + G::OFF_T1);
    cx<T>* const t2L = (cx<T>*)(smem + G::OFF_T2);
    cx<T>* const tw3 = (cx<T>*)(smem + G::OFF_TW3);
    cx<T>* const dz = (cx<T>*)(smem + G::OFF_BUF) + (size_t)wid * G::BUFC;
    double* const pwL = (double*)dz;                                  // [M + 1] |X[k]|^2 once the untangle has read dz
    double* const leL = pwL + M + 8;                                  // [nband] log band energies
    const cx<T>* const tab = (const cx<T>*)p.twiddle;
    constexpr int NMASK = G::N - 1;
    for (int i = threadIdx.x; i < G::N; i += blockDim.x) winL[i] = p.win[i];
    for (int i = threadIdx.x; i < R * 64; i += blockDim.x) t1L[i] = tab[(2 * (i & 63) * (i >> 6)) & NMASK];
    for (int i = threadIdx.x; i < 64; i += blockDim.x) t2L[i] = tab[((G::N / 64) * (i % P) * (i / P)) & NMASK];   // [t2][l1]
    for (int i = threadIdx.x; i <= G::HALF; i += blockDim.x) tw3[i] = tab[i];
    __syncthreads();
    const int Q = lane / P, L1 = lane % P;
    T csg[G::LOGP > 0 ? G::LOGP : 1];
    cx<T> cw[G::LOGP > 0 ? G::LOGP : 1];
#pragma unroll
    for (int s = 0; s < G::LOGP; s++) {
        const int h = P >> (s + 1);
        const bool up = (L1 & h) != 0;
        csg[s] = up ? (T)-1 : (T)1;
        const cx<T> wv = tab[((G::N / (2 * h)) * (L1 % h)) & NMASK];
        cw[s] = up ? wv : mkc<T>((T)1, (T)0);
    }
    int t1v = 0;
#pragma unroll
    for (int b = 0; b < G::LOGP; b++) if (L1 & (1 << b)) t1v |= 1 << (G::LOGP - 1 - b);

    // frames are dealt round-robin to the waves of the grid (neighbouring waves = neighbouring frames: their overlap is
    // served by L1 / L2); the samples of a wave's next frame are prefetched in four groups spread over the transform
    const int64_t W = (int64_t)gridDim.x * nw;
    const int64_t w = (int64_t)blockIdx.x * nw + wid;
    auto row_src = [&](int64_t j) -> const InT* { return j < p.nfr ? (const InT*)p.x + j * (int64_t)p.hop : nullptr; };
    T raw[2 * R];                                                     // samples (2l + 128 r, + 1) of the next frame
    auto prefetch_part = [&](const InT* src, int part) {
        if (src == nullptr) return;
        constexpr int PR = R / 4;
#pragma unroll
        for (int r = part * PR; r < (part + 1) * PR; r++) {
            const InT* q = src + 2 * lane + 128 * r;
            raw[2 * r] = (T)q[0]; raw[2 * r + 1] = (T)q[1];
        }
    };
    {
        const InT* s0 = row_src(w);
        prefetch_part(s0, 0); prefetch_part(s0, 1); prefetch_part(s0, 2); prefetch_part(s0, 3);
    }
    for (int64_t j = w; j < p.nfr; j += W) {
        const InT* nsrc = row_src(j + W);
        cx<T> z[R];
        lds_gather_use<0, R, lds_batch<R, T>(), T>((const cx<T>*)(winL + 2 * lane), 64, [&](int r, cx<T> wv) {
            z[r] = mkc<T>(raw[2 * r] * wv.x, raw[2 * r + 1] * wv.y);
            asm volatile("" : "+v"(z[r].x), "+v"(z[r].y));           // the multiplies stay above the next loads
        });
        __builtin_amdgcn_sched_barrier(0);
        prefetch_part(nsrc, 0);
        dftT<R, T>(z);                                                // stage 1
        __builtin_amdgcn_sched_barrier(0);
        prefetch_part(nsrc, 1);
        dz[lane] = z[0];
        lds_gather_use<1, R, lds_batch<R, T>(), T>(t1L + lane, 64, [&](int q2, cx<T> wv) { dz[q2 * PITCH + lane] = cmulT(z[q2], wv); });
        wave_sync();
#pragma unroll
        for (int l2 = 0; l2 < R; l2++) z[l2] = dz[Q * PITCH + L1 + P * l2];
        prefetch_part(nsrc, 2);
        wave_sync();
        dftT<R, T>(z);                                                // stage 2
        __builtin_amdgcn_sched_barrier(0);
        prefetch_part(nsrc, 3);
        cx<T> tq2[R];
        if constexpr (lds_batch<R, T>() == R) lds_gather<1, R, T>(tq2, t2L + L1, P);
#pragma unroll
        for (int t = 0; t < R; t++) {
            // twiddle W_64^(l1 t2), then stage 3: P-point DFT across the P lanes of a group (decimation in frequency)
            cx<T> a = (t > 0) ? cmulT(z[t], lds_batch<R, T>() == R ? tq2[t] : t2L[t * P + L1]) : z[t];
            if constexpr (G::LOGP >= 1) {
                if constexpr (P >= 16) a = xstepT<8, true, T>(a, csg[G::LOGP - 4], cw[G::LOGP - 4]);
                if constexpr (P >= 8) a = xstepT<4, true, T>(a, csg[G::LOGP - 3], cw[G::LOGP - 3]);
                if constexpr (P >= 4) a = xstepT<2, true, T>(a, csg[G::LOGP - 2], cw[G::LOGP - 2]);
                a = xstepT<1, false, T>(a, csg[G::LOGP - 1], cw[G::LOGP - 1]);
            }
            dz[zpadT<R, T>(Q + R * t + G::R2 * t1v)] = a;
        }
        wave_sync();
        // ---- untangle into |X|^2: pairs (k, M-k), k = lane + 64 j2 (k_stft.hip); every Z is read before the first power
        // is written over it
        constexpr int NPAIR = R / 2;
        cx<T> za[NPAIR], zb[NPAIR];
#pragma unroll
        for (int j2 = 0; j2 < NPAIR; j2++) {
            const int k = lane + 64 * j2;
            za[j2] = dz[zpadT<R, T>(k)];
            zb[j2] = dz[zpadT<R, T>((M - k) & (M - 1))];
        }
        const cx<T> zc = dz[zpadT<R, T>(G::HALF)];
        wave_sync();
#pragma unroll
        for (int j2 = 0; j2 < NPAIR; j2++) {
            const int k = lane + 64 * j2;
            const cx<T> S = mkc<T>(za[j2].x + zb[j2].x, za[j2].y - zb[j2].y);
            const cx<T> D = mkc<T>(za[j2].x - zb[j2].x, za[j2].y + zb[j2].y);
            const cx<T> O = mkc<T>((T)0.5 * D.y, (T)-0.5 * D.x);
            const cx<T> Pk = cmulT(O, tw3[k]);
            const cx<T> x0 = mkc<T>(fmaT((T)0.5, S.x, Pk.x), fmaT((T)0.5, S.y, Pk.y));
            const cx<T> x1 = mkc<T>(fmaT((T)0.5, S.x, -Pk.x), -fmaT((T)0.5, S.y, -Pk.y));
            pwL[k] = x0.x * x0.x + x0.y * x0.y;
            pwL[M - k] = x1.x * x1.x + x1.y * x1.y;                   // k = 0: the Nyquist bin M = nwind/2
        }
        if (lane == 0) pwL[G::HALF] = zc.x * zc.x + zc.y * zc.y;      // bin M/2 pairs with itself: X = conj Z
        wave_sync();
        fbank_tail(p, j, lane, leL, [&](int k) { return pwL[k]; });   // (ends with a wave_sync: dz is free again)
    }
}

// ---- rows route ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fbank_rows(FbankParams p) {
    __shared__ double leS[4][PVX_FBANK_MAX_NBAND];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t j = (int64_t)blockIdx.x * 4 + wid;
    if (j >= p.nfr) return;                                           // (no workgroup barrier below)
    const double2* row = (const double2*)p.rows + j * p.ldo;
    fbank_tail(p, j, lane, leS[wid], [&](int k) { const double2 v = row[k]; return v.x * v.x + v.y * v.y; });
}

template <int R> int launch_fused(const FbankParams& p, int x_dtype, hipStream_t s) {
    using G = StftGeo<R, double>;
    int dev = 0, ncu = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ncu = v;
    }
    int nw = 6;
    while (nw > 1 && G::total(nw) > 160 * 1024) nw--;
    const size_t lds = G::total(nw);
    const void* fn = nullptr;
    switch (x_dtype) {
        case PVX_F32: fn = (const void*)k_fbank_fused<R, float>; break;
        case PVX_F64: fn = (const void*)k_fbank_fused<R, double>; break;
        case PVX_I16: fn = (const void*)k_fbank_fused<R, int16_t>; break;
        default: pvx_set_error("bad x_dtype %d", x_dtype); return PVX_ERR_INVALID;
    }
    if (lds > 64 * 1024) PVX_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int per_cu = (int)((160 * 1024) / lds);                            // workgroups that fit a CU's LDS side by side
    if (per_cu < 1) per_cu = 1;
    if (per_cu * nw > 16) per_cu = 16 / nw > 0 ? 16 / nw : 1;
    { const int nb = pvx_resident_blocks(fn, 64 * nw, lds); if (nb >= 1 && nb < per_cu) per_cu = nb; }      // (registers: pvx_internal.h)
    int64_t nblocks = (int64_t)ncu * per_cu;
    const int64_t maxb = (p.nfr + nw - 1) / nw;
    if (nblocks > maxb) nblocks = maxb > 0 ? maxb : 1;
    FbankParams arg = p;
    void* args[] = {&arg};
    PVX_HIP_CHECK(hipLaunchKernel(fn, dim3((unsigned)nblocks), dim3(64 * nw), args, lds, s));
    return PVX_OK;
}

// ---- per-device workspace (pvx_fbank_ws.h): tables of the call, the rows route's buffers and rocFFT plans
std::mutex g_ws_mu;
std::map<int, FbankWs*> g_ws;                                         // device -> workspace (never erased)
constexpr size_t kMaxPlans = 4;                                       // window lengths with a live rocFFT plan


// rows per rocFFT batch: the windowed frames of a batch stay near 32 MB (and the half-spectrum rows beside them).  Fixed per
// nwind, whatever the call's frame count: a row's spectrum does not depend on how many rows the call has
int64_t rows_batch(int nwind) {
    const int64_t c = ((int64_t)32 << 20) / ((int64_t)nwind * 8);
    return c < 1 ? 1 : c;
}

}  // namespace

int pvx_fbank_ensure_plan(FbankWs& w, int nwind, FftPlan** out) {
    auto it = w.plans.find(nwind);
    if (it != w.plans.end()) { *out = &it->second; return PVX_OK; }
    if (w.plans.size() >= kMaxPlans) w.plans.clear();
    FftPlan fp;
    fp.batch = rows_batch(nwind);
    rocfft_status st;
    switch (fp.fft.create((size_t)nwind, (size_t)fp.batch, rocfft_precision_double, rocfft_placement_notinplace, (size_t)nwind, (size_t)(nwind / 2 + 1), &st)) {
        case RealFft::done: break;
        case RealFft::describe: pvx_set_error("rocfft_plan_description_create failed: rocfft_status %d", (int)st); return PVX_ERR_HIP;
        case RealFft::plan: pvx_set_error("rocfft_plan_create(nwind=%d, batch=%lld) failed: %d", nwind, (long long)fp.batch, (int)st); return PVX_ERR_HIP;
        case RealFft::info: pvx_set_error("rocfft execution setup (nwind=%d) failed", nwind); return PVX_ERR_HIP;
    }
    const size_t wb = fp.fft.work_bytes();
    if (wb > w.work.cap()) {
        // the plans share one work buffer (calls take turns); a larger one invalidates what the other plans were told: the old
        // one goes only once the new one exists, and every live plan hears of it
        DevMem larger;
        if (larger.alloc(wb) != PVX_OK) { pvx_set_error("hipMalloc(rocfft work, %zu) failed", wb); return PVX_ERR_ALLOC; }
        w.work = std::move(larger);
        for (auto& kv : w.plans) (void)kv.second.fft.set_work(w.work.get(), w.work.cap());
    }
    if (w.work && fp.fft.set_work(w.work.get(), w.work.cap()) != rocfft_status_success) {
        pvx_set_error("rocfft set_work_buffer failed");
        return PVX_ERR_HIP;
    }
    *out = &(w.plans[nwind] = std::move(fp));
    return PVX_OK;
}

namespace {

const double kPiD = 3.141592653589793238462643383279502884;

// cep[c] = sum_n L[n] * re[n][c] (+ i im[n][c]): the transforms' defining sums (scipy.fftpack.dct, norm=None; np.fft.ifft)
void cep_matrices(int mode, int N, double* re, double* im) {
    for (int n = 0; n < N; n++)
        for (int k = 0; k < N; k++) {
            double v = 0.0, u = 0.0;
            switch (mode) {
                case 1: v = n == 0 ? 1.0 : (n == N - 1 ? ((k & 1) ? -1.0 : 1.0) : 2.0 * cos(kPiD * (double)k * (double)n / (double)(N - 1))); break;
                case 2: v = 2.0 * cos(kPiD * (double)k * (double)(2 * n + 1) / (double)(2 * N)); break;
                case 3: v = n == 0 ? 1.0 : 2.0 * cos(kPiD * (double)(2 * k + 1) * (double)n / (double)(2 * N)); break;
                case 4: v = 2.0 * cos(kPiD * (double)(2 * k + 1) * (double)(2 * n + 1) / (double)(4 * N)); break;
                default: {
                    const int m = (int)(((int64_t)k * n) % N);       // the angle reduced exactly
                    v = cos(2.0 * kPiD * (double)m / (double)N) / (double)N;
                    u = sin(2.0 * kPiD * (double)m / (double)N) / (double)N;
                }
            }
            re[(size_t)n * N + k] = v;
            if (im) im[(size_t)n * N + k] = u;
        }
}

// the reference's cepstral row of a frame whose log energies are all -inf (scipy 1.15 / numpy; FILTERBANK.md):
// DCT1, DCT2: [-inf, nan, ...]; DCT3, DCT4: all nan; IFFT: [-inf+0j, nan+nanj, ...]
void silent_row(int mode, int N, double* out) {
    const double ninf = -INFINITY, qnan = NAN;
    if (mode == 5) {
        for (int k = 0; k < N; k++) { out[2 * k] = k == 0 ? ninf : qnan; out[2 * k + 1] = k == 0 ? 0.0 : qnan; }
    } else {
        for (int k = 0; k < N; k++) out[k] = (k == 0 && mode <= 2) ? ninf : qnan;
    }
}

bool fbank_fused_takes(int nwind) {
    return (nwind == 512 || nwind == 1024 || nwind == 2048) && getenv("PVX_FBANK_ROWS") == nullptr;
}

int run_locked(FbankWs& w, const void* d_x, int x_dtype, int64_t nfr, const double* h_wind, int nwind, int hop, const double* h_fb,
               int nband, int cep_mode, double* d_spec, double* d_cep, hipStream_t s, const char** kernels) {
    const bool fused = fbank_fused_takes(nwind);
    const int nhalf = nwind / 2 + 1;
    // fold fb onto the half spectrum (FFTFilters.py:286: sum over all nwind bins of |X|^2 * fb): bin 0 and, for even nwind,
    // bin nwind/2 are their own mirror images
    std::vector<double>& t = w.h_tab;
    std::vector<int>& hb = w.h_band;
    t.clear(); hb.assign((size_t)3 * nband, 0);
    t.insert(t.end(), h_wind, h_wind + nwind);
    const size_t off_tw = t.size();
    if (fused) {
        t.resize(off_tw + 2 * (size_t)nwind);
        for (int j = 0; j < nwind; j++) {
            t[off_tw + 2 * j] = cos(2.0 * kPiD * j / (double)nwind);
            t[off_tw + 2 * j + 1] = -sin(2.0 * kPiD * j / (double)nwind);
        }
    }
    const size_t off_wf = t.size();
    {
        std::vector<double> row((size_t)nhalf);
        for (int b = 0; b < nband; b++) {
            const double* f = h_fb + (size_t)b * nwind;
            int lo = nhalf, hi = -1;
            for (int k = 0; k < nhalf; k++) {
                const int m = nwind - k;
                row[k] = (k == 0 || m == k) ? f[k] : f[k] + f[m];
                if (row[k] != 0.0) { if (k < lo) lo = k; hi = k; }
            }
            const int n = hi >= lo ? hi - lo + 1 : 0;
            hb[b] = n ? lo : 0; hb[nband + b] = n; hb[2 * nband + b] = (int)(t.size() - off_wf);
            if (n) t.insert(t.end(), row.begin() + lo, row.begin() + hi + 1);
        }
    }
    const size_t off_cre = t.size();
    size_t off_cim = off_cre, off_sil = off_cre;
    if (cep_mode) {
        const size_t nn = (size_t)nband * nband;
        t.resize(off_cre + nn * (cep_mode == 5 ? 2 : 1) + (size_t)nband * 2);
        off_cim = off_cre + nn;
        off_sil = off_cre + nn * (cep_mode == 5 ? 2 : 1);
        cep_matrices(cep_mode, nband, &t[off_cre], cep_mode == 5 ? &t[off_cim] : nullptr);
        silent_row(cep_mode, nband, &t[off_sil]);
    }
    int rc;
    if ((rc = w.tab.grow(t.size() * 8, Sizing::exact)) != PVX_OK || (rc = w.band.grow(hb.size() * 4, Sizing::exact)) != PVX_OK) return rc;
    PVX_HIP_CHECK(hipMemcpyAsync(w.tab.get(), t.data(), t.size() * 8, hipMemcpyHostToDevice, s));
    PVX_HIP_CHECK(hipMemcpyAsync(w.band.get(), hb.data(), hb.size() * 4, hipMemcpyHostToDevice, s));
    const double* dt = w.tab.as<const double>();
    FbankParams p = {};
    p.hop = hop; p.nband = nband; p.cep_mode = cep_mode;
    p.win = dt; p.twiddle = dt + off_tw;
    p.band_lo = w.band.as<const int>(); p.band_n = p.band_lo + nband; p.band_off = p.band_lo + 2 * nband;
    p.wf = dt + off_wf; p.cre = dt + off_cre; p.cim = dt + off_cim; p.silent = dt + off_sil;
    const int cpx = cep_mode == 5 ? 2 : 1;
    if (fused) {
        p.x = d_x; p.nfr = nfr; p.spec = d_spec; p.cep = d_cep;
        switch (nwind) {
            case 512: rc = launch_fused<4>(p, x_dtype, s); *kernels = "k_fbank_fused<512>"; break;
            case 1024: rc = launch_fused<8>(p, x_dtype, s); *kernels = "k_fbank_fused<1024>"; break;
            default: rc = launch_fused<16>(p, x_dtype, s); *kernels = "k_fbank_fused<2048>"; break;
        }
        if (rc != PVX_OK) return rc;
    } else {
        FftPlan* fp = nullptr;
        if ((rc = pvx_fbank_ensure_plan(w, nwind, &fp)) != PVX_OK) return rc;
        const int64_t batch = fp->batch;
        if ((rc = w.frames.grow((size_t)batch * nwind * 8, Sizing::exact)) != PVX_OK ||
            (rc = w.spec.grow((size_t)batch * nhalf * 16, Sizing::exact)) != PVX_OK) return rc;
        for (int64_t c0 = 0; c0 < nfr; c0 += batch) {
            const int64_t rows = nfr - c0 < batch ? nfr - c0 : batch;
            // workspace row j = frame c0 + j in k_frames' row space (pvx_internal.h: global row g holds frame g - 1)
            FrameParams fr = {};
            fr.x = d_x; fr.nsamp = 0; fr.sig_stride = 0; fr.F = nfr; fr.R0 = c0 + 2; fr.ws_rows = rows; fr.total_rows = nfr + 1;
            fr.nfft = nwind; fr.hop = hop; fr.win = dt; fr.frames = w.frames.get(); fr.ldi = nwind;
            if ((rc = pvx_launch_frames(fr, x_dtype, 64, s)) != PVX_OK) return rc;
            PVX_FFT_CHECK(fp->fft.execute(w.frames.get(), w.spec.get(), s));   // the whole batch: rows beyond `rows` are not read
            p.rows = w.spec.get(); p.ldo = nhalf; p.nfr = rows;
            p.spec = d_spec ? d_spec + c0 * nband : nullptr;
            p.cep = d_cep ? d_cep + c0 * (int64_t)(nband * cpx) : nullptr;
            hipLaunchKernelGGL(k_fbank_rows, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, p);
            PVX_HIP_CHECK(hipGetLastError());
        }
        *kernels = "k_frames+rocfft+k_fbank_rows";
    }
    PVX_HIP_CHECK(hipStreamSynchronize(s));
    return PVX_OK;
}

}  // namespace

int pvx_fbank_workspace(FbankWs** ws) {
    int dev = 0;
    PVX_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_ws_mu);
    FbankWs*& e = g_ws[dev];
    if (!e) e = new FbankWs();
    *ws = e;
    return PVX_OK;
}

int pvx_fbank_run(const void* d_x, int x_dtype, int64_t nfr, const double* h_wind, int nwind, int hop, const double* h_fb, int nband,
                  int cep_mode, double* d_spec, double* d_cep, hipStream_t s, const char** kernels) {
    if (nfr <= 0) return PVX_OK;
    FbankWs* w;
    int rc;
    if ((rc = pvx_fbank_workspace(&w)) != PVX_OK) return rc;
    std::lock_guard<std::mutex> lk(w->mu);
    return run_locked(*w, d_x, x_dtype, nfr, h_wind, nwind, hop, h_fb, nband, cep_mode, d_spec, d_cep, s, kernels);
}

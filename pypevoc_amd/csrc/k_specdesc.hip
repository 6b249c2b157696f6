// k_specdesc.hip -- windowed spectral measures over the half spectrum |X_i[k]|, k = 0 .. nwind/2, of the frames
//   X_i = fft(x[i*hop : i*hop+nwind] * wind)
// of a call (pypevoc/SoundUtils.py: SpecCentWind :142-160, SpecFlux :196-231; speech/SpeechAnalysis.py: SpectralMoments
// :82-139).  float64 throughout.  Design and numbers: SPECDESC.md.
//   ratio  out[i] = sum_k a[k] |X_i[k]| / sum_k b[k] |X_i[k]|
//   flux   out[i] = sqrt(sum_k a[k] (|X_i[k]| - |X_{i+1}[k]|)^2)           (nfr values from nfr + 1 spectra)
//   psd    P[k]   = (1 / total) sum_i |X_i[k]|^2,  k < nwind/2
// a, b: the caller's weights per half-spectrum bin (the host folds the reference's full-spectrum bin ranges onto them).
//
// Two routes, as in k_fbank.hip:
//   fused  nwind 512 / 1024 / 2048: k_specdesc_fused, the single-wave transform of pvx_stft.h exactly as k_fbank_fused runs
//          it.  A wave walks a contiguous run of frames; the magnitudes of the previous frame (flux) or the sums of the block
//          (psd) stay in its registers, so a flux run costs one extra transform at its head and no spectrum row reaches
//          global memory.
//   rows   any other nwind: k_frames + a batched real rocFFT into the workspace shared with k_fbank.hip, then
//          k_specdesc_rows, a wave per value (ratio, flux) or per block of frames (psd).
// Every sum has a fixed order: a value is the work of one wave, lanes stride over the bins and wave_sum joins them.  The
// periodogram adds its frames in blocks of PVX_SPECDESC_BLOCK, frame after frame within a block, and k_specdesc_mean adds the
// blocks' partial sums one after the other in index order: no atomics, and the bits depend neither on the grid nor on how a
// long signal was cut into calls (the cuts fall on block boundaries).
#include <math.h>

#include <algorithm>
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

struct SdParams {
    const void* x;            // samples of frame 0 (fused) ...
    const void* rows;         // ... or complex double [spectra][ldo] half-spectrum rows (rows route)
    int64_t ldo;
    int64_t nfr;              // values (ratio, flux) or frames (psd) of this launch
    int hop, meas, run;       // run: frames a wave takes in one go (fused; psd: PVX_SPECDESC_BLOCK on both routes)
    int nhalf, nbin;          // nwind/2 + 1 bins of a spectrum; psd: the nwind/2 of them that are kept
    const double* win;        // [nwind]
    const void* twiddle;      // complex double [nwind] W_nwind^j (fused)
    const double* a;          // [nhalf] (ratio, flux)
    const double* b;          // [nhalf] (ratio)
    double* out;              // [nfr] (ratio, flux)
    double* part;             // [ceil(nfr / run)][nbin] (psd)
};

// ---- fused route -----------------------------------------------------------------------------------------------------
// The transform is k_fbank_fused's, stage for stage; the untangle keeps the magnitudes (or powers) in registers: lane l
// owns bins l + 64 j2 and M - (l + 64 j2), lane 0 also bin M/2.
template <int R> constexpr size_t sd_lds_bytes(int nw) { return StftGeo<R, double>::total(nw) + 2 * (size_t)(64 * R + 8) * sizeof(double); }

// Waves of a workgroup: six as in k_fbank_fused, four at nwind 2048, where the 34 registers of the kept magnitudes on top of the
// transform's need more than the 256 that two waves on a SIMD leave each.
template <int R> constexpr int sd_waves() { return R == 16 ? 4 : 6; }

template <int R, typename InT>
__global__ __launch_bounds__(64 * sd_waves<R>()) void k_specdesc_fused(SdParams p) {
    using T = double;
    using G = StftGeo<R, T>;
    constexpr int M = G::M, P = G::P, PITCH = G::PITCH;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nw = blockDim.x >> 6;
    T* const winL = (T*)(smem + G::OFF_WIN);
    cx<T>* const t1L = (cx<T>*)(smem + G::OFF_T1);
    cx<T>* const t2L = (cx<T>*)(smem + G::OFF_T2);
    cx<T>* const tw3 = (cx<T>*)(smem + G::OFF_TW3);
    cx<T>* const dz = (cx<T>*)(smem + G::OFF_BUF) + (size_t)wid * G::BUFC;
    double* const waL = (double*)(smem + G::total(nw));               // [M + 1] weights a, b of the workgroup
    double* const wbL = waL + M + 8;
    const cx<T>* const tab = (const cx<T>*)p.twiddle;
    constexpr int NMASK = G::N - 1;
    const int meas = p.meas;
    for (int i = threadIdx.x; i < G::N; i += blockDim.x) winL[i] = p.win[i];
    for (int i = threadIdx.x; i < R * 64; i += blockDim.x) t1L[i] = tab[(2 * (i & 63) * (i >> 6)) & NMASK];
    for (int i = threadIdx.x; i < 64; i += blockDim.x) t2L[i] = tab[((G::N / 64) * (i % P) * (i / P)) & NMASK];   // [t2][l1]
    for (int i = threadIdx.x; i <= G::HALF; i += blockDim.x) tw3[i] = tab[i];
    for (int i = threadIdx.x; i <= M; i += blockDim.x) {
        waL[i] = meas != PVX_SD_PSD ? p.a[i] : 0.0;
        wbL[i] = meas == PVX_SD_RATIO ? p.b[i] : 0.0;
    }
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

    // runs of p.run frames are dealt round-robin to the waves of the grid; a flux run also transforms the frame after its
    // last one.  The samples of a wave's next frame are prefetched in four groups spread over the transform
    const int64_t W = (int64_t)gridDim.x * nw;
    const int64_t run = p.run;
    const int64_t nunits = (p.nfr + run - 1) / run;
    const int extra = meas == PVX_SD_FLUX ? 1 : 0;
    auto unit_end = [&](int64_t u) -> int64_t { const int64_t e = (u + 1) * run; return (e < p.nfr ? e : p.nfr) + extra; };
    int64_t u = (int64_t)blockIdx.x * nw + wid;
    if (u >= nunits) return;                                          // (no workgroup barrier below)
    int64_t j = u * run, jend = unit_end(u);
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
        const InT* s0 = (const InT*)p.x + j * (int64_t)p.hop;
        prefetch_part(s0, 0); prefetch_part(s0, 1); prefetch_part(s0, 2); prefetch_part(s0, 3);
    }
    constexpr int NPAIR = R / 2;
    double st0[NPAIR], st1[NPAIR], stH = 0.0;                         // flux: the previous frame's magnitudes; psd: the block's sums
#pragma unroll
    for (int j2 = 0; j2 < NPAIR; j2++) { st0[j2] = 0.0; st1[j2] = 0.0; }
    for (;;) {
        const bool head = j == u * run;
        int64_t nj = j + 1, nu = u, nend = jend;
        if (nj >= jend) { nu = u + W; nj = nu * run; nend = nu < nunits ? unit_end(nu) : 0; }
        const InT* nsrc = nu < nunits ? (const InT*)p.x + nj * (int64_t)p.hop : nullptr;
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
        // ---- untangle: pairs (k, M-k), k = lane + 64 j2 (k_stft.hip); every Z is read before the next frame writes dz
        cx<T> za[NPAIR], zb[NPAIR];
#pragma unroll
        for (int j2 = 0; j2 < NPAIR; j2++) {
            const int k = lane + 64 * j2;
            za[j2] = dz[zpadT<R, T>(k)];
            zb[j2] = dz[zpadT<R, T>((M - k) & (M - 1))];
        }
        const cx<T> zc = dz[zpadT<R, T>(G::HALF)];
        wave_sync();
        double sa = 0.0, sb = 0.0;
#pragma unroll
        for (int j2 = 0; j2 < NPAIR; j2++) {
            const int k = lane + 64 * j2;
            const cx<T> S = mkc<T>(za[j2].x + zb[j2].x, za[j2].y - zb[j2].y);
            const cx<T> D = mkc<T>(za[j2].x - zb[j2].x, za[j2].y + zb[j2].y);
            const cx<T> O = mkc<T>((T)0.5 * D.y, (T)-0.5 * D.x);
            const cx<T> Pk = cmulT(O, tw3[k]);
            const cx<T> x0 = mkc<T>(fmaT((T)0.5, S.x, Pk.x), fmaT((T)0.5, S.y, Pk.y));
            const cx<T> x1 = mkc<T>(fmaT((T)0.5, S.x, -Pk.x), -fmaT((T)0.5, S.y, -Pk.y));
            const double q0 = x0.x * x0.x + x0.y * x0.y;             // bin k
            const double q1 = x1.x * x1.x + x1.y * x1.y;             // bin M - k (k = 0: the Nyquist bin M = nwind/2)
            if (meas == PVX_SD_PSD) {
                st0[j2] = head ? q0 : st0[j2] + q0;
                st1[j2] = head ? q1 : st1[j2] + q1;
            } else {
                const double m0 = sqrt(q0), m1 = sqrt(q1);
                if (meas == PVX_SD_RATIO) {
                    sa += waL[k] * m0; sa += waL[M - k] * m1;
                    sb += wbL[k] * m0; sb += wbL[M - k] * m1;
                } else {
                    const double d0 = st0[j2] - m0, d1 = st1[j2] - m1;
                    sa += waL[k] * (d0 * d0); sa += waL[M - k] * (d1 * d1);
                    st0[j2] = m0; st1[j2] = m1;
                }
            }
        }
        {
            const double qh = zc.x * zc.x + zc.y * zc.y;             // bin M/2 pairs with itself: X = conj Z
            if (meas == PVX_SD_PSD) {
                stH = head ? qh : stH + qh;
            } else {
                const double mh = sqrt(qh);
                if (meas == PVX_SD_RATIO) {
                    if (lane == 0) { sa += waL[G::HALF] * mh; sb += wbL[G::HALF] * mh; }
                } else {
                    const double dh = stH - mh;
                    if (lane == 0) sa += waL[G::HALF] * (dh * dh);
                    stH = mh;
                }
            }
        }
        if (meas == PVX_SD_RATIO) {
            const double ta = wave_sum(sa), tb = wave_sum(sb);
            if (lane == 0) p.out[j] = ta / tb;
        } else if (meas == PVX_SD_FLUX) {
            const double ta = wave_sum(sa);                           // (at a run's head: against the zeros st started from)
            if (!head && lane == 0) p.out[j - 1] = sqrt(ta);
        } else if (j + 1 == jend) {
            double* po = p.part + u * (int64_t)p.nbin;                // nbin = M: the Nyquist bin is not kept
#pragma unroll
            for (int j2 = 0; j2 < NPAIR; j2++) {
                const int k = lane + 64 * j2;
                po[k] = st0[j2];
                if (M - k < p.nbin) po[M - k] = st1[j2];
            }
            if (lane == 0) po[G::HALF] = stH;
        }
        if (nu >= nunits) break;
        j = nj; u = nu; jend = nend;
    }
}

// ---- rows route ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_specdesc_rows(SdParams p) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t unit = (int64_t)blockIdx.x * 4 + wid;
    const double2* rows = (const double2*)p.rows;
    if (p.meas == PVX_SD_PSD) {
        const int64_t f0 = unit * p.run;
        if (f0 >= p.nfr) return;
        const int64_t f1 = f0 + p.run < p.nfr ? f0 + p.run : p.nfr;
        for (int k = lane; k < p.nbin; k += 64) {
            double s = 0.0;
            for (int64_t f = f0; f < f1; f++) { const double2 v = rows[f * p.ldo + k]; s += v.x * v.x + v.y * v.y; }
            p.part[unit * p.nbin + k] = s;
        }
        return;
    }
    if (unit >= p.nfr) return;
    const double2* r0 = rows + unit * p.ldo;
    double sa = 0.0, sb = 0.0;
    if (p.meas == PVX_SD_RATIO) {
        for (int k = lane; k < p.nhalf; k += 64) {
            const double2 v = r0[k];
            const double m = sqrt(v.x * v.x + v.y * v.y);
            sa += p.a[k] * m; sb += p.b[k] * m;
        }
        const double ta = wave_sum(sa), tb = wave_sum(sb);
        if (lane == 0) p.out[unit] = ta / tb;
    } else {
        const double2* r1 = r0 + p.ldo;
        for (int k = lane; k < p.nhalf; k += 64) {
            const double2 v = r0[k], n = r1[k];
            const double d = sqrt(v.x * v.x + v.y * v.y) - sqrt(n.x * n.x + n.y * n.y);
            sa += p.a[k] * (d * d);
        }
        const double ta = wave_sum(sa);
        if (lane == 0) p.out[unit] = sqrt(ta);
    }
}

// acc[k] (+)= part[0][k] + part[1][k] + ...  one block after the other; the call's last pass divides by the frame count
__global__ __launch_bounds__(256) void k_specdesc_mean(const double* part, int64_t nblk, int nbin, double* acc, int first, double total) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nbin) return;
    double s = first ? 0.0 : acc[k];
    for (int64_t b = 0; b < nblk; b++) s += part[b * nbin + k];
    acc[k] = total > 0.0 ? s / total : s;
}

template <int R> int launch_fused(const SdParams& p, int x_dtype, hipStream_t s) {
    int dev = 0, ncu = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ncu = v;
    }
    int nw = sd_waves<R>();
    while (nw > 1 && sd_lds_bytes<R>(nw) > 160 * 1024) nw--;
    const size_t lds = sd_lds_bytes<R>(nw);
    const void* fn = nullptr;
    switch (x_dtype) {
        case PVX_F32: fn = (const void*)k_specdesc_fused<R, float>; break;
        case PVX_F64: fn = (const void*)k_specdesc_fused<R, double>; break;
        case PVX_I16: fn = (const void*)k_specdesc_fused<R, int16_t>; break;
        default: pvx_set_error("bad x_dtype %d", x_dtype); return PVX_ERR_INVALID;
    }
    if (lds > 64 * 1024) PVX_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int per_cu = (int)((160 * 1024) / lds);                            // workgroups that fit a CU's LDS side by side
    if (per_cu < 1) per_cu = 1;
    if (per_cu * nw > 16) per_cu = 16 / nw > 0 ? 16 / nw : 1;
    { const int nb = pvx_resident_blocks(fn, 64 * nw, lds); if (nb >= 1 && nb < per_cu) per_cu = nb; }      // (registers: pvx_internal.h)
    int64_t nblocks = (int64_t)ncu * per_cu;
    const int64_t nunits = (p.nfr + p.run - 1) / p.run;
    const int64_t maxb = (nunits + nw - 1) / nw;
    if (nblocks > maxb) nblocks = maxb > 0 ? maxb : 1;
    SdParams arg = p;
    void* args[] = {&arg};
    PVX_HIP_CHECK(hipLaunchKernel(fn, dim3((unsigned)nblocks), dim3(64 * nw), args, lds, s));
    return PVX_OK;
}

const double kPiD = 3.141592653589793238462643383279502884;
constexpr int64_t kPsdGroup = (int64_t)4096 * PVX_SPECDESC_BLOCK;     // frames whose block partials the workspace holds at a time (fused)

bool fused_takes(int nwind) {
    return (nwind == 512 || nwind == 1024 || nwind == 2048) && getenv("PVX_SPECDESC_ROWS") == nullptr;
}

// frames of a flux or ratio run, from the frame count alone: 4, and twice that while there are more than 8192 runs (up to
// 32): a flux run's extra transform is a quarter of its work at most, and a short call still spreads over many waves
int run_length(int64_t nfr) {
    int run = 4;
    while (run < 32 && nfr > (int64_t)run * 8192) run *= 2;
    return run;
}

int mean_pass(FbankWs& w, int64_t nblk, int nbin, double* d_acc, bool first, double total, hipStream_t s) {
    hipLaunchKernelGGL(k_specdesc_mean, dim3((unsigned)((nbin + 255) / 256)), dim3(256), 0, s, w.part.as<const double>(), nblk, nbin, d_acc,
                       first ? 1 : 0, total);
    PVX_HIP_CHECK(hipGetLastError());
    return PVX_OK;
}

int run_locked(FbankWs& w, const void* d_x, int x_dtype, int64_t nfr, const double* h_wind, int nwind, int hop, int meas, const double* h_a,
               const double* h_b, double* d_out, bool first, int64_t total, hipStream_t s, const char** kernels) {
    const bool fused = fused_takes(nwind);
    const int nhalf = nwind / 2 + 1, nbin = nwind / 2;
    const bool psd = meas == PVX_SD_PSD;
    std::vector<double>& t = w.h_tab;
    t.clear();
    t.insert(t.end(), h_wind, h_wind + nwind);
    const size_t off_tw = t.size();
    if (fused) {
        t.resize(off_tw + 2 * (size_t)nwind);
        for (int j = 0; j < nwind; j++) {
            t[off_tw + 2 * j] = cos(2.0 * kPiD * j / (double)nwind);
            t[off_tw + 2 * j + 1] = -sin(2.0 * kPiD * j / (double)nwind);
        }
    }
    const size_t off_a = t.size();
    if (!psd) t.insert(t.end(), h_a, h_a + nhalf);
    const size_t off_b = t.size();
    if (meas == PVX_SD_RATIO) t.insert(t.end(), h_b, h_b + nhalf);
    int rc;
    if ((rc = w.tab.grow(t.size() * 8, Sizing::exact)) != PVX_OK) return rc;
    PVX_HIP_CHECK(hipMemcpyAsync(w.tab.get(), t.data(), t.size() * 8, hipMemcpyHostToDevice, s));
    const double* dt = w.tab.as<const double>();
    SdParams p = {};
    p.hop = hop; p.meas = meas; p.nhalf = nhalf; p.nbin = nbin;
    p.run = psd ? PVX_SPECDESC_BLOCK : run_length(nfr);
    p.win = dt; p.twiddle = dt + off_tw; p.a = dt + off_a; p.b = dt + off_b;
    const size_t es = x_dtype == PVX_F64 ? 8 : (x_dtype == PVX_F32 ? 4 : 2);
    const double divisor = total > 0 ? (double)total : 0.0;
    if (fused) {
        const int64_t group = psd ? kPsdGroup : nfr;
        if (psd && (rc = w.part.grow((size_t)((std::min(group, nfr) + p.run - 1) / p.run) * nbin * 8, Sizing::exact)) != PVX_OK) return rc;
        for (int64_t g0 = 0; g0 < nfr; g0 += group) {
            const int64_t cnt = std::min(group, nfr - g0);
            p.x = (const char*)d_x + (size_t)(g0 * hop) * es; p.nfr = cnt; p.out = d_out; p.part = w.part.as<double>();
            switch (nwind) {
                case 512: rc = launch_fused<4>(p, x_dtype, s); *kernels = psd ? "k_specdesc_fused<512>+k_specdesc_mean" : "k_specdesc_fused<512>"; break;
                case 1024: rc = launch_fused<8>(p, x_dtype, s); *kernels = psd ? "k_specdesc_fused<1024>+k_specdesc_mean" : "k_specdesc_fused<1024>"; break;
                default: rc = launch_fused<16>(p, x_dtype, s); *kernels = psd ? "k_specdesc_fused<2048>+k_specdesc_mean" : "k_specdesc_fused<2048>"; break;
            }
            if (rc != PVX_OK) return rc;
            if (psd && (rc = mean_pass(w, (cnt + p.run - 1) / p.run, nbin, d_out, first && g0 == 0, g0 + cnt == nfr ? divisor : 0.0, s)) != PVX_OK) return rc;
        }
    } else {
        FftPlan* fp = nullptr;
        if ((rc = pvx_fbank_ensure_plan(w, nwind, &fp)) != PVX_OK) return rc;
        const int64_t batch = fp->batch;                              // spectra per rocFFT execution
        const int extra = meas == PVX_SD_FLUX ? 1 : 0;
        const int64_t step = psd ? batch - batch % PVX_SPECDESC_BLOCK : batch - extra;   // values (psd: frames) per batch
        if (step < 1) { pvx_set_error("pvx_specdesc: nwind %d is too long for the rows route", nwind); return PVX_ERR_UNSUPPORTED; }
        if ((rc = w.frames.grow((size_t)batch * nwind * 8, Sizing::exact)) != PVX_OK ||
            (rc = w.spec.grow((size_t)batch * nhalf * 16, Sizing::exact)) != PVX_OK) return rc;
        if (psd && (rc = w.part.grow((size_t)((std::min(step, nfr) + p.run - 1) / p.run) * nbin * 8, Sizing::exact)) != PVX_OK) return rc;
        const int64_t nspec = nfr + extra;
        for (int64_t c0 = 0; c0 < nfr; c0 += step) {
            const int64_t cnt = std::min(step, nfr - c0);
            // workspace row j = frame c0 + j in k_frames' row space (pvx_internal.h: global row g holds frame g - 1)
            FrameParams fr = {};
            fr.x = d_x; fr.nsamp = 0; fr.sig_stride = 0; fr.F = nspec; fr.R0 = c0 + 2; fr.ws_rows = cnt + extra; fr.total_rows = nspec + 1;
            fr.nfft = nwind; fr.hop = hop; fr.win = dt; fr.frames = w.frames.get(); fr.ldi = nwind;
            if ((rc = pvx_launch_frames(fr, x_dtype, 64, s)) != PVX_OK) return rc;
            PVX_FFT_CHECK(fp->fft.execute(w.frames.get(), w.spec.get(), s));   // the whole batch: rows beyond cnt + extra are not read
            p.rows = w.spec.get(); p.ldo = nhalf; p.nfr = cnt;
            p.out = psd ? nullptr : d_out + c0; p.part = w.part.as<double>();
            const int64_t units = psd ? (cnt + p.run - 1) / p.run : cnt;
            hipLaunchKernelGGL(k_specdesc_rows, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, s, p);
            PVX_HIP_CHECK(hipGetLastError());
            if (psd && (rc = mean_pass(w, units, nbin, d_out, first && c0 == 0, c0 + cnt == nfr ? divisor : 0.0, s)) != PVX_OK) return rc;
        }
        *kernels = psd ? "k_frames+rocfft+k_specdesc_rows+k_specdesc_mean" : "k_frames+rocfft+k_specdesc_rows";
    }
    PVX_HIP_CHECK(hipStreamSynchronize(s));
    return PVX_OK;
}

}  // namespace

int pvx_specdesc_run(const void* d_x, int x_dtype, int64_t nfr, const double* h_wind, int nwind, int hop, int meas, const double* h_a,
                     const double* h_b, double* d_out, bool first, int64_t total, hipStream_t s, const char** kernels) {
    if (nfr <= 0) return PVX_OK;
    FbankWs* w;
    int rc;
    if ((rc = pvx_fbank_workspace(&w)) != PVX_OK) return rc;
    std::lock_guard<std::mutex> lk(w->mu);
    return run_locked(*w, d_x, x_dtype, nfr, h_wind, nwind, hop, meas, h_a, h_b, d_out, first, total, s, kernels);
}

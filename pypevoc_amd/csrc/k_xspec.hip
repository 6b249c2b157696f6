// k_xspec.hip -- Welch-averaged cross and auto spectra of two signals, block by block (pypevoc/TransferFunctions.py:
// transferogram :112-185, tfe :21-26, and matplotlib.mlab's csd / psd / cohere behind them).  float64 throughout.  Design
// and numbers: TRANSFER.md.
// Block b of a call starts at sample b * delta of x (and of y), its segment s at s * step further on:
//   X_s = rfft(x[b*delta + s*step : .. + nwind] * wind),  Y_s likewise,  bins k = 0 .. nwind/2 (Nyquist included)
//   sxy[b][k] = (1/nseg) sum_s conj(Y_s[k]) X_s[k]      sxx[b][k] = (1/nseg) sum_s |X_s[k]|^2      syy likewise
// unscaled: the one-sided factor, Fs and sum(wind^2) are the host's.  y null: sxx only, and no second transform.
//
// Two routes, as in k_specdesc.hip:
//   fused  nwind 512 / 1024 / 2048: k_xspec_fused, the single-wave transform of pvx_stft.h exactly as k_specdesc_fused runs
//          it, twice per segment: X's half spectrum waits in the lane's registers while Y is transformed, the four sums per
//          bin stay in registers until the block's last segment.  No spectrum row reaches global memory.
//   rows   any other nwind: k_frames (a block is a "signal" of nseg frames, sig_stride = delta) + a batched real rocFFT into
//          the workspace shared with k_fbank.hip / k_specdesc.hip, then k_xspec_rows, a wave per block and 64 bins.
// A bin of a block is the work of one lane of one wave, the block's segments are added in index order: no atomics, and the
// bits depend neither on the grid nor on how a call was cut into batches or chunks (the cuts fall between blocks; a block
// too long for a batch is cut between segments and carries its sums through the outputs, which rounds nothing).
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

struct XsParams {
    const void* x;            // samples of block 0 (fused) ...
    const void* y;            // ... of the second signal; null: the auto spectrum of x alone
    const void* rows;         // complex double [..][ldo] half-spectrum rows (rows route): x's, then from row `yrow` on y's
    int64_t ldo, yrow;
    int64_t nblk;             // blocks of this launch
    int64_t delta;            // samples between block starts
    int step, nseg;           // samples between segment starts; segments of a block
    int rpb, lead, segn;      // rows route: rows per block, the first of them that is a segment, segments of this pass
    int first, last;          // rows route: this pass starts the sums from zero / ends them (divides by nseg)
    int two;                  // y (or its rows) present
    int nhalf;                // nwind/2 + 1 bins
    const double* win;        // [nwind]
    const void* twiddle;      // complex double [nwind] W_nwind^j (fused)
    double* sxy;              // [nblk][nhalf][2] (two)
    double* sxx;              // [nblk][nhalf]
    double* syy;              // [nblk][nhalf] (two)
};

// ---- fused route -----------------------------------------------------------------------------------------------------
// The transform is k_specdesc_fused's, stage for stage; the untangle leaves lane l with bins l + 64 j2 and M - (l + 64 j2)
// (lane 0 also bin M/2) of the spectrum in registers.
// Waves of a workgroup: six at nwind 512 as k_specdesc_fused; four from 1024 on, where the kept spectrum and the four sums
// (6 (R + 1) doubles) on top of the transform's registers need more than the 256 that two waves on a SIMD leave each.
template <int R> constexpr int xs_waves() { return R == 4 ? 6 : 4; }

template <int R, typename InT>
__global__ __launch_bounds__(64 * xs_waves<R>()) void k_xspec_fused(XsParams p) {
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
    const cx<T>* const tab = (const cx<T>*)p.twiddle;
    constexpr int NMASK = G::N - 1;
    const bool two = p.two != 0;
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

    // blocks are dealt round-robin to the waves of the grid; a wave transforms x's segment, then y's, segment after segment.
    // The samples of the wave's next transform are prefetched in four groups spread over the current one
    const int64_t W = (int64_t)gridDim.x * nw;
    int64_t b = (int64_t)blockIdx.x * nw + wid;
    if (b >= p.nblk) return;                                          // (no workgroup barrier below)
    int s = 0, sig = 0;
    auto src_of = [&](int64_t bb, int ss, int sg) -> const InT* {
        return (const InT*)(sg ? p.y : p.x) + bb * p.delta + (int64_t)ss * p.step;
    };
    T raw[2 * R];                                                     // samples (2l + 128 r, + 1) of the next transform
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
        const InT* s0 = src_of(b, 0, 0);
        prefetch_part(s0, 0); prefetch_part(s0, 1); prefetch_part(s0, 2); prefetch_part(s0, 3);
    }
    constexpr int NPAIR = R / 2;
    cx<T> hx0[NPAIR], hx1[NPAIR], hxH = mkc<T>((T)0, (T)0);           // x's spectrum of the segment, while y's is transformed
    cx<T> cxy0[NPAIR], cxy1[NPAIR], cxyH = mkc<T>((T)0, (T)0);        // the block's sums
    double pxx0[NPAIR], pxx1[NPAIR], pxxH = 0.0, pyy0[NPAIR], pyy1[NPAIR], pyyH = 0.0;
#pragma unroll
    for (int j2 = 0; j2 < NPAIR; j2++) {
        hx0[j2] = hx1[j2] = cxy0[j2] = cxy1[j2] = mkc<T>((T)0, (T)0);
        pxx0[j2] = pxx1[j2] = pyy0[j2] = pyy1[j2] = 0.0;
    }
    const double den = (double)p.nseg;
    for (;;) {
        const bool head = s == 0;
        int64_t nb = b;
        int ns = s, nsg = 0;
        if (two && sig == 0) nsg = 1;
        else if (++ns == p.nseg) { ns = 0; nb = b + W; }
        const InT* nsrc = nb < p.nblk ? src_of(nb, ns, nsg) : nullptr;
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
        // ---- untangle: pairs (k, M-k), k = lane + 64 j2 (k_stft.hip); every Z is read before the next transform writes dz
        cx<T> za[NPAIR], zb[NPAIR];
#pragma unroll
        for (int j2 = 0; j2 < NPAIR; j2++) {
            const int k = lane + 64 * j2;
            za[j2] = dz[zpadT<R, T>(k)];
            zb[j2] = dz[zpadT<R, T>((M - k) & (M - 1))];
        }
        const cx<T> zc = dz[zpadT<R, T>(G::HALF)];
        wave_sync();
        const bool hold = two && sig == 0;                            // x's spectrum: kept until y's is there
        // a = the spectrum of x, c = the spectrum just transformed (y's; x's own where there is no y)
        auto add = [&](cx<T> a, cx<T> c, cx<T>& sxy, double& sxx, double& syy) {
            const double qa = a.x * a.x + a.y * a.y;
            sxx = head ? qa : sxx + qa;
            if (two) {
                const double qc = c.x * c.x + c.y * c.y;
                const double re = c.x * a.x + c.y * a.y, im = c.x * a.y - c.y * a.x;      // conj(c) a
                syy = head ? qc : syy + qc;
                sxy.x = head ? re : sxy.x + re;
                sxy.y = head ? im : sxy.y + im;
            }
        };
#pragma unroll
        for (int j2 = 0; j2 < NPAIR; j2++) {
            const int k = lane + 64 * j2;
            const cx<T> S = mkc<T>(za[j2].x + zb[j2].x, za[j2].y - zb[j2].y);
            const cx<T> D = mkc<T>(za[j2].x - zb[j2].x, za[j2].y + zb[j2].y);
            const cx<T> O = mkc<T>((T)0.5 * D.y, (T)-0.5 * D.x);
            const cx<T> Pk = cmulT(O, tw3[k]);
            const cx<T> x0 = mkc<T>(fmaT((T)0.5, S.x, Pk.x), fmaT((T)0.5, S.y, Pk.y));         // bin k
            const cx<T> x1 = mkc<T>(fmaT((T)0.5, S.x, -Pk.x), -fmaT((T)0.5, S.y, -Pk.y));      // bin M - k (k = 0: the Nyquist bin)
            if (hold) {
                hx0[j2] = x0; hx1[j2] = x1;
            } else {
                add(two ? hx0[j2] : x0, x0, cxy0[j2], pxx0[j2], pyy0[j2]);
                add(two ? hx1[j2] : x1, x1, cxy1[j2], pxx1[j2], pyy1[j2]);
            }
        }
        {
            const cx<T> xh = mkc<T>(zc.x, -zc.y);                     // bin M/2 pairs with itself: X = conj Z
            if (hold) hxH = xh;
            else add(two ? hxH : xh, xh, cxyH, pxxH, pyyH);
        }
        if (!hold && s + 1 == p.nseg) {
            const int64_t o = b * (int64_t)p.nhalf;                   // nhalf = M + 1
            double2* const oxy = two ? (double2*)p.sxy + o : nullptr;
            double* const oxx = p.sxx + o;
            double* const oyy = two ? p.syy + o : nullptr;
#pragma unroll
            for (int j2 = 0; j2 < NPAIR; j2++) {
                const int k = lane + 64 * j2;
                oxx[k] = pxx0[j2] / den;
                oxx[M - k] = pxx1[j2] / den;
                if (two) {
                    oyy[k] = pyy0[j2] / den; oyy[M - k] = pyy1[j2] / den;
                    oxy[k] = make_double2(cxy0[j2].x / den, cxy0[j2].y / den);
                    oxy[M - k] = make_double2(cxy1[j2].x / den, cxy1[j2].y / den);
                }
            }
            if (lane == 0) {
                oxx[G::HALF] = pxxH / den;
                if (two) { oyy[G::HALF] = pyyH / den; oxy[G::HALF] = make_double2(cxyH.x / den, cxyH.y / den); }
            }
        }
        if (nb >= p.nblk) break;
        b = nb; s = ns; sig = nsg;
    }
}

// ---- rows route ------------------------------------------------------------------------------------------------------
// a wave per block and 64 bins (a bin's sums are one lane's, segment after segment: how the bins are dealt out changes no bit)
__global__ __launch_bounds__(256) void k_xspec_rows(XsParams p) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int ntile = (p.nhalf + 63) / 64;
    const int64_t unit = (int64_t)blockIdx.x * 4 + wid;
    const int64_t b = unit / ntile;
    const int k = (int)(unit - b * ntile) * 64 + lane;
    if (b >= p.nblk || k >= p.nhalf) return;
    const double2* xr = (const double2*)p.rows + (b * p.rpb + p.lead) * p.ldo + k;
    const double2* yr = xr + p.yrow * p.ldo;
    const int64_t o = b * (int64_t)p.nhalf + k;
    double sxx = 0.0, syy = 0.0, re = 0.0, im = 0.0;
    if (!p.first) {
        sxx = p.sxx[o];
        if (p.two) { syy = p.syy[o]; re = p.sxy[2 * o]; im = p.sxy[2 * o + 1]; }
    }
    for (int s = 0; s < p.segn; s++) {
        const double2 a = xr[s * p.ldo];
        sxx += a.x * a.x + a.y * a.y;
        if (p.two) {
            const double2 c = yr[s * p.ldo];
            syy += c.x * c.x + c.y * c.y;
            re += c.x * a.x + c.y * a.y;                              // conj(c) a
            im += c.x * a.y - c.y * a.x;
        }
    }
    if (p.last) { const double den = (double)p.nseg; sxx /= den; syy /= den; re /= den; im /= den; }
    p.sxx[o] = sxx;
    if (p.two) { p.syy[o] = syy; p.sxy[2 * o] = re; p.sxy[2 * o + 1] = im; }
}

template <int R> size_t xs_lds_bytes(int nw) { return StftGeo<R, double>::total(nw); }

template <int R> int launch_fused(const XsParams& p, int x_dtype, hipStream_t s) {
    int dev = 0, ncu = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ncu = v;
    }
    int nw = xs_waves<R>();
    while (nw > 1 && xs_lds_bytes<R>(nw) > 160 * 1024) nw--;
    const size_t lds = xs_lds_bytes<R>(nw);
    const void* fn = nullptr;
    switch (x_dtype) {
        case PVX_F32: fn = (const void*)k_xspec_fused<R, float>; break;
        case PVX_F64: fn = (const void*)k_xspec_fused<R, double>; break;
        case PVX_I16: fn = (const void*)k_xspec_fused<R, int16_t>; break;
        default: pvx_set_error("bad x_dtype %d", x_dtype); return PVX_ERR_INVALID;
    }
    if (lds > 64 * 1024) PVX_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int per_cu = (int)((160 * 1024) / lds);                            // workgroups that fit a CU's LDS side by side
    if (per_cu < 1) per_cu = 1;
    if (per_cu * nw > 16) per_cu = 16 / nw > 0 ? 16 / nw : 1;
    { const int nb = pvx_resident_blocks(fn, 64 * nw, lds); if (nb >= 1 && nb < per_cu) per_cu = nb; }      // (registers: pvx_internal.h)
    int64_t nblocks = (int64_t)ncu * per_cu;
    const int64_t maxb = (p.nblk + nw - 1) / nw;
    if (nblocks > maxb) nblocks = maxb > 0 ? maxb : 1;
    XsParams arg = p;
    void* args[] = {&arg};
    PVX_HIP_CHECK(hipLaunchKernel(fn, dim3((unsigned)nblocks), dim3(64 * nw), args, lds, s));
    return PVX_OK;
}

const double kPiD = 3.141592653589793238462643383279502884;

bool fused_takes(int nwind) {
    return (nwind == 512 || nwind == 1024 || nwind == 2048) && getenv("PVX_XSPEC_ROWS") == nullptr;
}

int frames_of(const void* d_sig, int x_dtype, size_t es, int64_t sig_off, int64_t sig_stride, int64_t F, int64_t R0, int64_t ws_rows,
              int64_t total_rows, int nwind, int step, const double* d_win, double* frames, hipStream_t s) {
    FrameParams fr = {};
    fr.x = (const char*)d_sig + (size_t)sig_off * es; fr.nsamp = 0; fr.sig_stride = sig_stride; fr.F = F; fr.R0 = R0; fr.ws_rows = ws_rows;
    fr.total_rows = total_rows; fr.nfft = nwind; fr.hop = step; fr.win = d_win; fr.frames = frames; fr.ldi = nwind;
    return pvx_launch_frames(fr, x_dtype, 64, s);
}

int run_locked(FbankWs& w, const void* d_x, const void* d_y, int x_dtype, const double* h_wind, int nwind, int step, int64_t delta, int64_t nblk,
               int nseg, double* d_sxy, double* d_sxx, double* d_syy, hipStream_t s, const char** kernels) {
    const bool fused = fused_takes(nwind);
    const bool two = d_y != nullptr;
    const int nhalf = nwind / 2 + 1;
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
    int rc;
    if ((rc = w.tab.grow(t.size() * 8, Sizing::exact)) != PVX_OK) return rc;
    PVX_HIP_CHECK(hipMemcpyAsync(w.tab.get(), t.data(), t.size() * 8, hipMemcpyHostToDevice, s));
    const double* dt = w.tab.as<const double>();
    XsParams p = {};
    p.delta = delta; p.step = step; p.nseg = nseg; p.two = two ? 1 : 0; p.nhalf = nhalf;
    p.win = dt; p.twiddle = dt + off_tw;
    const size_t es = x_dtype == PVX_F64 ? 8 : (x_dtype == PVX_F32 ? 4 : 2);
    if (fused) {
        p.x = d_x; p.y = d_y; p.nblk = nblk; p.sxy = d_sxy; p.sxx = d_sxx; p.syy = d_syy;
        switch (nwind) {
            case 512: rc = launch_fused<4>(p, x_dtype, s); *kernels = "k_xspec_fused<512>"; break;
            case 1024: rc = launch_fused<8>(p, x_dtype, s); *kernels = "k_xspec_fused<1024>"; break;
            default: rc = launch_fused<16>(p, x_dtype, s); *kernels = "k_xspec_fused<2048>"; break;
        }
        if (rc != PVX_OK) return rc;
    } else {
        FftPlan* fp = nullptr;
        if ((rc = pvx_fbank_ensure_plan(w, nwind, &fp)) != PVX_OK) return rc;
        const int64_t batch = fp->batch;                              // spectra per rocFFT execution
        const int nsig = two ? 2 : 1;
        const int64_t ntile = (nhalf + 63) / 64;                       // waves of k_xspec_rows per block
        if (batch < nsig) { pvx_set_error("pvx_xspec: nwind %d is too long for the rows route", nwind); return PVX_ERR_UNSUPPORTED; }
        if ((rc = w.frames.grow((size_t)batch * nwind * 8, Sizing::exact)) != PVX_OK ||
            (rc = w.spec.grow((size_t)batch * nhalf * 16, Sizing::exact)) != PVX_OK) return rc;
        double* const frames = w.frames.as<double>();
        p.rows = w.spec.get(); p.ldo = nhalf;
        const int64_t rpb = (int64_t)nseg + 1;                        // k_frames' row space: a signal's row 0 is a zero frame
        const int64_t bpb = batch / (rpb * nsig);                     // whole blocks of both signals in a batch
        if (bpb >= 1) {
            p.rpb = (int)rpb; p.lead = 1; p.segn = nseg; p.first = 1; p.last = 1; p.yrow = bpb * rpb;
            for (int64_t c0 = 0; c0 < nblk; c0 += bpb) {
                const int64_t cnt = std::min(bpb, nblk - c0);
                // workspace row j of a signal = global row c0 * rpb + j (pvx_internal.h: workspace row j holds global row R0 - 1 + j)
                if ((rc = frames_of(d_x, x_dtype, es, 0, delta, nseg, c0 * rpb + 1, cnt * rpb, nblk * rpb, nwind, step, dt, frames, s)) != PVX_OK) return rc;
                if (two && (rc = frames_of(d_y, x_dtype, es, 0, delta, nseg, c0 * rpb + 1, cnt * rpb, nblk * rpb, nwind, step, dt,
                                           frames + p.yrow * nwind, s)) != PVX_OK) return rc;
                PVX_FFT_CHECK(fp->fft.execute(w.frames.get(), w.spec.get(), s));   // the whole batch: the other rows are not read
                p.nblk = cnt;
                p.sxy = two ? d_sxy + 2 * c0 * nhalf : nullptr; p.sxx = d_sxx + c0 * nhalf; p.syy = two ? d_syy + c0 * nhalf : nullptr;
                hipLaunchKernelGGL(k_xspec_rows, dim3((unsigned)((cnt * ntile + 3) / 4)), dim3(256), 0, s, p);
                PVX_HIP_CHECK(hipGetLastError());
            }
        } else {
            // a block whose segments do not fit one batch: block after block, a batch of its segments at a time (as a plain
            // signal of nseg frames: workspace row j = frame g0 + j); the sums go through the outputs between the passes
            const int64_t spb = batch / nsig;
            p.rpb = 0; p.lead = 0; p.nblk = 1; p.yrow = spb;
            for (int64_t b = 0; b < nblk; b++) {
                for (int64_t g0 = 0; g0 < nseg; g0 += spb) {
                    const int64_t cnt = std::min<int64_t>(spb, nseg - g0);
                    if ((rc = frames_of(d_x, x_dtype, es, b * delta, 0, nseg, g0 + 2, cnt, (int64_t)nseg + 1, nwind, step, dt, frames, s)) != PVX_OK) return rc;
                    if (two && (rc = frames_of(d_y, x_dtype, es, b * delta, 0, nseg, g0 + 2, cnt, (int64_t)nseg + 1, nwind, step, dt,
                                               frames + p.yrow * nwind, s)) != PVX_OK) return rc;
                    PVX_FFT_CHECK(fp->fft.execute(w.frames.get(), w.spec.get(), s));
                    p.segn = (int)cnt; p.first = g0 == 0; p.last = g0 + cnt == nseg;
                    p.sxy = two ? d_sxy + 2 * b * nhalf : nullptr; p.sxx = d_sxx + b * nhalf; p.syy = two ? d_syy + b * nhalf : nullptr;
                    hipLaunchKernelGGL(k_xspec_rows, dim3((unsigned)((ntile + 3) / 4)), dim3(256), 0, s, p);
                    PVX_HIP_CHECK(hipGetLastError());
                }
            }
        }
        *kernels = "k_frames+rocfft+k_xspec_rows";
    }
    PVX_HIP_CHECK(hipStreamSynchronize(s));
    return PVX_OK;
}

}  // namespace

int pvx_xspec_run(const void* d_x, const void* d_y, int x_dtype, const double* h_wind, int nwind, int step, int64_t delta, int64_t nblk,
                  int nseg, double* d_sxy, double* d_sxx, double* d_syy, hipStream_t s, const char** kernels) {
    if (nblk <= 0) return PVX_OK;
    FbankWs* w;
    int rc;
    if ((rc = pvx_fbank_workspace(&w)) != PVX_OK) return rc;
    std::lock_guard<std::mutex> lk(w->mu);
    return run_locked(*w, d_x, d_y, x_dtype, h_wind, nwind, step, delta, nblk, nseg, d_sxy, d_sxx, d_syy, s, kernels);
}

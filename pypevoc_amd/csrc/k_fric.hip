// k_fric.hip -- fricative descriptors of many snippets of one signal (pypevoc/speech/SpeechAnalysis.py:
// FricativeDataFromSnip :349-384): a Welch power spectrum with scipy's conventions (every segment's mean removed), the
// refined position of its maximum, the two spectral slopes either side of it, the four distribution moments and the
// snippet's RMS.  float64 throughout.  Design and numbers: FRICATIVES.md.
// Snippet r is x[starts[r] : starts[r] + L]; nper = min(nwind, L), nov = nper/2, step = nper - nov, nseg = (L - nov)/step:
//   X_s = rfft((seg_s - mean(seg_s)) * win),  psd[r][k] = c[k] (1/nseg) sum_s |X_s[k]|^2 / (sr sum(win^2)),  k = 0 .. nper/2
// with c[k] = 2 but 1 at DC and, for even nper, at the last bin.
//
// Two routes for the spectrum, as in k_xspec.hip:
//   fused  nper 512 / 1024 / 2048: k_fric_fused, the single-wave transform of pvx_stft.h exactly as k_xspec_fused runs it
//          for one signal; the wave takes the segment's mean over the 2R samples each lane holds before the window
//          multiply, |X|^2 stays in registers across the snippet's segments, the lane scales and writes the psd row once.
//   rows   any other nper: k_fric_frames (a wave per segment: mean, then (x - mean) * win) + a batched real rocFFT into the
//          workspace shared with k_fbank.hip / k_specdesc.hip / k_xspec.hip, then k_fric_acc, one bin per lane.
// The descriptors (k_fric_desc) and the RMS (k_fric_rms) are a wave per row each and read the psd row / the samples and
// nothing else.  A row is one wave's work with a fixed summation order -- a lane adds its elements l, l + 64, .. in index
// order, then wave_sum -- so the bits depend neither on the grid nor on the other rows of the call.
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

struct FrParams {
    const void* x;            // samples; snippet r starts at x[starts[r]]
    const int64_t* starts;    // [nrows]
    int64_t nrows;            // snippets of this launch
    int L;                    // samples of a snippet (k_fric_rms)
    int nper, step, nseg;     // segment length, samples between segment starts, segments of a snippet
    int nhalf;                // nper/2 + 1 bins
    int segn, seg0;           // rows route: segments of a snippet in this pass, the first of them
    int first, last;          // rows route: this pass starts the sums from zero / ends them (scales)
    const double* win;        // [nper]
    const void* twiddle;      // complex double [nper] W_nper^j (fused)
    double den;               // sr * sum(win^2)
    double* frames;           // [..][nper] (x - mean) * win (rows route)
    const void* rows;         // complex double [..][nhalf] half-spectrum rows (rows route)
    double* psd;              // [nrows][nhalf]
};

// c[k] / nseg / den applied to a bin's sum over the segments
__device__ __forceinline__ double fr_scale(double sum, int k, const FrParams& p) {
    const double v = sum / (double)p.nseg / p.den;
    const bool once = k == 0 || ((p.nper & 1) == 0 && k == p.nhalf - 1);
    return once ? v : 2.0 * v;
}

// ---- fused route -----------------------------------------------------------------------------------------------------
// Waves of a workgroup as k_xspec_fused: six at nper 512, four from 1024 on.
template <int R> constexpr int fr_waves() { return R == 4 ? 6 : 4; }

template <int R, typename InT>
__global__ __launch_bounds__(64 * fr_waves<R>()) void k_fric_fused(FrParams p) {
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

    // snippets are dealt round-robin to the waves of the grid; a wave transforms a snippet's segments one after the other.
    // The samples of the wave's next transform are prefetched in four groups spread over the current one
    const int64_t W = (int64_t)gridDim.x * nw;
    int64_t b = (int64_t)blockIdx.x * nw + wid;
    if (b >= p.nrows) return;                                         // (no workgroup barrier below)
    int s = 0;
    auto src_of = [&](int64_t bb, int ss) -> const InT* { return (const InT*)p.x + p.starts[bb] + (int64_t)ss * p.step; };
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
        const InT* s0 = src_of(b, 0);
        prefetch_part(s0, 0); prefetch_part(s0, 1); prefetch_part(s0, 2); prefetch_part(s0, 3);
    }
    constexpr int NPAIR = R / 2;
    double pxx0[NPAIR], pxx1[NPAIR], pxxH = 0.0;                      // the snippet's sums of |X|^2
#pragma unroll
    for (int j2 = 0; j2 < NPAIR; j2++) pxx0[j2] = pxx1[j2] = 0.0;
    for (;;) {
        const bool head = s == 0;
        int64_t nb = b;
        int ns = s;
        if (++ns == p.nseg) { ns = 0; nb = b + W; }
        const InT* nsrc = nb < p.nrows ? src_of(nb, ns) : nullptr;
        // the segment's mean: a lane's samples in index order, then wave_sum
        T lsum = raw[0];
#pragma unroll
        for (int i = 1; i < 2 * R; i++) lsum += raw[i];
        const T mean = wave_sum(lsum) / (T)G::N;
        cx<T> z[R];
        lds_gather_use<0, R, lds_batch<R, T>(), T>((const cx<T>*)(winL + 2 * lane), 64, [&](int r, cx<T> wv) {
            z[r] = mkc<T>((raw[2 * r] - mean) * wv.x, (raw[2 * r + 1] - mean) * wv.y);
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
        auto add = [&](cx<T> a, double& sxx) {
            const double qa = a.x * a.x + a.y * a.y;
            sxx = head ? qa : sxx + qa;
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
            add(x0, pxx0[j2]);
            add(x1, pxx1[j2]);
        }
        add(mkc<T>(zc.x, -zc.y), pxxH);                               // bin M/2 pairs with itself: X = conj Z
        if (s + 1 == p.nseg) {
            double* const o = p.psd + b * (int64_t)p.nhalf;           // nhalf = M + 1
#pragma unroll
            for (int j2 = 0; j2 < NPAIR; j2++) {
                const int k = lane + 64 * j2;
                o[k] = fr_scale(pxx0[j2], k, p);
                o[M - k] = fr_scale(pxx1[j2], M - k, p);
            }
            if (lane == 0) o[G::HALF] = fr_scale(pxxH, G::HALF, p);
        }
        if (nb >= p.nrows) break;
        b = nb; s = ns;
    }
}

// ---- rows route ------------------------------------------------------------------------------------------------------
// a wave per segment: workspace row j is segment seg0 + j % segn of snippet j / segn of this launch
template <typename InT>
__global__ __launch_bounds__(256) void k_fric_frames(FrParams p, int64_t total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t j = (int64_t)blockIdx.x * 4 + wid;
    if (j >= total) return;
    const int64_t r = j / p.segn;
    const int s = p.seg0 + (int)(j - r * p.segn);
    const InT* src = (const InT*)p.x + p.starts[r] + (int64_t)s * p.step;
    double lsum = 0.0;
    for (int i = lane; i < p.nper; i += 64) lsum += (double)src[i];
    const double mean = wave_sum(lsum) / (double)p.nper;
    double* const o = p.frames + j * (int64_t)p.nper;
    for (int i = lane; i < p.nper; i += 64) o[i] = ((double)src[i] - mean) * p.win[i];
}

// one bin per lane: a snippet's segments added in index order (a wave per snippet and 64 bins, as k_xspec_rows)
__global__ __launch_bounds__(256) void k_fric_acc(FrParams p) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int ntile = (p.nhalf + 63) / 64;
    const int64_t unit = (int64_t)blockIdx.x * 4 + wid;
    const int64_t b = unit / ntile;
    const int k = (int)(unit - b * ntile) * 64 + lane;
    if (b >= p.nrows || k >= p.nhalf) return;
    const double2* xr = (const double2*)p.rows + b * (int64_t)p.segn * p.nhalf + k;
    const int64_t o = b * (int64_t)p.nhalf + k;
    double sxx = p.first ? 0.0 : p.psd[o];
    for (int s = 0; s < p.segn; s++) {
        const double2 a = xr[(int64_t)s * p.nhalf];
        sxx += a.x * a.x + a.y * a.y;
    }
    p.psd[o] = p.last ? fr_scale(sxx, k, p) : sxx;
}

// ---- descriptors of a psd row ----------------------------------------------------------------------------------------
// S[nb], f[nb] -> d[7] = f_max, slope_left, slope_right, cent, stdev, skew, kurt; the arg-max and the status word
// (1: the maximum is at an end bin; 2: a bin that is zero, negative or not finite).  One wave; every lane returns the same
// values.  Every sum is "lane l adds bins l, l + 64, .. in index order, then wave_sum".
__device__ __forceinline__ bool fr_bad(double v) { return !(v > 0.0 && v < INFINITY); }
__device__ __forceinline__ double fr_db(double v) { return 10.0 * log10(v); }

__device__ void fric_tail(const double* S, const double* f, int nb, int lane, double* d, int* imax_out, int* status_out) {
    const double qnan = __builtin_nan("");
    // arg-max, lowest index on ties (a NaN bin never wins); bad bins
    double bv = -INFINITY;
    int bi = 0x7fffffff;
    bool bad = false;
    double m0 = 0.0, m1 = 0.0;
    for (int k = lane; k < nb; k += 64) {
        const double v = S[k];
        if (v > bv) { bv = v; bi = k; }
        bad = bad || fr_bad(v);
        m0 += v;
        m1 += v * f[k];
    }
    const double top = wave_max(bv);
    const double first = wave_min(bv == top && bi != 0x7fffffff ? (double)bi : 2147483647.0);
    const int imax = first < 2147483647.0 ? (int)first : 0;
    const bool anybad = __ballot(bad) != 0ull;
    m0 = wave_sum(m0);
    m1 = wave_sum(m1) / m0;
    // central moments; the means of the two fits
    double mu2 = 0.0, mu3 = 0.0, mu4 = 0.0, fl = 0.0, yl = 0.0, fr = 0.0, yr = 0.0;
    bool badl = false, badr = false;
    for (int k = lane; k < nb; k += 64) {
        const double v = S[k], fk = f[k];
        const double dd = fk - m1, d2 = dd * dd;
        mu2 += d2 * v;
        mu3 += d2 * dd * v;
        mu4 += d2 * d2 * v;
        const double y = fr_db(v);
        if (k <= imax) { fl += fk; yl += y; badl = badl || fr_bad(v); }
        if (k >= imax) { fr += fk; yr += y; badr = badr || fr_bad(v); }
    }
    mu2 = wave_sum(mu2) / m0; mu3 = wave_sum(mu3) / m0; mu4 = wave_sum(mu4) / m0;
    const int nl = imax + 1, nr = nb - imax;
    fl = wave_sum(fl) / (double)nl; yl = wave_sum(yl) / (double)nl;
    fr = wave_sum(fr) / (double)nr; yr = wave_sum(yr) / (double)nr;
    const bool anyl = __ballot(badl) != 0ull, anyr = __ballot(badr) != 0ull;
    // centred sums of the two fits
    double sl_xy = 0.0, sl_xx = 0.0, sr_xy = 0.0, sr_xx = 0.0;
    for (int k = lane; k < nb; k += 64) {
        const double fk = f[k], y = fr_db(S[k]);
        if (k <= imax) { const double df = fk - fl; sl_xy += df * (y - yl); sl_xx += df * df; }
        if (k >= imax) { const double df = fk - fr; sr_xy += df * (y - yr); sr_xx += df * df; }
    }
    sl_xy = wave_sum(sl_xy); sl_xx = wave_sum(sl_xx); sr_xy = wave_sum(sr_xy); sr_xx = wave_sum(sr_xx);
    // the refined position of the maximum (refine_max :26-48) and freq interpolated there
    const int pk = imax > 1 ? imax : 1;                               // <= nb - 1: nb >= 2
    double fmax;
    if (pk >= nb - 1) {
        fmax = fr_bad(S[pk]) ? qnan : f[pk];
    } else {
        const double s0 = S[pk - 1], s1 = S[pk], s2 = S[pk + 1];
        const double y0 = fr_db(s0), y1 = fr_db(s1), y2 = fr_db(s2);
        double pos = (double)pk;
        if (y1 > y0 && y1 > y2) {
            const double bq = (y2 - y0) / 2.0, aq = (y2 + y0) / 2.0 - y1;
            pos = (double)pk + (-bq / 2.0 / aq);
        }
        int j = (int)floor(pos);
        j = j < 0 ? 0 : (j > nb - 2 ? nb - 2 : j);
        const double at = pos < 0.0 ? 0.0 : (pos > (double)(nb - 1) ? (double)(nb - 1) : pos);
        fmax = (f[j + 1] - f[j]) * (at - (double)j) + f[j];
        if (fr_bad(s0) || fr_bad(s1) || fr_bad(s2) || !(pos == pos)) fmax = qnan;
    }
    const bool dead = !(m0 != 0.0);                                   // an all-zero row (or a NaN sum): nan throughout
    d[0] = dead ? qnan : fmax;
    d[1] = (dead || anyl || nl < 2) ? qnan : 1000.0 * (sl_xy / sl_xx);
    d[2] = (dead || anyr || nr < 2) ? qnan : 1000.0 * (sr_xy / sr_xx);
    d[3] = dead ? qnan : m1;
    d[4] = dead ? qnan : sqrt(mu2);
    d[5] = dead ? qnan : mu3 / (mu2 * sqrt(mu2));
    d[6] = dead ? qnan : mu4 / (mu2 * mu2) - 3.0;
    *imax_out = imax;
    *status_out = ((imax == 0 || imax == nb - 1) ? 1 : 0) | (anybad ? 2 : 0);
}

__global__ __launch_bounds__(256) void k_fric_desc(const double* psd, const double* freq, int64_t nrows, int nb, double* desc, int* imax, int* status) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * 4 + wid;
    if (r >= nrows) return;
    double d[7];
    int im, st;
    fric_tail(psd + r * (int64_t)nb, freq, nb, lane, d, &im, &st);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 7; i++) desc[r * 7 + i] = d[i];
        imax[r] = im;
        status[r] = st;
    }
}

// np.std of the snippet's L samples where they are: two passes of the lane-strided sum, population form
template <typename InT>
__global__ __launch_bounds__(256) void k_fric_rms(FrParams p, double* rms) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * 4 + wid;
    if (r >= p.nrows) return;
    const InT* src = (const InT*)p.x + p.starts[r];
    double a = 0.0;
    for (int i = lane; i < p.L; i += 64) a += (double)src[i];
    const double mean = wave_sum(a) / (double)p.L;
    double q = 0.0;
    for (int i = lane; i < p.L; i += 64) { const double dv = (double)src[i] - mean; q += dv * dv; }
    q = wave_sum(q);
    if (lane == 0) rms[r] = sqrt(q / (double)p.L);
}

template <int R> int launch_fused(const FrParams& p, int x_dtype, hipStream_t s) {
    int dev = 0, ncu = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ncu = v;
    }
    int nw = fr_waves<R>();
    while (nw > 1 && StftGeo<R, double>::total(nw) > 160 * 1024) nw--;
    const size_t lds = StftGeo<R, double>::total(nw);
    const void* fn = nullptr;
    switch (x_dtype) {
        case PVX_F32: fn = (const void*)k_fric_fused<R, float>; break;
        case PVX_F64: fn = (const void*)k_fric_fused<R, double>; break;
        case PVX_I16: fn = (const void*)k_fric_fused<R, int16_t>; break;
        default: pvx_set_error("bad x_dtype %d", x_dtype); return PVX_ERR_INVALID;
    }
    if (lds > 64 * 1024) PVX_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int per_cu = (int)((160 * 1024) / lds);                            // workgroups that fit a CU's LDS side by side
    if (per_cu < 1) per_cu = 1;
    if (per_cu * nw > 16) per_cu = 16 / nw > 0 ? 16 / nw : 1;
    { const int nb = pvx_resident_blocks(fn, 64 * nw, lds); if (nb >= 1 && nb < per_cu) per_cu = nb; }      // (registers: pvx_internal.h)
    int64_t nblocks = (int64_t)ncu * per_cu;
    const int64_t maxb = (p.nrows + nw - 1) / nw;
    if (nblocks > maxb) nblocks = maxb > 0 ? maxb : 1;
    FrParams arg = p;
    void* args[] = {&arg};
    PVX_HIP_CHECK(hipLaunchKernel(fn, dim3((unsigned)nblocks), dim3(64 * nw), args, lds, s));
    return PVX_OK;
}

const double kPiD = 3.141592653589793238462643383279502884;

bool fused_takes(int nper) {
    return (nper == 512 || nper == 1024 || nper == 2048) && getenv("PVX_FRIC_ROWS") == nullptr;
}

int launch_frames(const FrParams& p, int64_t total, int x_dtype, hipStream_t s) {
    const dim3 grid((unsigned)((total + 3) / 4)), blk(256);
    switch (x_dtype) {
        case PVX_F32: hipLaunchKernelGGL(k_fric_frames<float>, grid, blk, 0, s, p, total); break;
        case PVX_F64: hipLaunchKernelGGL(k_fric_frames<double>, grid, blk, 0, s, p, total); break;
        case PVX_I16: hipLaunchKernelGGL(k_fric_frames<int16_t>, grid, blk, 0, s, p, total); break;
        default: pvx_set_error("bad x_dtype %d", x_dtype); return PVX_ERR_INVALID;
    }
    PVX_HIP_CHECK(hipGetLastError());
    return PVX_OK;
}

int launch_rms(const FrParams& p, double* d_rms, int x_dtype, hipStream_t s) {
    const dim3 grid((unsigned)((p.nrows + 3) / 4)), blk(256);
    switch (x_dtype) {
        case PVX_F32: hipLaunchKernelGGL(k_fric_rms<float>, grid, blk, 0, s, p, d_rms); break;
        case PVX_F64: hipLaunchKernelGGL(k_fric_rms<double>, grid, blk, 0, s, p, d_rms); break;
        case PVX_I16: hipLaunchKernelGGL(k_fric_rms<int16_t>, grid, blk, 0, s, p, d_rms); break;
        default: pvx_set_error("bad x_dtype %d", x_dtype); return PVX_ERR_INVALID;
    }
    PVX_HIP_CHECK(hipGetLastError());
    return PVX_OK;
}

int run_locked(FbankWs& w, const void* d_x, int x_dtype, const int64_t* h_starts, int64_t nrows, int L, int nwind, const double* h_win,
               double sr, const double* h_freq, double* d_psd, double* d_desc, int32_t* d_imax, int32_t* d_status, double* d_rms,
               hipStream_t s, const char** kernels) {
    const int nper = std::min(nwind, L), nov = nper / 2, step = nper - nov, nseg = (L - nov) / step, nhalf = nper / 2 + 1;
    const bool spectrum = d_x != nullptr, tail = d_desc != nullptr;
    const bool fused = spectrum && fused_takes(nper);
    // the call's tables: window | twiddles (fused) | freq (descriptors)
    std::vector<double>& t = w.h_tab;
    t.clear();
    double sumw2 = 0.0;
    if (spectrum) {
        t.resize((size_t)nper);
        for (int i = 0; i < nper; i++) {
            t[i] = h_win ? h_win[i] : 0.5 - 0.5 * cos(2.0 * kPiD * i / (double)nper);    // the periodic Hann window
            sumw2 += t[i] * t[i];
        }
    }
    const size_t off_tw = t.size();
    if (fused) {
        t.resize(off_tw + 2 * (size_t)nper);
        for (int j = 0; j < nper; j++) {
            t[off_tw + 2 * j] = cos(2.0 * kPiD * j / (double)nper);
            t[off_tw + 2 * j + 1] = -sin(2.0 * kPiD * j / (double)nper);
        }
    }
    const size_t off_fr = t.size();
    if (tail) t.insert(t.end(), h_freq, h_freq + nhalf);
    int rc;
    if ((rc = w.tab.grow(t.size() * 8, Sizing::exact)) != PVX_OK) return rc;
    PVX_HIP_CHECK(hipMemcpyAsync(w.tab.get(), t.data(), t.size() * 8, hipMemcpyHostToDevice, s));
    const double* dt = w.tab.as<const double>();
    DevMem own_psd;                                                   // the descriptors read psd rows: a call that returns none keeps its own
    if (spectrum) {
        if ((rc = w.band.grow((size_t)nrows * 8, Sizing::exact)) != PVX_OK) return rc;
        PVX_HIP_CHECK(hipMemcpyAsync(w.band.get(), h_starts, (size_t)nrows * 8, hipMemcpyHostToDevice, s));
        if (!d_psd) {
            if ((rc = own_psd.alloc((size_t)nrows * nhalf * 8)) != PVX_OK) return rc;
            d_psd = own_psd.as<double>();
        }
        FrParams p = {};
        p.x = d_x; p.starts = w.band.as<const int64_t>(); p.nrows = nrows; p.L = L; p.nper = nper; p.step = step; p.nseg = nseg; p.nhalf = nhalf;
        p.win = dt; p.twiddle = dt + off_tw; p.den = sr * sumw2; p.psd = d_psd;
        if (fused) {
            switch (nper) {
                case 512: rc = launch_fused<4>(p, x_dtype, s); *kernels = tail ? "k_fric_fused<512>+k_fric_desc+k_fric_rms" : "k_fric_fused<512>"; break;
                case 1024: rc = launch_fused<8>(p, x_dtype, s); *kernels = tail ? "k_fric_fused<1024>+k_fric_desc+k_fric_rms" : "k_fric_fused<1024>"; break;
                default: rc = launch_fused<16>(p, x_dtype, s); *kernels = tail ? "k_fric_fused<2048>+k_fric_desc+k_fric_rms" : "k_fric_fused<2048>"; break;
            }
            if (rc != PVX_OK) return rc;
        } else {
            if (nper > (1 << 22)) { pvx_set_error("pvx_welch: segments of %d samples are too long for the rows route", nper); return PVX_ERR_UNSUPPORTED; }
            FftPlan* fp = nullptr;
            if ((rc = pvx_fbank_ensure_plan(w, nper, &fp)) != PVX_OK) return rc;
            const int64_t batch = fp->batch;                          // spectra per rocFFT execution
            if (batch < 1) { pvx_set_error("pvx_welch: nper %d is too long for the rows route", nper); return PVX_ERR_UNSUPPORTED; }
            if ((rc = w.frames.grow((size_t)batch * nper * 8, Sizing::exact)) != PVX_OK ||
                (rc = w.spec.grow((size_t)batch * nhalf * 16, Sizing::exact)) != PVX_OK) return rc;
            p.frames = w.frames.as<double>(); p.rows = w.spec.get();
            const int64_t ntile = (nhalf + 63) / 64;                   // waves of k_fric_acc per snippet
            const int64_t spb = batch / nseg;                         // whole snippets in a batch
            if (spb >= 1) {
                p.segn = nseg; p.seg0 = 0; p.first = 1; p.last = 1;
                for (int64_t c0 = 0; c0 < nrows; c0 += spb) {
                    const int64_t cnt = std::min(spb, nrows - c0);
                    p.starts = w.band.as<const int64_t>() + c0; p.nrows = cnt; p.psd = d_psd + c0 * nhalf;
                    if ((rc = launch_frames(p, cnt * nseg, x_dtype, s)) != PVX_OK) return rc;
                    PVX_FFT_CHECK(fp->fft.execute(w.frames.get(), w.spec.get(), s));   // the whole batch: the other rows are not read
                    hipLaunchKernelGGL(k_fric_acc, dim3((unsigned)((cnt * ntile + 3) / 4)), dim3(256), 0, s, p);
                    PVX_HIP_CHECK(hipGetLastError());
                }
            } else {
                // a snippet whose segments do not fit one batch: snippet after snippet, a batch of its segments at a time; the
                // sums go through the output row between the passes
                p.nrows = 1;
                for (int64_t b = 0; b < nrows; b++) {
                    p.starts = w.band.as<const int64_t>() + b; p.psd = d_psd + b * nhalf;
                    for (int64_t g0 = 0; g0 < nseg; g0 += batch) {
                        const int64_t cnt = std::min<int64_t>(batch, nseg - g0);
                        p.segn = (int)cnt; p.seg0 = (int)g0; p.first = g0 == 0; p.last = g0 + cnt == nseg;
                        if ((rc = launch_frames(p, cnt, x_dtype, s)) != PVX_OK) return rc;
                        PVX_FFT_CHECK(fp->fft.execute(w.frames.get(), w.spec.get(), s));
                        hipLaunchKernelGGL(k_fric_acc, dim3((unsigned)((ntile + 3) / 4)), dim3(256), 0, s, p);
                        PVX_HIP_CHECK(hipGetLastError());
                    }
                }
            }
            *kernels = tail ? "k_fric_frames+rocfft+k_fric_acc+k_fric_desc+k_fric_rms" : "k_fric_frames+rocfft+k_fric_acc";
        }
        if (tail) {
            p.starts = w.band.as<const int64_t>(); p.nrows = nrows;
            if ((rc = launch_rms(p, d_rms, x_dtype, s)) != PVX_OK) return rc;
        }
    } else {
        *kernels = "k_fric_desc";
    }
    if (tail) {
        hipLaunchKernelGGL(k_fric_desc, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, s, (const double*)d_psd, dt + off_fr, nrows, nhalf, d_desc,
                           (int*)d_imax, (int*)d_status);
        PVX_HIP_CHECK(hipGetLastError());
    }
    PVX_HIP_CHECK(hipStreamSynchronize(s));
    return PVX_OK;
}

}  // namespace

int pvx_fric_run(const void* d_x, int x_dtype, const int64_t* h_starts, int64_t nrows, int L, int nwind, const double* h_win, double sr,
                 const double* h_freq, double* d_psd, double* d_desc, int32_t* d_imax, int32_t* d_status, double* d_rms, hipStream_t s,
                 const char** kernels) {
    if (nrows <= 0) return PVX_OK;
    FbankWs* w;
    int rc;
    if ((rc = pvx_fbank_workspace(&w)) != PVX_OK) return rc;
    std::lock_guard<std::mutex> lk(w->mu);
    return run_locked(*w, d_x, x_dtype, h_starts, nrows, L, nwind, h_win, sr, h_freq, d_psd, d_desc, d_imax, d_status, d_rms, s, kernels);
}

// k_hetharm.hip -- HeterodyneHarmonic (pypevoc/Heterodyne.py:261-542): every harmonic of one f0 track in one pass.
//   extract_partial(n)          h[i] = 2 * sum_j x[i*hop+j] * exp(+i*n*phi[i*hop+j]) * wind[j] / sum(wind)      (:460-471, :35-60)
//   extract_partials()          ah[i][n] = h_n[i] for n in 0 .. nharm-1, column 0 halved                          (:521-532)
//   resynth_partial(n, filter)  y[t] = Re(conj(exp(i*n*phi[t])) * hf[t]),  hf = np.interp(t/sr, th, ah[:, n])    (:485-499)
//   filter_harmonic(n)          hf[t] = 0 where f0<fmin | f0>fmax | f0*n>sr/2.2 | |hf| < ampthr * max|hf|         (:473-483)
// with phi = cumsum(2*pi*fvec) (:391-400).  The harmonics of one track share one phase: exp(i*n*phi) is a power of
// exp(i*phi), so the signal, the window and ONE running sum are read once whatever nharm is.
//
// The running sum is kept in CYCLES (cyc = cumsum(fvec)), not radians: n * cyc is then reduced mod 1 without loss
// (p = n*cyc, e = fma(n, cyc, -p): p + e is the exact product; frac = (p - rint(p)) + e) and handed to sincospi, which
// needs no range reduction by an inexact pi.  float64 throughout.
//
// k_hh_tilesum / k_hh_tilescan / k_hh_apply: the inclusive scan in three launches (sums of PVX_HH_TILE samples, one block
//   scanning those sums, each tile scanning itself on top of its offset).  No block waits for another one inside a kernel.
// k_hh_extract: one wave64 per (frame, group of PVX_HH_GROUP harmonics).  Groups are ALIGNED (harmonics 0..7, 8..15, ..)
//   whatever `first` is, and a harmonic is always reached by the same walk from its group's first one: column n of
//   extract_partials() and extract_partial(n) are the same arithmetic, bit for bit, and so are the shared columns of two
//   nharm.  Per sample: two sincospi (z = exp(2*pi*i*g0*cyc), the step exp(2*pi*i*cyc)) and up to 7 complex rotations,
//   error O(group * 2^-52); no table.
// k_hh_ampmax / k_hh_resynth: one thread per output sample; the knot of np.interp comes from (t - wlen/2) / hop (th sits
//   on sample positions).  |linear interpolation| is convex along a segment and the ends are clamped, so max|hf| over the
//   samples is max_i |ah[i][n]|: a reduction over the nfr knots (k_hh_ampmax), not over the samples.
#include "pvx_wave.h"

using namespace pvxw;

namespace {

constexpr int kTile = PVX_HH_TILE, kPer = PVX_HH_TILE / 256, G = PVX_HH_GROUP;

__device__ __forceinline__ double wave_scan_incl(double v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const double u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    return v;
}

// exclusive prefix of v over the block's 256 threads (thread order); *total: the block's sum
__device__ __forceinline__ double block_scan_excl(double v, double* lds, double* total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const double inc = wave_scan_incl(v, lane);
    const double up = __shfl_up(inc, 1);
    if (lane == 63) lds[wid] = inc;
    __syncthreads();
    double off = 0.0, tot = 0.0;
    for (int w = 0; w < 4; w++) {
        const double t = lds[w];
        if (w < wid) off += t;
        tot += t;
    }
    __syncthreads();                                                  // lds is free for the next call
    *total = tot;
    return lane == 0 ? off : off + up;
}

__global__ __launch_bounds__(256) void k_hh_tilesum(const double* __restrict__ f, int64_t n, double* __restrict__ tsum) {
    __shared__ double lds[4];
    const int64_t base = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kPer;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kPer; k++) s += base + k < n ? f[base + k] : 0.0;
    double tot;
    (void)block_scan_excl(s, lds, &tot);
    if (threadIdx.x == 0) tsum[blockIdx.x] = tot;
}

// one block: tsum[i] <- tsum[0] + .. + tsum[i-1]
__global__ __launch_bounds__(256) void k_hh_tilescan(double* __restrict__ tsum, int64_t ntiles) {
    __shared__ double lds[4];
    double carry = 0.0;
    for (int64_t base = 0; base < ntiles; base += 256) {
        const int64_t i = base + threadIdx.x;
        const double v = i < ntiles ? tsum[i] : 0.0;
        double tot;
        const double ex = block_scan_excl(v, lds, &tot);
        if (i < ntiles) tsum[i] = carry + ex;
        carry += tot;
    }
}

__global__ __launch_bounds__(256) void k_hh_apply(const double* __restrict__ f, int64_t n, const double* __restrict__ tsum,
                                                   double* __restrict__ cyc) {
    __shared__ double lds[4];
    const int64_t base = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kPer;
    double run[kPer];
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        s += base + k < n ? f[base + k] : 0.0;
        run[k] = s;
    }
    double tot;
    const double off = tsum[blockIdx.x] + block_scan_excl(s, lds, &tot);
#pragma unroll
    for (int k = 0; k < kPer; k++)
        if (base + k < n) cyc[base + k] = off + run[k];
}

// exp(2*pi*i * m * c) for an integer-valued m: the product is reduced mod 1 exactly before sincospi sees it
__device__ __forceinline__ void cis_cycles(double m, double c, double& re, double& im) {
    const double p = m * c, e = fma(m, c, -p);
    const double fr = (p - rint(p)) + e;
    sincospi(2.0 * fr, &im, &re);
}

__global__ __launch_bounds__(256) void k_hh_extract(HhExtractParams p) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int gfirst = p.first / G, ngrp = (p.first + p.count - 1) / G - gfirst + 1;
    const int64_t w = (int64_t)blockIdx.x * nw + wid;
    const int64_t fr = w / ngrp;
    if (fr >= p.nfr) return;
    const int g0 = (gfirst + (int)(w - fr * ngrp)) * G;
    // the group's harmonics that are asked for: g0 + lo .. g0 + hi - 1 (wave-uniform)
    const int lo = p.first > g0 ? p.first - g0 : 0, hi = p.first + p.count - g0 < G ? p.first + p.count - g0 : G;
    const int64_t pos = fr * (int64_t)p.hop;
    const double* x = p.x + pos;
    const double* cyc = p.cyc + pos;
    double ar[G], ai[G];
#pragma unroll
    for (int k = 0; k < G; k++) ar[k] = ai[k] = 0.0;
    for (int j = lane; j < p.wlen; j += 64) {
        const double xw = x[j] * p.wind[j], c = cyc[j];
        double zr, zi, sr, si;
        cis_cycles((double)g0, c, zr, zi);
        cis_cycles(1.0, c, sr, si);
#pragma unroll
        for (int k = 0; k < G; k++) {
            if (k >= lo && k < hi) {
                ar[k] = fma(xw, zr, ar[k]);
                ai[k] = fma(xw, zi, ai[k]);
            }
            if (k + 1 < hi) {                                         // z^(g0+k+1) = z^(g0+k) * step
                const double nr = fma(zr, sr, -(zi * si)), ni = fma(zr, si, zi * sr);
                zr = nr; zi = ni;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < G; k++) {
        if (k >= lo && k < hi) {
            const double tr = wave_sum(ar[k]), ti = wave_sum(ai[k]);
            if (lane == 0) {
                const int h = g0 + k;
                double vr = tr / p.norm * 2.0, vi = ti / p.norm * 2.0;     // Heterodyne.py:58, 60
                if (h == 0 && p.halve_dc) { vr /= 2.0; vi /= 2.0; }        // Heterodyne.py:530
                double* o = p.ah + 2 * (fr * (int64_t)p.count + (h - p.first));
                o[0] = vr; o[1] = vi;
            }
        }
    }
    if (lane == 0 && g0 == gfirst * G && p.icent) p.icent[fr] = pos + p.wlen / 2;   // Heterodyne.py:59
}

// amax[k] = np.max(np.abs(ah[:, first + k])): one wave per harmonic
__global__ __launch_bounds__(64) void k_hh_ampmax(HhResynthParams p) {
    const int lane = threadIdx.x, k = blockIdx.x;
    const double2* a = (const double2*)p.ah + (p.first + k);
    double m = -INFINITY;
    bool nan = false;                                                // np.max propagates NaN
    for (int64_t i = lane; i < p.nfr; i += 64) {
        const double2 v = a[i * p.nharm_total];
        const double r = hypot(v.x, v.y);
        m = fmax(m, r);
        nan = nan || (r != r);
    }
    m = wave_max(m);
    if (__ballot(nan) != 0ull) m = NAN;
    if (lane == 0) p.amax[k] = m;
}

__global__ __launch_bounds__(256) void k_hh_resynth(HhResynthParams p) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= p.n) return;
    const double c = p.cyc[t];
    const double f0 = p.fvec[t] * p.sr;                               // the f0 property, Heterodyne.py:306-307
    // np.interp(t/sr, th, .): th[i] = (wlen/2 + i*hop) / sr, clamped to the end values (one knot: constant)
    const int64_t r = t - p.wlen / 2;
    int64_t i0 = 0;
    double fr = 0.0;
    if (r > 0 && p.nfr > 1) {
        i0 = r / p.hop;
        if (i0 >= p.nfr - 1) i0 = p.nfr - 1;
        else fr = (double)(r - i0 * p.hop) / (double)p.hop;
    }
    const double2* a0 = (const double2*)p.ah + i0 * p.nharm_total;
    const double2* a1 = fr != 0.0 ? a0 + p.nharm_total : a0;
    const bool band = f0 < p.fmin || f0 > p.fmax;
    const double nyq = p.sr / 2.2;
    double zr = 1.0, zi = 0.0, sr = 1.0, si = 0.0, y = 0.0;
    cis_cycles(1.0, c, sr, si);
    double2 hf = {0.0, 0.0};
    // a harmonic's carrier is reached as in k_hh_extract, by the walk from its aligned group's first one (re-anchored every G
    // harmonics: the walk's error stays O(G * 2^-52)), so resynth() is the sum of its resynth_partial(n) bit for bit
    for (int h = p.first / G * G; h < p.first + p.count; h++) {
        if ((h & (G - 1)) == 0) cis_cycles((double)h, c, zr, zi);
        else {
            const double nr = fma(zr, sr, -(zi * si)), ni = fma(zr, si, zi * sr);
            zr = nr; zi = ni;
        }
        if (h < p.first) continue;
        const int k = h - p.first;
        const double2 u = a0[h], v = a1[h];
        hf.x = u.x + (v.x - u.x) * fr;
        hf.y = u.y + (v.y - u.y) * fr;
        if (p.filter) {
            const bool cut = band || f0 * (double)h > nyq || hypot(hf.x, hf.y) < p.amax[k] * p.ampthr;   // Heterodyne.py:479-481
            if (cut) { hf.x = 0.0; hf.y = 0.0; }
        }
        y += zr * hf.x + zi * hf.y;                                   // Re(conj(hsig) * hf), Heterodyne.py:499
    }
    p.y[t] = y;
    if (p.hf) { p.hf[2 * t] = hf.x; p.hf[2 * t + 1] = hf.y; }
}

}  // namespace

int pvx_launch_hh_phase(const double* fvec, int64_t n, double* cyc, double* tsum, hipStream_t s) {
    if (n <= 0) return PVX_OK;
    const int64_t nt = pvx_hh_tiles(n);
    if (nt > 0x7fffffff) { pvx_set_error("a frequency track of %lld samples is beyond the phase scan's grid", (long long)n); return PVX_ERR_SIZE; }
    hipLaunchKernelGGL(k_hh_tilesum, dim3((unsigned)nt), dim3(256), 0, s, fvec, n, tsum);
    hipLaunchKernelGGL(k_hh_tilescan, dim3(1), dim3(256), 0, s, tsum, nt);
    hipLaunchKernelGGL(k_hh_apply, dim3((unsigned)nt), dim3(256), 0, s, fvec, n, (const double*)tsum, cyc);
    PVX_HIP_CHECK(hipGetLastError());
    return PVX_OK;
}

int pvx_launch_hh_extract(const HhExtractParams& p, hipStream_t s) {
    if (p.nfr <= 0 || p.count <= 0) return PVX_OK;
    const int ngrp = (p.first + p.count - 1) / G - p.first / G + 1;
    const int64_t nb = (p.nfr * ngrp + 3) / 4;
    if (nb > 0x7fffffff) { pvx_set_error("%lld frames of %d harmonics are beyond one launch's grid", (long long)p.nfr, p.count); return PVX_ERR_SIZE; }
    hipLaunchKernelGGL(k_hh_extract, dim3((unsigned)nb), dim3(256), 0, s, p);
    PVX_HIP_CHECK(hipGetLastError());
    return PVX_OK;
}

int pvx_launch_hh_resynth(const HhResynthParams& p, hipStream_t s) {
    if (p.n <= 0 || p.nfr <= 0 || p.count <= 0) return PVX_OK;
    const int64_t nb = (p.n + 255) / 256;
    if (nb > 0x7fffffff) { pvx_set_error("%lld samples are beyond one launch's grid", (long long)p.n); return PVX_ERR_SIZE; }
    if (p.filter) hipLaunchKernelGGL(k_hh_ampmax, dim3((unsigned)p.count), dim3(64), 0, s, p);
    hipLaunchKernelGGL(k_hh_resynth, dim3((unsigned)nb), dim3(256), 0, s, p);
    PVX_HIP_CHECK(hipGetLastError());
    return PVX_OK;
}

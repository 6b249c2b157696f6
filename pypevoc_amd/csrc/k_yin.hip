// k_yin.hip -- YIN f0 tracking (de Cheveigne & Kawahara 2002, steps 1-5): the reference's aubio_f0yin
// (pypevoc/SoundUtils.py:234-261) needs the aubio package; the algorithm here is the one YIN.md specifies.
//
// One 256-thread workgroup per frame (persistent: a workgroup walks frames fr, fr + grid, ...).
//   1. the frame xs = x[start : start + nwind] goes to LDS (float64, zero padded by kPad entries);
//   2. lanes own lags: a thread computes kR neighbouring lags d[l0 .. l0 + kR) = sum_j (xs[j] - xs[j + lag])^2 over a
//      sliding register window -- per kR samples one broadcast 32-byte read and one shifted 32-byte read for
//      kR * kR subtract + fma pairs -- for the lags 0 .. hi + 1 only.  Where the lags do not fill the workgroup
//      (nwind <= 2048) the sum over j is split into nseg <= 4 segments owned by different lanes, added in segment order;
//   3. S = prefix sum of d over the lags: per-thread runs of consecutive lags, a shuffle scan inside each wave, the
//      waves' totals in wave order; d' = d * lag / S in place;
//   4. first dip below the tolerance (block minimum of the qualifying lags) or, without one, the first arg-min
//      (block arg-max of -d' in the order value, index); parabolic refinement, frequency and confidence by thread 0.
// float64 throughout, every sum in an order fixed by (nwind, hi) alone: a frame's result does not depend on the
// workgroup, the grid, the other frames of the call or the launch.  No atomics, no global scratch.
#include <float.h>
#include <math.h>

#include <map>
#include <mutex>

#include "pvx_block.h"
#include "pvx_internal.h"
#include "pvx_mem.h"

namespace {

using namespace pvxb;

constexpr int kThreads = kBlock;
constexpr int kR = 4;              // lags per thread per pass; lag blocks and segments start at multiples of kR (16-byte LDS reads)
constexpr int kPad = 8;            // zeros behind the frame: the last lag block's window reads up to xs[nwind + 2]
constexpr int kMaxSeg = 4;
constexpr int kGridMax = 1024;
constexpr int kHeadRed = (sizeof(Red) + 7) / 8;                     // doubles the reductions' scratch takes
constexpr int kHead = (kHeadRed + kThreads / 64 + 1 + 1) / 2 * 2;   // ... + the waves' totals + S[hi + 1], kept even
static_assert(kR == 4, "lag_block reads its samples as two double2");
static_assert(sizeof(Red) % 8 == 0 && kHead % 2 == 0, "the frame starts 16-byte aligned");

// acc[r] += (xs[j] - xs[j + l0 + r])^2 for j = j0 .. j1 - 1 in ascending order; j0 and l0 are multiples of kR.
// Reads xs[j0 .. j1) and xs[j0 + l0 .. j1 + l0 + kR): the caller keeps both inside the padded frame.
__device__ __forceinline__ void lag_block(const double* xs, int j0, int j1, int l0, double (&acc)[kR]) {
    const double2* x2 = (const double2*)xs;
    double w[2 * kR];                                                // w[k] = xs[j + l0 + k]
    {
        const double2 u = x2[(j0 + l0) / 2], v = x2[(j0 + l0) / 2 + 1];
        w[0] = u.x; w[1] = u.y; w[2] = v.x; w[3] = v.y;
    }
    int j = j0;
    for (; j + kR <= j1; j += kR) {
        const double2 a0 = x2[j / 2], a1 = x2[j / 2 + 1];
        const double2 b0 = x2[(j + l0 + kR) / 2], b1 = x2[(j + l0 + kR) / 2 + 1];
        const double a[kR] = {a0.x, a0.y, a1.x, a1.y};
        w[4] = b0.x; w[5] = b0.y; w[6] = b1.x; w[7] = b1.y;
#pragma unroll
        for (int k = 0; k < kR; k++) {
#pragma unroll
            for (int r = 0; r < kR; r++) { const double d = a[k] - w[k + r]; acc[r] = fma(d, d, acc[r]); }
        }
#pragma unroll
        for (int k = 0; k < kR; k++) w[k] = w[kR + k];
    }
    for (; j < j1; j++) {                                            // at most kR - 1 samples (odd nwind / 2)
        const double a = xs[j];
#pragma unroll
        for (int r = 0; r < kR; r++) { const double d = a - xs[j + l0 + r]; acc[r] = fma(d, d, acc[r]); }
    }
}

__global__ __launch_bounds__(kThreads) void k_yin(YinParams p) {
    // all LDS is dynamic: static variables would sit in front of it unpadded and could take the frame off the 16-byte
    // alignment its double2 reads need.  [Red][wtot][s_top] fill kHead doubles, then the frame, then the lag sums.
    extern __shared__ __attribute__((aligned(16))) double lds[];
    Red& red = *(Red*)lds;
    double* wtot = lds + kHeadRed;
    double& s_top = lds[kHeadRed + kThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int n = p.nwind, L = n / 2;
    const int nl = p.hi + 2;                                         // lags 0 .. hi + 1
    const int nlp = p.nblk * kR;                                     // nl rounded up to whole lag blocks
    double* xs = lds + kHead;                                        // [n + kPad]
    double* dp = xs + (n + kPad);                                    // [nseg][nlp]: partial sums, then d, then d' in row 0
    const int C = (nl + kThreads - 1) / kThreads;                    // consecutive lags per thread in the prefix sum
    const int c0 = min(nl, t * C), c1 = min(nl, c0 + C);
    for (int64_t fr = blockIdx.x; fr < p.nfr; fr += gridDim.x) {
        const int64_t st = p.starts[fr];
        if (st < 0 || st + n > p.nsamp) {                            // the entry point checked this; never read outside x
            if (t == 0) {
                p.freq[fr] = NAN; p.conf[fr] = NAN;
                if (p.tau) p.tau[fr] = NAN;
                if (p.flag) p.flag[fr] = -1;
                if (p.pick) p.pick[fr] = -1;
            }
            continue;
        }
        for (int i = t; i < n + kPad; i += kThreads) xs[i] = i < n ? p.x[st + i] : 0.0;
        __syncthreads();

        // ---- step 1: the difference sums, a lag block and a segment of j per work item
        const int nwork = p.nblk * p.nseg;
        for (int wk = t; wk < nwork; wk += kThreads) {
            const int sg = wk / p.nblk, blk = wk - sg * p.nblk;
            const int j0 = sg * p.seglen, j1 = min(L, j0 + p.seglen);
            double acc[kR] = {0.0, 0.0, 0.0, 0.0};
            if (j0 < L) lag_block(xs, j0, j1, blk * kR, acc);
            double* o = dp + sg * nlp + blk * kR;
#pragma unroll
            for (int r = 0; r < kR; r++) o[r] = acc[r];
        }
        __syncthreads();

        // ---- step 2: d (segments in order), S (prefix sum), d' in place
        double local = 0.0;
        for (int k = c0; k < c1; k++) {
            double d = 0.0;
            if (k > 0) {
                d = dp[k];
                for (int sg = 1; sg < p.nseg; sg++) d += dp[sg * nlp + k];
            }
            dp[k] = d;
            local += d;
        }
        double v = local;
        for (int o = 1; o < 64; o <<= 1) { const double u = __shfl_up(v, o); if (lane >= o) v += u; }
        double excl = __shfl_up(v, 1);
        if (lane == 0) excl = 0.0;
        if (lane == 63) wtot[wv] = v;
        __syncthreads();
        double run = 0.0;
        for (int q = 0; q < wv; q++) run += wtot[q];
        run += excl;
        for (int k = c0; k < c1; k++) {
            const double d = dp[k];
            run += d;                                                // S[k]
            dp[k] = k == 0 ? 1.0 : (run != 0.0 ? d * (double)k / run : 1.0);
            if (k == p.hi + 1) s_top = run;
        }
        __syncthreads();

        // ---- steps 3, 4: the first dip below the tolerance, else the first arg-min
        int first = INT_MAX;
        for (int k = p.lo + t; k <= p.hi; k += kThreads)
            if (dp[k] < p.tol && dp[k] < dp[k + 1]) first = min(first, k);
        first = block_imin(first, red);
        int flag = 0, pick = first;
        if (first == INT_MAX) {                                      // block-uniform
            flag = 1;
            double bs = -INFINITY;
            int bk = INT_MAX;
            for (int k = p.lo + t; k <= p.hi; k += kThreads) { const double s = -dp[k]; if (better(s, k, bs, bk)) { bs = s; bk = k; } }
            block_argmax(bs, bk, red);
            pick = bk;
        }

        // ---- steps 5, 6
        if (t == 0) {
            double tf = 0.0, freq = 0.0, conf = 0.0;
            if (s_top == 0.0 || pick == INT_MAX) {                   // silent or constant frame (INT_MAX: NaN samples)
                flag = 2; pick = 0;
            } else {
                const double s0 = dp[pick - 1], s1 = dp[pick], s2 = dp[pick + 1];
                const double den = s0 - 2.0 * s1 + s2;
                tf = den != 0.0 ? (double)pick + 0.5 * (s0 - s2) / den : (double)pick;
                freq = p.sr / tf;
                conf = 1.0 - s1;
            }
            p.freq[fr] = freq;
            p.conf[fr] = conf;
            if (p.tau) p.tau[fr] = tf;
            if (p.flag) p.flag[fr] = flag;
            if (p.pick) p.pick[fr] = pick;
        }
        __syncthreads();                                             // thread 0 read d': the next frame overwrites it
    }
}

// the frame starts of a call, kept per device for the process (grow-only; calls on one device take turns)
struct YinWs {
    std::mutex mu;
    DevMem starts;
};
std::mutex g_ws_mu;
std::map<int, YinWs*> g_ws;                                          // device -> workspace (never erased)

}  // namespace

int pvx_yin_run(YinParams p, const int64_t* h_starts, hipStream_t s, const char** kernels) {
    *kernels = "";
    if (p.nfr <= 0) return PVX_OK;
    int dev = 0;
    PVX_HIP_CHECK(hipGetDevice(&dev));
    YinWs* w;
    {
        std::lock_guard<std::mutex> lk(g_ws_mu);
        YinWs*& e = g_ws[dev];
        if (!e) e = new YinWs();
        w = e;
    }
    std::lock_guard<std::mutex> lk(w->mu);
    int rc;
    if ((rc = w->starts.grow((size_t)p.nfr * 8, Sizing::headroom)) != PVX_OK) return rc;
    PVX_HIP_CHECK(hipMemcpyAsync(w->starts.get(), h_starts, (size_t)p.nfr * 8, hipMemcpyHostToDevice, s));
    p.starts = w->starts.as<const int64_t>();
    // the split: lag blocks of kR lags; while they leave half of the workgroup idle, twice as many segments of j
    const int L = p.nwind / 2;
    p.nblk = (p.hi + 2 + kR - 1) / kR;
    p.nseg = 1;
    while (p.nseg < kMaxSeg && p.nblk * p.nseg * 2 <= kThreads) p.nseg *= 2;
    p.seglen = ((L + p.nseg - 1) / p.nseg + kR - 1) / kR * kR;
    const size_t lds = ((size_t)(kHead + p.nwind + kPad) + (size_t)p.nseg * p.nblk * kR) * 8;
    if (lds > 64 * 1024) PVX_HIP_CHECK(hipFuncSetAttribute((const void*)k_yin, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned grid = (unsigned)(p.nfr < kGridMax ? p.nfr : kGridMax);
    hipLaunchKernelGGL(k_yin, dim3(grid), dim3(kThreads), lds, s, p);
    PVX_HIP_CHECK(hipGetLastError());
    PVX_HIP_CHECK(hipStreamSynchronize(s));                          // the workspace is free for the next call from here on
    *kernels = p.nseg == 1 ? "k_yin" : (p.nseg == 2 ? "k_yin/seg2" : "k_yin/seg4");
    return PVX_OK;
}

// pvx_lpc.h -- workgroup-level linear prediction in float64 (pypevoc/speech/SpeechAnalysis.py:9-24: np.correlate's lags
// 0 .. p and scipy's solve_toeplitz), for kernels that run one 256-thread workgroup per frame (k_iaif.hip; a later
// formant kernel).  Device only; design and bounds: GLOTTAL.md.
//
//   lpc_autocorr   r[k] = sum_i v[i+k] v[i], k = 0 .. p, of an LDS-resident vector v[0..n)
//   lpc_levinson   a = [1, a_1 .. a_p] with toeplitz(r[:p]) a[1:] = -r[1:], and a status
//
// Every sum has one order whatever the grid: lag k belongs to wave k % 4, lane l of it adds the products i = l, l + 64,
// ... in ascending i, and the 64 partial sums meet in the xor butterfly below.  The recursion runs on wave 0 alone, its
// vector in LDS, the other waves waiting at the barrier that ends it.  All threads of the workgroup call both functions
// with the same arguments; both end with a barrier, so their results are visible to every thread afterwards.
#pragma once
#include <hip/hip_runtime.h>

#include "pvx.h"

namespace pvxlpc {

constexpr int kThreads = 256;
static_assert(PVX_LPC_MAX_ORDER <= 128, "lpc_levinson updates two coefficients per lane");

struct Work {
    double r[PVX_LPC_MAX_ORDER + 1];
    double a[PVX_LPC_MAX_ORDER + 1];
    int status;
};

// LDS hand-off between the lanes of one wave: its LDS operations execute in order, the compiler must not move them across
__device__ __forceinline__ void wave_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// the same bits in every lane: a pair of lanes adds the same two numbers
__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the caller has made v visible to the workgroup (a barrier after its last write)
__device__ inline void lpc_autocorr(const double* v, int n, int p, Work& w) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int k = wave; k <= p; k += kThreads / 64) {
        double s = 0.0;
        for (int i = lane; i + k < n; i += 64) s = fma(v[i + k], v[i], s);
        s = wave_sum(s);
        if (lane == 0) w.r[k] = s;
    }
    __syncthreads();
}

// Levinson-Durbin on w.r[0..p] into w.a[0..p].  Returns 0, or the step 1 .. p that met a prediction error of exactly 0
// (step 1: r[0] == 0, a silent frame); w.a is then unfinished.  The value is the same in every thread.
__device__ inline int lpc_levinson(Work& w, int p) {
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        double err = w.r[0];
        int st = 0;
        if (lane == 0) w.a[0] = 1.0;
        for (int i = 1; i <= p; i++) {
            if (err == 0.0) { st = i; break; }                       // (wave-uniform: err has the same bits in every lane)
            double s = 0.0;
            for (int j = 1 + lane; j < i; j += 64) s = fma(w.a[j], w.r[i - j], s);
            s = wave_sum(s);
            const double k = -(w.r[i] + s) / err;
            const int j0 = 1 + lane, j1 = 65 + lane;                 // j < i <= 128
            double n0 = 0.0, n1 = 0.0;
            if (j0 < i) n0 = fma(k, w.a[i - j0], w.a[j0]);
            if (j1 < i) n1 = fma(k, w.a[i - j1], w.a[j1]);
            wave_sync();                                             // every lane has read the old vector
            if (j0 < i) w.a[j0] = n0;
            if (j1 < i) w.a[j1] = n1;
            if (lane == 0) w.a[i] = k;
            wave_sync();
            err = err * (1.0 - k * k);
        }
        if (lane == 0) w.status = st;
    }
    __syncthreads();
    return w.status;
}

}  // namespace pvxlpc

// pvx_block.h -- reductions over one 256-thread workgroup, shared by the frame-per-workgroup kernels (k_period.hip,
// k_yin.hip).  Every one has a fixed order -- xor butterflies inside a wave, then the four waves' values in index order --
// so a result does not depend on which workgroup runs a frame.  Each takes the workgroup's `Red` scratch in LDS and
// synchronises the workgroup (twice); all threads must call it.
#pragma once
#include <limits.h>
#include <math.h>

#include <hip/hip_runtime.h>

namespace pvxb {

constexpr int kBlock = 256;

struct Red {
    double d[kBlock / 64];
    int i[kBlock / 64];
};

inline __device__ double block_sum(double v, Red& r) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) r.d[w] = v;
    __syncthreads();
    return (r.d[0] + r.d[1]) + (r.d[2] + r.d[3]);
}
// max ignoring NaN (fmax); -inf when every value is NaN / absent
inline __device__ double block_fmax(double v, Red& r) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) r.d[w] = v;
    __syncthreads();
    return fmax(fmax(r.d[0], r.d[1]), fmax(r.d[2], r.d[3]));
}
// numpy's np.min: NaN as soon as one value is NaN
inline __device__ double block_nanmin(double v, Red& r) {
    for (int o = 32; o > 0; o >>= 1) {
        const double u = __shfl_xor(v, o);
        v = (v != v || u != u) ? NAN : (u < v ? u : v);
    }
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) r.d[w] = v;
    __syncthreads();
    double m = r.d[0];
    for (int k = 1; k < kBlock / 64; k++) { const double u = r.d[k]; m = (m != m || u != u) ? NAN : (u < m ? u : m); }
    return m;
}
inline __device__ int block_imin(int v, Red& r) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) r.i[w] = v;
    __syncthreads();
    return min(min(r.i[0], r.i[1]), min(r.i[2], r.i[3]));
}
// (score desc, index asc): the first arg-max of a repeated argmax(); with negated scores, the first arg-min
__device__ __forceinline__ bool better(double s, int k, double s2, int k2) { return s > s2 || (s == s2 && k < k2); }
inline __device__ void block_argmax(double& s, int& k, Red& r) {
    for (int o = 32; o > 0; o >>= 1) {
        const double s2 = __shfl_xor(s, o);
        const int k2 = __shfl_xor(k, o);
        if (better(s2, k2, s, k)) { s = s2; k = k2; }
    }
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { r.d[w] = s; r.i[w] = k; }
    __syncthreads();
    s = r.d[0]; k = r.i[0];
    for (int q = 1; q < kBlock / 64; q++) if (better(r.d[q], r.i[q], s, k)) { s = r.d[q]; k = r.i[q]; }
}

}  // namespace pvxb

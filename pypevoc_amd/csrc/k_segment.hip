// k_segment.hip -- SpeechSegmenter's device half (pypevoc/speech/SpeechSegmenter.py: process :203-222, the parabolic fit
// :224-260, refine_segment_all_bands :262-302, refine_transition_points :39-124) on band energies that a filter bank left in
// device memory.  float64 throughout, no fused multiply-add (the library is built with -ffp-contract=off), no atomics, every
// sum in numpy's own order.  Design: SEGMENT.md.
//
// k_seg_detect: det[i] = sum_b |10 log10 spec[i+1][b] - 10 log10 spec[i][b]|, its strict peaks above the threshold and their
//   parabolic positions, ascending and left-packed.  ONE workgroup walks the table in tiles of kDetTile det values -- an
//   ordered pass, so the running count of the peaks before a tile is a register, not a message between workgroups.  A tile
//   reads kDetTile + 1 rows (one halo row), kDetChunk bands at a time: every thread takes the logs of its row's chunk into LDS
//   once, then adds the chunk's |differences| against the row below in band order.  The sum follows np.sum of a row: bands
//   before nband - nband % 8 go to eight accumulators by band % 8, these are added as a tree, the remaining bands one by one
//   (fewer than 8 bands: one by one from 0.0).  A tile's det values go to LDS behind the last two of the tile before; the
//   peak test runs one index behind, so index i is tested when det[i+1] exists and every index is tested once.  Peak flags
//   are a ballot per wave, the waves' counts a prefix in LDS.
// k_seg_refine: one workgroup per segment, its waves take the bands in turn: one wave64 per (segment, band).  The wave loads
//   the dB values of its iall range into LDS once, takes the medians of the two sides by rank counting (pvx_select.h), scans
//   the range for sign changes against valm, lane by lane, and picks the one nearest to len(ibef) by a wave-wide arg-min on
//   (distance, index): the earlier of two equally near ones.  After a workgroup barrier one lane adds the bands' pk * w and w
//   in np.sum's order and divides.
// k_seg_transitions: one wave64 (and workgroup) per series of up to PVX_SEG_MAX_SERIES points in LDS: the typical values
//   before and after trt by mode (order statistics by the same rank counting, min / max by wave reduction, the mean in
//   np.sum's pairwise order), the crossings of the level between them and the one nearest to trt in time.
// Reads are clamped to the tables whatever the ranges and the data hold.
#include <math.h>
#include <stdint.h>

#include <map>
#include <mutex>

#include "pvx_internal.h"
#include "pvx_mem.h"
#include "pvx_select.h"

namespace {

using namespace pvxsel;
static_assert(PVX_SEG_MAX_SERIES <= kNpSumMaxRun, "np_sum's stacks (pvx_select.h) are sized for runs of up to kNpSumMaxRun terms");

// ---- k_seg_detect -------------------------------------------------------------------------------------------------------
constexpr int kDetTile = 512, kDetChunk = 8, kDetWaves = kDetTile / 64;

struct DetectParams {
    const double* spec;         // [nfr][nband] energies
    int64_t nfr;
    int nband, maxseg;
    double thresh;
    double* det;                // [nfr - 1] or null
    int* idx;                   // [maxseg] or null
    double* fpos;               // [maxseg] or null
    long long* count;           // the full number of kept peaks
};

__global__ __launch_bounds__(kDetTile) void k_seg_detect(DetectParams p) {
    __shared__ double L[kDetTile + 1][kDetChunk + 1];                // the logs of a chunk of bands of the tile's rows
    __shared__ double D[kDetTile + 2];                               // det[f0 - 2], det[f0 - 1], then the tile's
    __shared__ int wcnt[kDetWaves];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, B = p.nband;
    const int64_t nd = p.nfr - 1;
    const int nfull = B >= 8 ? B - B % 8 : 0;                        // bands that go through the eight accumulators
    long long base = 0;                                              // peaks kept before this tile (the same in every thread)
    if (t < 2) D[t] = 0.0;
    for (int64_t f0 = 0; f0 < nd; f0 += kDetTile) {
        const int ntile = (int)(nd - f0 < kDetTile ? nd - f0 : kDetTile);
        double r[8], res = 0.0;
#pragma unroll
        for (int j = 0; j < 8; j++) r[j] = 0.0;
        for (int b0 = 0; b0 < B; b0 += kDetChunk) {
            const int nb = B - b0 < kDetChunk ? B - b0 : kDetChunk;
            for (int s = t; s <= ntile; s += kDetTile) {             // rows f0 .. f0 + ntile: thread 0 takes the halo row too
                const double* row = p.spec + (f0 + s) * B + b0;      // f0 + s <= nd = nfr - 1
                for (int j = 0; j < nb; j++) L[s][j] = 10.0 * log10(row[j]);
            }
            __syncthreads();
            if (t < ntile) {
                if (b0 < nfull) {                                    // a whole chunk of accumulator bands (nfull is a multiple of 8)
#pragma unroll
                    for (int j = 0; j < 8; j++) r[j] += fabs(L[t + 1][j] - L[t][j]);
                } else {
                    if (b0 == nfull && nfull > 0) res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
                    for (int j = 0; j < nb; j++) res += fabs(L[t + 1][j] - L[t][j]);
                }
            }
            __syncthreads();
        }
        if (nfull == B) res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        res = 0.0 + res;
        if (t < ntile) {
            D[t + 2] = res;
            if (p.det) p.det[f0 + t] = res;
        }
        __syncthreads();
        // index c = f0 + t - 1 has both neighbours now
        const int64_t c = f0 + t - 1;
        bool pk = false;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        if (t < ntile && c >= 1 && c <= nd - 2) {
            s0 = D[t]; s1 = D[t + 1]; s2 = D[t + 2];
            pk = s0 < s1 && s2 < s1 && s1 > p.thresh;
        }
        const unsigned long long bal = __ballot(pk);
        if (lane == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        long long before = base;
        int total = 0;
#pragma unroll
        for (int w = 0; w < kDetWaves; w++) {
            const int cw = wcnt[w];
            before += w < wave ? cw : 0;
            total += cw;
        }
        if (pk) {
            const long long at = before + __popcll(bal & ((1ull << lane) - 1ull));
            if (at < p.maxseg) {
                const double cc = s1;
                const double b = (s2 - s0) / 2.0;
                const double a = (s2 + s0) / 2.0 - cc;
                const double lpos = -b / 2.0 / a;
                if (p.idx) p.idx[at] = (int)c;
                if (p.fpos) p.fpos[at] = (double)c + lpos;
            }
        }
        base += total;
        const double c0 = D[ntile], c1 = D[ntile + 1];               // the tile's last two (a short tile is the last one)
        __syncthreads();
        if (t == 0) { D[0] = c0; D[1] = c1; }
        __syncthreads();
    }
    if (t == 0) *p.count = base;
}

// ---- k_seg_refine -------------------------------------------------------------------------------------------------------
constexpr int kRefWaves = 4, kRefThreads = kRefWaves * 64;
constexpr int kMaxAll = 2 * PVX_SEG_MAX_SIDE + 1;                    // both sides and the frame between them

struct RefineParams {
    const double* spec;         // [nfine][nband] energies
    int64_t nfine;
    int nband;
    const int* ranges;          // [nseg][6]: ibef, iaft, iall as [first, last + 1)
    const double* tseg;         // [nseg]
    int hop;
    double half, tsr, sr, thr;  // tfine[k] = (k hop + half) / tsr
    int has_thr;
    double *valb, *vala;        // [nseg][nband]
    int* cross;                 // [nseg][nband]
    double* out;                // [nseg]
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(kRefThreads) void k_seg_refine(RefineParams p) {
    __shared__ double f[kRefWaves][kMaxAll + 3];
    __shared__ double mid[kRefWaves][4];
    __shared__ double pkw[2][PVX_FBANK_MAX_NBAND];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, B = p.nband;
    const int64_t seg = blockIdx.x;
    const int* rg = p.ranges + seg * 6;
    const int nfine = (int)p.nfine;
    // iall inside the table and no longer than the buffer, the sides inside iall
    const int l0 = clampi(rg[4], 0, nfine), l1 = clampi(rg[5], l0, l0 + kMaxAll < nfine ? l0 + kMaxAll : nfine);
    const int b0 = clampi(rg[0], l0, l1), b1 = clampi(rg[1], b0, l1), a0 = clampi(rg[2], l0, l1), a1 = clampi(rg[3], a0, l1);
    const int L = l1 - l0, nb = b1 - b0, na = a1 - a0;
    const double tseg = p.tseg[seg];
    double* fw = f[wave];
    for (int b = wave; b < B; b += kRefWaves) {                      // (wave-uniform)
        for (int k = lane; k < L; k += 64) fw[k] = 10.0 * log10(p.spec[(int64_t)(l0 + k) * B + b]);
        lds_sync();
        const double* xb = fw + (b0 - l0);
        const double* xa = fw + (a0 - l0);
        const bool nanb = wave_any_nan(xb, nb, lane), nana = wave_any_nan(xa, na, lane);
        if (!nanb) { const int want[2] = {(nb - 1) / 2, nb / 2}; select_ranks(xb, nb, want, mid[wave], lane); }
        if (!nana) { const int want[2] = {(na - 1) / 2, na / 2}; select_ranks(xa, na, want, mid[wave] + 2, lane); }
        lds_sync();
        const double valb = nanb ? NAN : median_of(mid[wave][0], mid[wave][1], nb);
        const double vala = nana ? NAN : median_of(mid[wave][2], mid[wave][3], na);
        double valm;
        if (!p.has_thr) valm = (valb + vala) / 2.0;
        else valm = (vala != vala || valb != valb) ? NAN : (vala < valb ? vala : valb) + p.thr;   // np.min hands a NaN on
        double key = INFINITY;
        int at = 0x7fffffff;
        for (int k = lane; k < L - 1; k += 64) {
            if ((fw[k] - valm) * (fw[k + 1] - valm) < 0.0) {
                const double d = fabs((double)(k - nb));
                if (d < key) { key = d; at = k; }                    // (a lane's k ascend: the first of equals stays)
            }
        }
        wave_argmin(key, at);
        const int cr = key < INFINITY ? at : -1;
        double pk = tseg;                                            // no crossing: seconds among samples, as the reference has it
        if (cr >= 0) pk = ((double)((int64_t)(cr + b0) * p.hop) + p.half) / p.tsr * p.sr;
        const double w = fabs(valb - vala);
        if (lane == 0) {
            const int64_t o = seg * B + b;
            if (p.valb) p.valb[o] = valb;
            if (p.vala) p.vala[o] = vala;
            if (p.cross) p.cross[o] = cr;
            pkw[0][b] = pk * w;
            pkw[1][b] = w;
        }
        lds_sync();                                                  // fw and mid are rewritten by the next band
    }
    __syncthreads();
    if (threadIdx.x == 0 && p.out) {
        const double* num = pkw[0];
        const double* den = pkw[1];
        const double sn = 0.0 + np_block_sum([num](int i) { return num[i]; }, 0, B);
        const double sd = 0.0 + np_block_sum([den](int i) { return den[i]; }, 0, B);
        p.out[seg] = sn / sd;
    }
}

// ---- k_seg_transitions --------------------------------------------------------------------------------------------------
struct TransParams {
    const double* v;            // series s: v[s * row_stride + k * elem_stride], k < n
    int64_t nser, row_stride, elem_stride;
    int n;
    double escale;              // > 0: v holds energies, x = 10 log10(v escale); 0: x = v
    const double* tx;           // [n], or [nser][n] with tx_stride = n
    int64_t tx_stride;
    const double* trt;          // [nser]
    int mode;
    double pct, thr;
    double *ttr, *vbef, *vaft;  // [nser]
    int* status;                // [nser]
};

__global__ __launch_bounds__(64) void k_seg_transitions(TransParams p) {
    __shared__ double x[PVX_SEG_MAX_SERIES];
    __shared__ double sel[12];
    const int lane = threadIdx.x, n = p.n;
    const int64_t s = blockIdx.x;
    const double* tx = p.tx + s * p.tx_stride;
    const double trt = p.trt[s];
    if (trt > tx[n - 1] || trt < tx[0]) {                            // (wave-uniform) :69-70
        if (lane == 0) { p.ttr[s] = trt; p.vbef[s] = 0.0; p.vaft[s] = 0.0; p.status[s] = PVX_SEG_OUTSIDE; }
        return;
    }
    const double* v = p.v + s * p.row_stride;
    int below = 0, above = 0;
    for (int k = lane; k < n; k += 64) {
        const double e = v[(int64_t)k * p.elem_stride];
        x[k] = p.escale > 0.0 ? 10.0 * log10(e * p.escale) : e;
        below += tx[k] < trt ? 1 : 0;
        above += tx[k] > trt ? 1 : 0;
    }
    lds_sync();
    const int nb = wave_sum(below), na = wave_sum(above);            // tx ascends: x[:nb] before, x[n - na:] after
    const double* xb = x;
    const double* xa = x + (n - na);
    const bool order = p.mode != PVX_SEG_MEAN;
    if (na == 0 || ((p.mode == PVX_SEG_MINMAX || p.mode == PVX_SEG_PCT) && nb == 0)) {
        if (lane == 0) { p.ttr[s] = NAN; p.vbef[s] = NAN; p.vaft[s] = NAN; p.status[s] = PVX_SEG_EMPTY_SIDE; }
        return;
    }
    const bool nanb = wave_any_nan(xb, nb, lane), nana = wave_any_nan(xa, na, lane);
    double vbef = NAN, vaft = NAN;
    if (order) {
        // places: the two of the median, the two of percentile pct, the two of percentile 100 - pct
        const PctPlan bl = pct_plan(nb, p.pct), bh = pct_plan(nb, 100.0 - p.pct);
        const PctPlan al = pct_plan(na, p.pct), ah = pct_plan(na, 100.0 - p.pct);
        const bool pc = p.mode == PVX_SEG_PCT;
        if (!nanb) {
            const int want[6] = {(nb - 1) / 2, nb / 2, pc ? bl.prev : -1, pc ? bl.next : -1, pc ? bh.prev : -1, pc ? bh.next : -1};
            select_ranks(xb, nb, want, sel, lane);
        }
        if (!nana) {
            const int want[6] = {(na - 1) / 2, na / 2, pc ? al.prev : -1, pc ? al.next : -1, pc ? ah.prev : -1, pc ? ah.next : -1};
            select_ranks(xa, na, want, sel + 6, lane);
        }
        lds_sync();
        const double medb = nanb ? NAN : median_of(sel[0], sel[1], nb), meda = nana ? NAN : median_of(sel[6], sel[7], na);
        if (p.mode == PVX_SEG_MEDIAN) {
            vbef = medb; vaft = meda;
        } else if (p.mode == PVX_SEG_MINMAX) {
            double bmn, bmx, amn, amx;
            wave_minmax(xb, nb, lane, &bmn, &bmx);
            wave_minmax(xa, na, lane, &amn, &amx);
            const bool falls = medb > meda;                          // :79 (false with a NaN median)
            vbef = nanb ? NAN : (falls ? bmx : bmn);
            vaft = nana ? NAN : (falls ? amn : amx);
        } else {
            const bool falls = medb > meda;                          // :87
            vbef = nanb ? NAN : (falls ? pct_value(sel[4], sel[5], bh.t) : pct_value(sel[2], sel[3], bl.t));
            vaft = nana ? NAN : (falls ? pct_value(sel[8], sel[9], al.t) : pct_value(sel[10], sel[11], ah.t));
        }
    } else {
        // np.mean: np.sum's order.  Every lane walks both sides (LDS broadcasts: the time of one lane) and holds the result, so
        // nothing is handed over and the walk's control flow is the wave's; an empty side gives 0.0 / 0 = NaN, as np.mean does
        vbef = np_sum([xb](int i) { return xb[i]; }, nb) / (double)nb;
        vaft = np_sum([xa](int i) { return xa[i]; }, na) / (double)na;
    }
    const bool rises = vaft > vbef;                                  // :100
    const double vtran = rises ? vbef * p.thr + vaft * (1.0 - p.thr) : vaft * p.thr + vbef * (1.0 - p.thr);
    double key = INFINITY;
    int at = 0x7fffffff;
    for (int k = lane; k < n - 1; k += 64) {
        const bool hit = rises ? (x[k] < vtran && x[k + 1] > vtran) : (x[k] > vtran && x[k + 1] < vtran);
        if (hit) {
            const double d = fabs((tx[k] + tx[k + 1]) / 2.0 - trt);
            if (d < key) { key = d; at = k; }
        }
    }
    wave_argmin(key, at);
    if (lane == 0) {
        p.vbef[s] = vbef; p.vaft[s] = vaft;
        if (key < INFINITY) {
            p.ttr[s] = tx[at] + (tx[at + 1] - tx[at]) * (vtran - x[at]) / (x[at + 1] - x[at]);
            p.status[s] = PVX_SEG_OK;
        } else {
            p.ttr[s] = NAN;
            p.status[s] = PVX_SEG_NO_CROSSING;
        }
    }
}

// ---- host side: launches on device tables -------------------------------------------------------------------------------
// Per-device staging of the small host tables (ranges, times) and the peak count, kept for the process (grow-only); a call
// holds the mutex until its stream is synchronised.
struct SegWs {
    std::mutex mu;
    DevMem count, a, b;
};
std::mutex g_ws_mu;
std::map<int, SegWs*> g_ws;                                          // device -> workspace (never erased)

int workspace(SegWs** out) {
    int dev = 0;
    PVX_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_ws_mu);
    SegWs*& e = g_ws[dev];
    if (!e) e = new SegWs();
    *out = e;
    return PVX_OK;
}

}  // namespace

int pvx_seg_detect_run(const double* d_spec, int64_t nfr, int nband, double thresh, int maxseg, double* d_det, int* d_idx, double* d_fpos,
                       int64_t* count, hipStream_t s, const char** kernels) {
    *count = 0;
    if (nfr < 2) return PVX_OK;                                      // no det value: nothing to launch
    SegWs* w;
    int rc;
    if ((rc = workspace(&w)) != PVX_OK) return rc;
    std::lock_guard<std::mutex> lk(w->mu);
    if ((rc = w->count.grow(8, Sizing::exact)) != PVX_OK) return rc;
    DetectParams p = {};
    p.spec = d_spec; p.nfr = nfr; p.nband = nband; p.maxseg = maxseg; p.thresh = thresh;
    p.det = d_det; p.idx = d_idx; p.fpos = d_fpos; p.count = w->count.as<long long>();
    hipLaunchKernelGGL(k_seg_detect, dim3(1), dim3(kDetTile), 0, s, p);
    PVX_HIP_CHECK(hipGetLastError());
    *kernels = "k_seg_detect";
    long long h = 0;
    PVX_HIP_CHECK(hipMemcpyAsync(&h, w->count.get(), 8, hipMemcpyDeviceToHost, s));
    PVX_HIP_CHECK(hipStreamSynchronize(s));
    *count = h;
    return PVX_OK;
}

int pvx_seg_refine_run(const double* d_spec, int64_t nfine, int nband, const int32_t* h_ranges, const double* h_tseg, int64_t nseg, int hop,
                       double half, double tsr, double sr, double thr, int has_thr, double* d_valb, double* d_vala, int* d_cross,
                       double* d_out, hipStream_t s, const char** kernels) {
    if (nseg <= 0) return PVX_OK;
    SegWs* w;
    int rc;
    if ((rc = workspace(&w)) != PVX_OK) return rc;
    std::lock_guard<std::mutex> lk(w->mu);
    if ((rc = w->a.grow((size_t)nseg * 24, Sizing::headroom)) != PVX_OK || (rc = w->b.grow((size_t)nseg * 8, Sizing::headroom)) != PVX_OK) return rc;
    PVX_HIP_CHECK(hipMemcpyAsync(w->a.get(), h_ranges, (size_t)nseg * 24, hipMemcpyHostToDevice, s));
    PVX_HIP_CHECK(hipMemcpyAsync(w->b.get(), h_tseg, (size_t)nseg * 8, hipMemcpyHostToDevice, s));
    RefineParams p = {};
    p.spec = d_spec; p.nfine = nfine; p.nband = nband; p.ranges = w->a.as<int>(); p.tseg = w->b.as<double>(); p.hop = hop;
    p.half = half; p.tsr = tsr; p.sr = sr; p.thr = thr; p.has_thr = has_thr;
    p.valb = d_valb; p.vala = d_vala; p.cross = d_cross; p.out = d_out;
    hipLaunchKernelGGL(k_seg_refine, dim3((unsigned)nseg), dim3(kRefThreads), 0, s, p);
    PVX_HIP_CHECK(hipGetLastError());
    *kernels = "k_seg_refine";
    PVX_HIP_CHECK(hipStreamSynchronize(s));
    return PVX_OK;
}

int pvx_seg_transitions_run(const double* d_v, int64_t nser, int n, int64_t row_stride, int64_t elem_stride, double escale,
                            const double* h_tx, int64_t tx_stride, const double* h_trt, int mode, double pct, double thr, double* d_ttr,
                            double* d_vbef, double* d_vaft, int* d_status, hipStream_t s, const char** kernels) {
    if (nser <= 0) return PVX_OK;
    const size_t ntx = tx_stride ? (size_t)nser * n : (size_t)n;
    SegWs* w;
    int rc;
    if ((rc = workspace(&w)) != PVX_OK) return rc;
    std::lock_guard<std::mutex> lk(w->mu);
    if ((rc = w->a.grow(ntx * 8, Sizing::headroom)) != PVX_OK || (rc = w->b.grow((size_t)nser * 8, Sizing::headroom)) != PVX_OK) return rc;
    PVX_HIP_CHECK(hipMemcpyAsync(w->a.get(), h_tx, ntx * 8, hipMemcpyHostToDevice, s));
    PVX_HIP_CHECK(hipMemcpyAsync(w->b.get(), h_trt, (size_t)nser * 8, hipMemcpyHostToDevice, s));
    TransParams p = {};
    p.v = d_v; p.nser = nser; p.row_stride = row_stride; p.elem_stride = elem_stride; p.n = n; p.escale = escale;
    p.tx = w->a.as<double>(); p.tx_stride = tx_stride ? n : 0; p.trt = w->b.as<double>(); p.mode = mode; p.pct = pct; p.thr = thr;
    p.ttr = d_ttr; p.vbef = d_vbef; p.vaft = d_vaft; p.status = d_status;
    hipLaunchKernelGGL(k_seg_transitions, dim3((unsigned)nser), dim3(64), 0, s, p);
    PVX_HIP_CHECK(hipGetLastError());
    *kernels = "k_seg_transitions";
    PVX_HIP_CHECK(hipStreamSynchronize(s));
    return PVX_OK;
}

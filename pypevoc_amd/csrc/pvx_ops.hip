// pvx_ops.hip -- host side of the entry points of include/pvx.h that take arrays, not a pvx_plan: a `_dev` form on the caller's
// device arrays and stream, and a host form that stages host arrays through pvx_api.hip's copies (pvx_host.h).
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "pvx_host.h"

// ---- windowed reductions with the analysis framing (Heterodyne.py:35-60, SoundUtils.py:71-103) ----
static int reduce_args(int64_t n, const double* wind, int wlen, int hop, double* norm, int power) {
    if (n < 0 || wlen <= 0 || hop <= 0 || !wind) { pvx_set_error("bad windowed-reduction argument"); return PVX_ERR_INVALID; }
    double s = 0.0;
    for (int i = 0; i < wlen; i++) s += power == 2 ? wind[i] * wind[i] : wind[i];
    *norm = s;
    return PVX_OK;
}

// what the `_dev` reductions share: the window on the device, the launch on `s`, and the synchronisation after which the
// window's buffer may go
template <typename Launch> static int reduce_with_window(ReduceParams& rp, const double* wind, hipStream_t s, Launch launch) {
    DevMem dw;
    int rc;
    if ((rc = dw.alloc((size_t)rp.wlen * 8)) != PVX_OK) return rc;
    PVX_HIP_CHECK(hipMemcpy(dw.get(), wind, (size_t)rp.wlen * 8, hipMemcpyHostToDevice));
    rp.wind = dw.as<const double>();
    if ((rc = launch(rp, s)) != PVX_OK) return rc;
    PVX_HIP_CHECK(hipStreamSynchronize(s));
    return PVX_OK;
}

extern "C" int64_t pvx_heterodyne_dev(const double* d_x, const double* d_hetsig, int64_t n, const double* wind, int wlen, int hop,
                                      double* d_out, int64_t* d_icent, void* stream) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    double norm;
    if ((rc = reduce_args(n, wind, wlen, hop, &norm, 1)) != PVX_OK) return rc;
    const int64_t nfr = pvx_nframes(n, wlen, hop);
    if (nfr == 0) return 0;
    if (!d_x || !d_hetsig || !d_out) { pvx_set_error("null heterodyne array"); return PVX_ERR_INVALID; }
    ReduceParams rp = {};
    rp.x = d_x; rp.hetsig = d_hetsig; rp.nfr = nfr; rp.wlen = wlen; rp.hop = hop;
    rp.norm = norm; rp.out = d_out; rp.icent = d_icent;
    rc = reduce_with_window(rp, wind, (hipStream_t)stream, [](const ReduceParams& q, hipStream_t s) { return pvx_launch_reduce(q, 0, s); });
    return rc == PVX_OK ? nfr : rc;
}

extern "C" int64_t pvx_heterodyne(const double* x, const double* hetsig, int64_t n, const double* wind, int wlen, int hop,
                                  double* out, int64_t* icent) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    double norm;
    if ((rc = reduce_args(n, wind, wlen, hop, &norm, 1)) != PVX_OK) return rc;
    const int64_t nfr = pvx_nframes(n, wlen, hop);
    if (nfr == 0) return 0;
    if (!x || !hetsig || !out) { pvx_set_error("null heterodyne array"); return PVX_ERR_INVALID; }
    Staged dx, dh, dout, dic;
    if ((rc = dout.room((size_t)nfr * 16)) != PVX_OK || (icent && (rc = dic.room((size_t)nfr * 8)) != PVX_OK) ||
        (rc = dx.put(x, (size_t)n * 8)) != PVX_OK || (rc = dh.put(hetsig, (size_t)n * 16)) != PVX_OK) return rc;
    const int64_t r = pvx_heterodyne_dev(dx.as<double>(), dh.as<double>(), n, wind, wlen, hop, dout.as<double>(), dic.as<int64_t>(), nullptr);
    if (r < 0) return r;
    if ((rc = dout.get(out, (size_t)nfr * 16)) != PVX_OK || (icent && (rc = dic.get(icent, (size_t)nfr * 8)) != PVX_OK)) return rc;
    return nfr;
}

extern "C" int64_t pvx_rms_frames_dev(const double* d_x, int64_t n, const double* wind, int wlen, int hop, double* d_out,
                                      void* stream) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    double norm;
    if ((rc = reduce_args(n, wind, wlen, hop, &norm, 2)) != PVX_OK) return rc;
    const int64_t nfr = pvx_nframes(n, wlen, hop);
    if (nfr == 0) return 0;
    if (!d_x || !d_out) { pvx_set_error("null rms array"); return PVX_ERR_INVALID; }
    ReduceParams rp = {};
    rp.x = d_x; rp.nfr = nfr; rp.wlen = wlen; rp.hop = hop; rp.norm = norm; rp.out = d_out;
    rc = reduce_with_window(rp, wind, (hipStream_t)stream, [](const ReduceParams& q, hipStream_t s) { return pvx_launch_reduce(q, 1, s); });
    return rc == PVX_OK ? nfr : rc;
}

extern "C" int64_t pvx_rms_frames(const double* x, int64_t n, const double* wind, int wlen, int hop, double* out) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    double norm;
    if ((rc = reduce_args(n, wind, wlen, hop, &norm, 2)) != PVX_OK) return rc;
    const int64_t nfr = pvx_nframes(n, wlen, hop);
    if (nfr == 0) return 0;
    if (!x || !out) { pvx_set_error("null rms array"); return PVX_ERR_INVALID; }
    Staged dx, dout;
    if ((rc = dout.room((size_t)nfr * 8)) != PVX_OK || (rc = dx.put(x, (size_t)n * 8)) != PVX_OK) return rc;
    const int64_t r = pvx_rms_frames_dev(dx.as<double>(), n, wind, wlen, hop, dout.as<double>(), nullptr);
    if (r < 0) return r;
    if ((rc = dout.get(out, (size_t)nfr * 8)) != PVX_OK) return rc;
    return nfr;
}

// FuncWind's named reducers (SoundUtils.py:42-69)
static int funcwind_args(int x_complex, int64_t n, const double* wind, int wlen, int hop, int func, double divisor) {
    if (n < 0 || wlen <= 0 || hop <= 0 || !wind) { pvx_set_error("bad windowed-reduction argument"); return PVX_ERR_INVALID; }
    if (func < PVX_FW_SUM || func > PVX_FW_VAR) { pvx_set_error("pvx_funcwind: unknown reducer %d", func); return PVX_ERR_INVALID; }
    if (!(divisor == divisor) || divisor == 0.0) { pvx_set_error("pvx_funcwind: divisor %g", divisor); return PVX_ERR_INVALID; }
    if (x_complex && (func == PVX_FW_MAX || func == PVX_FW_MIN)) { pvx_set_error("pvx_funcwind: max / min of complex frames"); return PVX_ERR_UNSUPPORTED; }
    return PVX_OK;
}

extern "C" int64_t pvx_funcwind_dev(const double* d_x, int x_complex, int64_t n, const double* wind, int wlen, int hop, int func, double divisor,
                                    double* d_out, void* stream) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    if ((rc = funcwind_args(x_complex, n, wind, wlen, hop, func, divisor)) != PVX_OK) return rc;
    const int64_t nfr = pvx_nframes(n, wlen, hop);
    if (nfr == 0) return 0;
    if (!d_x || !d_out) { pvx_set_error("null funcwind array"); return PVX_ERR_INVALID; }
    ReduceParams rp = {};
    rp.x = d_x; rp.nfr = nfr; rp.wlen = wlen; rp.hop = hop; rp.norm = divisor; rp.out = d_out;
    rc = reduce_with_window(rp, wind, (hipStream_t)stream,
                            [&](const ReduceParams& q, hipStream_t s) { return pvx_launch_funcwind(q, func, x_complex != 0, s); });
    return rc == PVX_OK ? nfr : rc;
}

extern "C" int64_t pvx_funcwind(const double* x, int x_complex, int64_t n, const double* wind, int wlen, int hop, int func, double divisor, double* out) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    if ((rc = funcwind_args(x_complex, n, wind, wlen, hop, func, divisor)) != PVX_OK) return rc;
    const int64_t nfr = pvx_nframes(n, wlen, hop);
    if (nfr == 0) return 0;
    if (!x || !out) { pvx_set_error("null funcwind array"); return PVX_ERR_INVALID; }
    const size_t xb = (size_t)n * (x_complex ? 16 : 8);
    const size_t ob = (size_t)nfr * ((x_complex && (func == PVX_FW_SUM || func == PVX_FW_MEAN)) ? 16 : 8);
    Staged dx, dout;
    if ((rc = dout.room(ob)) != PVX_OK || (rc = dx.put(x, xb)) != PVX_OK) return rc;
    const int64_t r = pvx_funcwind_dev(dx.as<double>(), x_complex, n, wind, wlen, hop, func, divisor, dout.as<double>(), nullptr);
    if (r < 0) return r;
    if ((rc = dout.get(out, ob)) != PVX_OK) return rc;
    return nfr;
}

// ---- harmonic heterodyne on one f0 track (k_hetharm.hip, Heterodyne.py:261-542) -----------------
static int hetharm_args(int64_t n, const double* wind, int wlen, int hop, int first, int count, double* norm) {
    int rc;
    if ((rc = reduce_args(n, wind, wlen, hop, norm, 1)) != PVX_OK) return rc;
    if (first < 0 || count < 1 || (int64_t)first + count > PVX_HH_MAX_HARM) {
        pvx_set_error("pvx_hetharm: harmonics %d .. %lld (first >= 0, count >= 1, up to %d)", first, (long long)first + count - 1, PVX_HH_MAX_HARM);
        return PVX_ERR_INVALID;
    }
    return PVX_OK;
}

// the running phase of d_fvec in a workspace of this call: cyc [n] and the scan's tile sums behind it
static int hetharm_phase(const double* d_fvec, int64_t n, DevMem& ws, hipStream_t s) {
    int rc;
    if ((rc = ws.alloc(((size_t)n + (size_t)pvx_hh_tiles(n)) * 8)) != PVX_OK) return rc;
    return pvx_launch_hh_phase(d_fvec, n, ws.as<double>(), ws.as<double>() + n, s);
}

extern "C" int64_t pvx_hetharm_dev(const double* d_x, int64_t n, const double* d_fvec, const double* wind, int wlen, int hop, int first,
                                   int count, int halve_dc, double* d_ah, int64_t* d_icent, void* stream) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    double norm;
    if ((rc = hetharm_args(n, wind, wlen, hop, first, count, &norm)) != PVX_OK) return rc;
    const int64_t nfr = pvx_nframes(n, wlen, hop);
    if (nfr == 0) return 0;
    if (!d_x || !d_fvec || !d_ah) { pvx_set_error("null hetharm array"); return PVX_ERR_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    DevMem dw, ws;
    if ((rc = dw.alloc((size_t)wlen * 8)) != PVX_OK) return rc;
    PVX_HIP_CHECK(hipMemcpy(dw.get(), wind, (size_t)wlen * 8, hipMemcpyHostToDevice));
    if ((rc = hetharm_phase(d_fvec, n, ws, s)) != PVX_OK) return rc;
    HhExtractParams ep = {};
    ep.x = d_x; ep.cyc = ws.as<const double>(); ep.wind = dw.as<const double>(); ep.nfr = nfr; ep.wlen = wlen; ep.hop = hop;
    ep.first = first; ep.count = count; ep.halve_dc = halve_dc ? 1 : 0; ep.norm = norm; ep.ah = d_ah; ep.icent = d_icent;
    rc = pvx_launch_hh_extract(ep, s);
    PVX_HIP_CHECK(hipStreamSynchronize(s));                           // the workspaces go with this call
    return rc == PVX_OK ? nfr : rc;
}

extern "C" int64_t pvx_hetharm(const double* x, int64_t n, const double* fvec, const double* wind, int wlen, int hop, int first, int count,
                               int halve_dc, double* ah, int64_t* icent) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    double norm;
    if ((rc = hetharm_args(n, wind, wlen, hop, first, count, &norm)) != PVX_OK) return rc;
    const int64_t nfr = pvx_nframes(n, wlen, hop);
    if (nfr == 0) return 0;
    if (!x || !fvec || !ah) { pvx_set_error("null hetharm array"); return PVX_ERR_INVALID; }
    const size_t ab = (size_t)nfr * count * 16;
    Staged dx, df, da, dic;
    if ((rc = da.room(ab)) != PVX_OK || (icent && (rc = dic.room((size_t)nfr * 8)) != PVX_OK) || (rc = dx.put(x, (size_t)n * 8)) != PVX_OK ||
        (rc = df.put(fvec, (size_t)n * 8)) != PVX_OK) return rc;
    const int64_t r = pvx_hetharm_dev(dx.as<double>(), n, df.as<double>(), wind, wlen, hop, first, count, halve_dc, da.as<double>(), dic.as<int64_t>(),
                                      nullptr);
    if (r < 0) return r;
    if ((rc = da.get(ah, ab)) != PVX_OK || (icent && (rc = dic.get(icent, (size_t)nfr * 8)) != PVX_OK)) return rc;
    return nfr;
}

static int hetharm_resynth_args(int64_t n, int64_t nfr, int nharm_total, int wlen, int hop, int first, int count, int want_hf) {
    if (n < 0 || wlen <= 0 || hop <= 0 || nharm_total < 1) { pvx_set_error("bad harmonic-resynthesis argument"); return PVX_ERR_INVALID; }
    if (first < 0 || count < 1 || (int64_t)first + count > nharm_total || nharm_total > PVX_HH_MAX_HARM) {
        pvx_set_error("pvx_hetharm_resynth: harmonics %d .. %lld of %d", first, (long long)first + count - 1, nharm_total);
        return PVX_ERR_INVALID;
    }
    if (nfr != pvx_nframes(n, wlen, hop)) {
        pvx_set_error("pvx_hetharm_resynth: %lld frames, %lld samples at window %d / hop %d have %lld", (long long)nfr, (long long)n, wlen, hop,
                      (long long)pvx_nframes(n, wlen, hop));
        return PVX_ERR_SIZE;
    }
    if (want_hf && count != 1) { pvx_set_error("pvx_hetharm_resynth: the interpolated amplitude is one harmonic's (count %d)", count); return PVX_ERR_INVALID; }
    return PVX_OK;
}

extern "C" int64_t pvx_hetharm_resynth_dev(const double* d_fvec, int64_t n, const double* d_ah, int64_t nfr, int nharm_total, int wlen, int hop,
                                           int first, int count, int filter, double sr, double fmin, double fmax, double ampthr, double* d_y,
                                           double* d_hf, void* stream) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    if ((rc = hetharm_resynth_args(n, nfr, nharm_total, wlen, hop, first, count, d_hf != nullptr)) != PVX_OK) return rc;
    if (nfr == 0) return 0;
    if (!d_fvec || !d_ah || !d_y) { pvx_set_error("null harmonic-resynthesis array"); return PVX_ERR_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    DevMem ws, dmax;
    if ((rc = hetharm_phase(d_fvec, n, ws, s)) != PVX_OK) return rc;
    if (filter && (rc = dmax.alloc((size_t)count * 8)) != PVX_OK) return rc;
    HhResynthParams rp = {};
    rp.fvec = d_fvec; rp.cyc = ws.as<const double>(); rp.ah = d_ah; rp.n = n; rp.nfr = nfr; rp.nharm_total = nharm_total; rp.wlen = wlen;
    rp.hop = hop; rp.first = first; rp.count = count; rp.filter = filter ? 1 : 0; rp.sr = sr; rp.fmin = fmin; rp.fmax = fmax; rp.ampthr = ampthr;
    rp.amax = dmax.as<double>(); rp.y = d_y; rp.hf = d_hf;
    rc = pvx_launch_hh_resynth(rp, s);
    PVX_HIP_CHECK(hipStreamSynchronize(s));
    return rc == PVX_OK ? n : rc;
}

extern "C" int64_t pvx_hetharm_resynth(const double* fvec, int64_t n, const double* ah, int64_t nfr, int nharm_total, int wlen, int hop, int first,
                                       int count, int filter, double sr, double fmin, double fmax, double ampthr, double* y, double* hf) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    if ((rc = hetharm_resynth_args(n, nfr, nharm_total, wlen, hop, first, count, hf != nullptr)) != PVX_OK) return rc;
    if (nfr == 0) return 0;
    if (!fvec || !ah || !y) { pvx_set_error("null harmonic-resynthesis array"); return PVX_ERR_INVALID; }
    const size_t ab = (size_t)nfr * nharm_total * 16;
    Staged df, da, dy, dh;
    if ((rc = dy.room((size_t)n * 8)) != PVX_OK || (hf && (rc = dh.room((size_t)n * 16)) != PVX_OK) || (rc = df.put(fvec, (size_t)n * 8)) != PVX_OK ||
        (rc = da.put(ah, ab)) != PVX_OK) return rc;
    const int64_t r = pvx_hetharm_resynth_dev(df.as<double>(), n, da.as<double>(), nfr, nharm_total, wlen, hop, first, count, filter, sr,
                                              fmin, fmax, ampthr, dy.as<double>(), dh.as<double>(), nullptr);
    if (r < 0) return r;
    if ((rc = dy.get(y, (size_t)n * 8)) != PVX_OK || (hf && (rc = dh.get(hf, (size_t)n * 16)) != PVX_OK)) return rc;
    return n;
}

// ---- time-domain periodicity (k_period.hip) ---------------------------------------------------
// numpy's clipping of a slice bound on an array of `len` entries
static int np_bound(int64_t b, int64_t len) {
    if (b < 0) b += len;
    return (int)(b < 0 ? 0 : (b > len ? len : b));
}
static int period_args(int64_t nsamp, const double* wind, int nwind, const int64_t* idx, int64_t nidx, int method, int cand_method,
                       int mindelay, int maxdelay, int ncand, PeriodParams* p) {
    if (nsamp < 0 || !wind || nwind < 1 || nidx < 0 || (nidx > 0 && !idx)) { pvx_set_error("bad periodicity argument"); return PVX_ERR_INVALID; }
    if (method != PVX_PERIOD_XCORR && method != PVX_PERIOD_AMDF) { pvx_set_error("pvx_periodicity: unknown method %d", method); return PVX_ERR_INVALID; }
    if (cand_method < PVX_CAND_FFT || cand_method > PVX_CAND_OTHER) { pvx_set_error("pvx_periodicity: unknown cand_method %d", cand_method); return PVX_ERR_INVALID; }
    if (mindelay < 0) { pvx_set_error("pvx_periodicity: mindelay %d < 0", mindelay); return PVX_ERR_INVALID; }
    if (ncand < 1 || ncand > PVX_PERIOD_MAX_NCAND) { pvx_set_error("pvx_periodicity: ncand %d outside 1..%d", ncand, PVX_PERIOD_MAX_NCAND); return PVX_ERR_UNSUPPORTED; }
    if (nwind > PVX_PERIOD_MAX_NWIND) { pvx_set_error("pvx_periodicity: window of %d samples (the kernels take up to %d)", nwind, PVX_PERIOD_MAX_NWIND); return PVX_ERR_UNSUPPORTED; }
    const int64_t n = nwind, nwl = n / 2;
    for (int64_t i = 0; i < nidx; i++) {
        if (idx[i] - nwl < 0 || idx[i] - nwl + n > nsamp) {
            pvx_set_error("pvx_periodicity: the frame centred at %lld leaves the signal of %lld samples (window %d)", (long long)idx[i], (long long)nsamp, nwind);
            return PVX_ERR_INVALID;
        }
    }
    const int64_t len = method == PVX_PERIOD_AMDF ? n : 2 * n - 1;   // amdf(xw) has nwind entries, correlate(.., "full") 2*nwind-1
    p->ns = np_bound(n - 1 - (int64_t)maxdelay, len);
    p->ne = np_bound(n - 1 + (int64_t)maxdelay, len);
    if (p->ns >= p->ne) { pvx_set_error("pvx_periodicity: maxdelay %d leaves the normalising slice empty (the reference raises ValueError)", maxdelay); return PVX_ERR_INVALID; }
    const int pend = (int)std::min<int64_t>(std::max(maxdelay, 0), n);
    if (method == PVX_PERIOD_AMDF) {
        p->lo[0] = std::min(mindelay, pend); p->hi[0] = pend;
        p->lo[1] = p->ns; p->hi[1] = p->ne;
    } else {
        const int64_t nmax = std::max(std::llabs((int64_t)p->ns - (n - 1)), std::llabs((int64_t)p->ne - 1 - (n - 1)));
        p->lo[0] = 0; p->hi[0] = (int)std::min<int64_t>(n, std::max<int64_t>(pend, nmax + 1));
        p->lo[1] = 0; p->hi[1] = 0;
    }
    p->nsamp = nsamp; p->nwind = nwind; p->nfr = nidx;
    p->amdf = method == PVX_PERIOD_AMDF; p->cand_method = cand_method;
    p->mindelay = mindelay; p->maxdelay = maxdelay; p->ncand = ncand;
    return PVX_OK;
}

extern "C" int64_t pvx_periodicity_dev(const double* d_x, int64_t nsamp, const double* wind, int nwind, const int64_t* idx, int64_t nidx,
                                       int method, int cand_method, int mindelay, int maxdelay, double threshold, double vthresh, int ncand,
                                       double fftthresh, double* d_cand_period, double* d_cand_strength, int32_t* d_ncands,
                                       int32_t* d_preferred, void* stream) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    PeriodParams p = {};
    if ((rc = period_args(nsamp, wind, nwind, idx, nidx, method, cand_method, mindelay, maxdelay, ncand, &p)) != PVX_OK) return rc;
    if (nidx == 0) return 0;
    if (!d_x || !d_cand_period || !d_cand_strength || !d_ncands || !d_preferred) { pvx_set_error("null periodicity array"); return PVX_ERR_INVALID; }
    p.x = d_x;
    p.threshold = threshold; p.vthresh = vthresh; p.fftthresh = fftthresh;
    p.cand_period = d_cand_period; p.cand_strength = d_cand_strength; p.ncands = d_ncands; p.preferred = d_preferred;
    if ((rc = pvx_period_run(p, wind, idx, (hipStream_t)stream)) != PVX_OK) return rc;   // synchronises the stream
    return nidx;
}

extern "C" int64_t pvx_periodicity(const double* x, int64_t nsamp, const double* wind, int nwind, const int64_t* idx, int64_t nidx,
                                   int method, int cand_method, int mindelay, int maxdelay, double threshold, double vthresh, int ncand,
                                   double fftthresh, double* cand_period, double* cand_strength, int32_t* ncands, int32_t* preferred) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    PeriodParams chk = {};
    if ((rc = period_args(nsamp, wind, nwind, idx, nidx, method, cand_method, mindelay, maxdelay, ncand, &chk)) != PVX_OK) return rc;
    if (nidx == 0) return 0;
    if (!x || !cand_period || !cand_strength || !ncands || !preferred) { pvx_set_error("null periodicity array"); return PVX_ERR_INVALID; }
    const size_t cb = (size_t)nidx * ncand * 8, ib = (size_t)nidx * 4;
    Staged dx, dp, ds, dn, dq;
    if ((rc = dp.room(cb)) != PVX_OK || (rc = ds.room(cb)) != PVX_OK || (rc = dn.room(ib)) != PVX_OK || (rc = dq.room(ib)) != PVX_OK ||
        (rc = dx.put(x, (size_t)nsamp * 8)) != PVX_OK) return rc;
    const int64_t r = pvx_periodicity_dev(dx.as<double>(), nsamp, wind, nwind, idx, nidx, method, cand_method, mindelay, maxdelay, threshold,
                                          vthresh, ncand, fftthresh, dp.as<double>(), ds.as<double>(), dn.as<int32_t>(), dq.as<int32_t>(), nullptr);
    if (r < 0) return r;
    if ((rc = dp.get(cand_period, cb)) != PVX_OK || (rc = ds.get(cand_strength, cb)) != PVX_OK || (rc = dn.get(ncands, ib)) != PVX_OK ||
        (rc = dq.get(preferred, ib)) != PVX_OK) return rc;
    return nidx;
}

// ---- YIN f0 tracking (k_yin.hip) --------------------------------------------------------------
static thread_local const char* t_yin_kernels = "";
extern "C" const char* pvx_yin_last_kernels(void) { return t_yin_kernels; }

static int yin_args(int64_t nsamp, const int64_t* starts, int64_t nfr, int nwind, int lo, int hi, double tol, double sr) {
    if (nsamp < 0 || nfr < 0 || (nfr > 0 && !starts)) { pvx_set_error("bad pvx_yin argument"); return PVX_ERR_INVALID; }
    if (nwind < 8) { pvx_set_error("pvx_yin: window of %d samples (at least 8 are needed)", nwind); return PVX_ERR_INVALID; }
    if (nwind > PVX_YIN_MAX_NWIND) { pvx_set_error("pvx_yin: window of %d samples (the kernel takes up to %d)", nwind, PVX_YIN_MAX_NWIND); return PVX_ERR_UNSUPPORTED; }
    if (lo < 2 || lo > hi || hi > nwind / 2 - 2) {
        pvx_set_error("pvx_yin: lags %d .. %d are not inside 2 .. nwind/2 - 2 = %d", lo, hi, nwind / 2 - 2);
        return PVX_ERR_INVALID;
    }
    if (!(tol == tol) || !(sr > 0.0)) { pvx_set_error("pvx_yin: tolerance %g, sample rate %g", tol, sr); return PVX_ERR_INVALID; }
    for (int64_t i = 0; i < nfr; i++) {
        if (starts[i] < 0 || starts[i] > nsamp - nwind) {
            pvx_set_error("pvx_yin: frame %lld (samples %lld .. %lld) does not lie inside the %lld samples of the signal", (long long)i,
                          (long long)starts[i], (long long)starts[i] + nwind, (long long)nsamp);
            return PVX_ERR_INVALID;
        }
    }
    return PVX_OK;
}

extern "C" int64_t pvx_yin_dev(const double* d_x, int64_t nsamp, const int64_t* starts, int64_t nfr, int nwind, int lo, int hi, double tol,
                               double sr, double* d_freq, double* d_conf, double* d_tau, int32_t* d_flag, int32_t* d_pick, void* stream) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    if ((rc = yin_args(nsamp, starts, nfr, nwind, lo, hi, tol, sr)) != PVX_OK) return rc;
    t_yin_kernels = "";
    if (nfr == 0) return 0;
    if (!d_x || !d_freq || !d_conf) { pvx_set_error("null pvx_yin array"); return PVX_ERR_INVALID; }
    YinParams p = {};
    p.x = d_x; p.nsamp = nsamp; p.nfr = nfr;
    p.nwind = nwind; p.lo = lo; p.hi = hi; p.tol = tol; p.sr = sr;
    p.freq = d_freq; p.conf = d_conf; p.tau = d_tau; p.flag = d_flag; p.pick = d_pick;
    if ((rc = pvx_yin_run(p, starts, (hipStream_t)stream, &t_yin_kernels)) != PVX_OK) return rc;   // synchronises the stream
    return nfr;
}

extern "C" int64_t pvx_yin(const double* x, int64_t nsamp, const int64_t* starts, int64_t nfr, int nwind, int lo, int hi, double tol, double sr,
                           double* freq, double* conf, double* tau, int32_t* flag, int32_t* pick) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    if ((rc = yin_args(nsamp, starts, nfr, nwind, lo, hi, tol, sr)) != PVX_OK) return rc;
    t_yin_kernels = "";
    if (nfr == 0) return 0;
    if (!x || !freq || !conf) { pvx_set_error("null pvx_yin array"); return PVX_ERR_INVALID; }
    const size_t db = (size_t)nfr * 8, ib = (size_t)nfr * 4;
    Staged dx, df, dc, dt, dg, dk;
    if ((rc = df.room(db)) != PVX_OK || (rc = dc.room(db)) != PVX_OK || (tau && (rc = dt.room(db)) != PVX_OK) ||
        (flag && (rc = dg.room(ib)) != PVX_OK) || (pick && (rc = dk.room(ib)) != PVX_OK) || (rc = dx.put(x, (size_t)nsamp * 8)) != PVX_OK) return rc;
    const int64_t r = pvx_yin_dev(dx.as<double>(), nsamp, starts, nfr, nwind, lo, hi, tol, sr, df.as<double>(), dc.as<double>(),
                                  dt.as<double>(), dg.as<int32_t>(), dk.as<int32_t>(), nullptr);
    if (r < 0) return r;
    if ((rc = df.get(freq, db)) != PVX_OK || (rc = dc.get(conf, db)) != PVX_OK || (tau && (rc = dt.get(tau, db)) != PVX_OK) ||
        (flag && (rc = dg.get(flag, ib)) != PVX_OK) || (pick && (rc = dk.get(pick, ib)) != PVX_OK)) return rc;
    return nfr;
}

// ---- Period marks (k_marks.hip) ----------------------------------------------------------------
static thread_local const char* t_marks_kernels = "";
extern "C" const char* pvx_marks_last_kernels(void) { return t_marks_kernels; }

static int marks_args(const char* who, int64_t nsamp, const int64_t* row_start, const int64_t* row_stop, int64_t nrows, double sr,
                      int64_t max_marks, int64_t max_steps) {
    if (nsamp < 0 || nrows < 0 || (nrows > 0 && (!row_start || !row_stop))) { pvx_set_error("bad %s argument", who); return PVX_ERR_INVALID; }
    if (!(sr > 0.0) || !(sr < INFINITY)) { pvx_set_error("%s: sample rate %g", who, sr); return PVX_ERR_INVALID; }
    if (max_marks < 1 || max_marks > INT32_MAX || max_steps < 0) {
        pvx_set_error("%s: max_marks %lld, max_steps %lld", who, (long long)max_marks, (long long)max_steps);
        return PVX_ERR_INVALID;
    }
    for (int64_t i = 0; i < nrows; i++) {
        if (row_start[i] < 0 || row_start[i] > row_stop[i] || row_stop[i] > nsamp) {
            pvx_set_error("%s: row %lld (samples %lld .. %lld) does not lie inside the %lld samples of the signal", who, (long long)i,
                          (long long)row_start[i], (long long)row_stop[i], (long long)nsamp);
            return PVX_ERR_INVALID;
        }
    }
    return PVX_OK;
}
static int marks_track(const char* who, const double* tf, const double* f, int64_t ntf) {
    if (!tf || !f || ntf < 1 || ntf > INT32_MAX) { pvx_set_error("%s: a track of %lld knots", who, (long long)ntf); return PVX_ERR_INVALID; }
    for (int64_t i = 0; i < ntf; i++) {
        if (!(tf[i] - tf[i] == 0.0) || (i > 0 && !(tf[i] > tf[i - 1]))) {
            pvx_set_error("%s: tf must be finite and strictly increasing (knot %lld)", who, (long long)i);
            return PVX_ERR_INVALID;
        }
    }
    return PVX_OK;
}

// the LDS plan of the corr walk: *cap doubles for a step's stretch, from the largest period the track can give
static int marks_corr_plan(const double* f, int64_t ntf, double f_fallback, double sr, int window, int* cap) {
    double fmin = INFINITY;
    for (int64_t i = 0; i <= ntf; i++) {
        const double v = i < ntf ? f[i] : f_fallback;
        if (v > 0.0 && v < fmin) fmin = v;
    }
    const double q = fmin < INFINITY ? sr / fmin : 0.0;
    if (window > PVX_MARKS_CORR_MAX_LDS || !(3.0 * window + floor(q) <= (double)PVX_MARKS_CORR_MAX_LDS)) {
        pvx_set_error("pvx_marks_corr: window %d with periods of up to %.0f samples (3 * window + period may be %d at most)", window,
                      floor(q), PVX_MARKS_CORR_MAX_LDS);
        return PVX_ERR_UNSUPPORTED;
    }
    *cap = (window + (int)q + 2 + 1) / 2 * 2;                         // one more than Pmax: interp may round below the smallest knot
    return PVX_OK;
}

extern "C" int64_t pvx_marks_corr_dev(const double* d_x, int64_t nsamp, const int64_t* row_start, const int64_t* row_stop, const double* t0,
                                      const double* toff, int64_t nrows, const double* tf, const double* f, int64_t ntf, double f_fallback,
                                      double sr, int window, double min_per, int64_t max_marks, int64_t max_steps, double* d_marks,
                                      int32_t* d_count, int32_t* d_status, void* stream) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    if ((rc = marks_args("pvx_marks_corr", nsamp, row_start, row_stop, nrows, sr, max_marks, max_steps)) != PVX_OK) return rc;
    if ((rc = marks_track("pvx_marks_corr", tf, f, ntf)) != PVX_OK) return rc;
    if (window < 2 || !(min_per == min_per) || (nrows > 0 && !t0)) { pvx_set_error("pvx_marks_corr: window %d, min_per %g", window, min_per); return PVX_ERR_INVALID; }
    int cap = 0;
    if ((rc = marks_corr_plan(f, ntf, f_fallback, sr, window, &cap)) != PVX_OK) return rc;
    t_marks_kernels = "";
    if (nrows == 0) return 0;
    if (!d_x || !d_marks || !d_count || !d_status) { pvx_set_error("null pvx_marks_corr array"); return PVX_ERR_INVALID; }
    MarksCorrParams p = {};
    p.x = d_x; p.nsamp = nsamp; p.nrows = nrows; p.f_fallback = f_fallback; p.sr = sr; p.min_per = min_per;
    p.W = window; p.cap = cap; p.max_marks = (int)max_marks; p.max_steps = max_steps;
    p.marks = d_marks; p.count = d_count; p.status = d_status;
    MarksRows h = {row_start, row_stop, t0, toff, tf, f, ntf, ntf};
    if ((rc = pvx_marks_corr_run(p, h, (hipStream_t)stream, &t_marks_kernels)) != PVX_OK) return rc;   // synchronises the stream
    return nrows;
}

extern "C" int64_t pvx_marks_corr(const double* x, int64_t nsamp, const int64_t* row_start, const int64_t* row_stop, const double* t0,
                                  const double* toff, int64_t nrows, const double* tf, const double* f, int64_t ntf, double f_fallback,
                                  double sr, int window, double min_per, int64_t max_marks, int64_t max_steps, double* marks,
                                  int32_t* count, int32_t* status) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    if ((rc = marks_args("pvx_marks_corr", nsamp, row_start, row_stop, nrows, sr, max_marks, max_steps)) != PVX_OK) return rc;
    t_marks_kernels = "";
    if (nrows == 0) return 0;
    if (!x || !marks || !count || !status) { pvx_set_error("null pvx_marks_corr array"); return PVX_ERR_INVALID; }
    const size_t mb = (size_t)nrows * (size_t)max_marks * 8, ib = (size_t)nrows * 4;
    Staged dx, dm, dc, ds;
    if ((rc = dm.room(mb)) != PVX_OK || (rc = dc.room(ib)) != PVX_OK || (rc = ds.room(ib)) != PVX_OK ||
        (rc = dx.put(x, (size_t)nsamp * 8)) != PVX_OK) return rc;
    PVX_HIP_CHECK(hipMemsetAsync(dm.as<void>(), 0, mb, nullptr));      // the padding behind a row's marks reads as 0
    const int64_t r = pvx_marks_corr_dev(dx.as<double>(), nsamp, row_start, row_stop, t0, toff, nrows, tf, f, ntf, f_fallback, sr,
                                         window, min_per, max_marks, max_steps, dm.as<double>(), dc.as<int32_t>(), ds.as<int32_t>(), nullptr);
    if (r < 0) return r;
    if ((rc = dm.get(marks, mb)) != PVX_OK || (rc = dc.get(count, ib)) != PVX_OK || (rc = ds.get(status, ib)) != PVX_OK) return rc;
    return nrows;
}

extern "C" int64_t pvx_marks_peak_dev(const double* d_x, int64_t nsamp, const int64_t* row_start, const int64_t* row_stop, const double* toff,
                                      int64_t nrows, const double* tf, const double* f, int64_t ntf, int64_t nf, double sr, int fit_points,
                                      int64_t max_marks, int64_t max_steps, double* d_marks, double* d_vals, int32_t* d_count,
                                      int32_t* d_status, void* stream) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    if ((rc = marks_args("pvx_marks_peak", nsamp, row_start, row_stop, nrows, sr, max_marks, max_steps)) != PVX_OK) return rc;
    if (tf) {
        if ((rc = marks_track("pvx_marks_peak", tf, f, ntf)) != PVX_OK) return rc;
        nf = ntf;
    } else {
        ntf = 0;
        if (!f || (nf != 1 && nf != nsamp)) {
            pvx_set_error("pvx_marks_peak: without tf, f holds one value or one per sample (%lld values, %lld samples)", (long long)nf, (long long)nsamp);
            return PVX_ERR_INVALID;
        }
    }
    if (fit_points < 3) { pvx_set_error("pvx_marks_peak: fit_points %d (at least 3)", fit_points); return PVX_ERR_INVALID; }
    if (fit_points > PVX_MARKS_MAX_FIT_POINTS) {
        pvx_set_error("pvx_marks_peak: fit_points %d (the kernel takes up to %d)", fit_points, PVX_MARKS_MAX_FIT_POINTS);
        return PVX_ERR_UNSUPPORTED;
    }
    t_marks_kernels = "";
    if (nrows == 0) return 0;
    if (!d_x || !d_marks || !d_vals || !d_count || !d_status) { pvx_set_error("null pvx_marks_peak array"); return PVX_ERR_INVALID; }
    MarksPeakParams p = {};
    p.x = d_x; p.nsamp = nsamp; p.nrows = nrows; p.sr = sr; p.fit_points = fit_points;
    p.max_marks = (int)max_marks; p.max_steps = max_steps;
    p.marks = d_marks; p.vals = d_vals; p.count = d_count; p.status = d_status;
    MarksRows h = {row_start, row_stop, nullptr, toff, tf, f, ntf, nf};
    if ((rc = pvx_marks_peak_run(p, h, (hipStream_t)stream, &t_marks_kernels)) != PVX_OK) return rc;   // synchronises the stream
    return nrows;
}

extern "C" int64_t pvx_marks_peak(const double* x, int64_t nsamp, const int64_t* row_start, const int64_t* row_stop, const double* toff,
                                  int64_t nrows, const double* tf, const double* f, int64_t ntf, int64_t nf, double sr, int fit_points,
                                  int64_t max_marks, int64_t max_steps, double* marks, double* vals, int32_t* count, int32_t* status) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    if ((rc = marks_args("pvx_marks_peak", nsamp, row_start, row_stop, nrows, sr, max_marks, max_steps)) != PVX_OK) return rc;
    t_marks_kernels = "";
    if (nrows == 0) return 0;
    if (!x || !marks || !vals || !count || !status) { pvx_set_error("null pvx_marks_peak array"); return PVX_ERR_INVALID; }
    const size_t mb = (size_t)nrows * (size_t)max_marks * 8, ib = (size_t)nrows * 4;
    Staged dx, dm, dv, dc, ds;
    if ((rc = dm.room(mb)) != PVX_OK || (rc = dv.room(mb)) != PVX_OK || (rc = dc.room(ib)) != PVX_OK || (rc = ds.room(ib)) != PVX_OK ||
        (rc = dx.put(x, (size_t)nsamp * 8)) != PVX_OK) return rc;
    PVX_HIP_CHECK(hipMemsetAsync(dm.as<void>(), 0, mb, nullptr));
    PVX_HIP_CHECK(hipMemsetAsync(dv.as<void>(), 0, mb, nullptr));
    const int64_t r = pvx_marks_peak_dev(dx.as<double>(), nsamp, row_start, row_stop, toff, nrows, tf, f, ntf, nf, sr, fit_points,
                                         max_marks, max_steps, dm.as<double>(), dv.as<double>(), dc.as<int32_t>(), ds.as<int32_t>(), nullptr);
    if (r < 0) return r;
    if ((rc = dm.get(marks, mb)) != PVX_OK || (rc = dv.get(vals, mb)) != PVX_OK || (rc = dc.get(count, ib)) != PVX_OK ||
        (rc = ds.get(status, ib)) != PVX_OK) return rc;
    return nrows;
}

// ---- FFT filter banks (k_fbank.hip) -----------------------------------------------------------
static thread_local const char* t_fbank_kernels = "";
extern "C" const char* pvx_filterbank_last_kernels(void) { return t_fbank_kernels; }

static int fbank_args(int x_dtype, int64_t n, const double* wind, int nwind, int hop, const double* fb, int nband, int cep_mode,
                      const double* spec, const double* cep) {
    if (n < 0 || !wind || nwind < 2 || hop < 1 || !fb || nband < 1) { pvx_set_error("bad filter-bank argument"); return PVX_ERR_INVALID; }
    if (x_dtype != PVX_F32 && x_dtype != PVX_F64 && x_dtype != PVX_I16) { pvx_set_error("bad x_dtype %d", x_dtype); return PVX_ERR_INVALID; }
    if (cep_mode < PVX_CEP_NONE || cep_mode > PVX_CEP_IFFT) { pvx_set_error("pvx_filterbank: unknown cep_mode %d", cep_mode); return PVX_ERR_INVALID; }
    if (nband > PVX_FBANK_MAX_NBAND) { pvx_set_error("pvx_filterbank: %d bands (the kernels take up to %d)", nband, PVX_FBANK_MAX_NBAND); return PVX_ERR_UNSUPPORTED; }
    if (cep_mode == PVX_CEP_DCT1 && nband < 2) { pvx_set_error("pvx_filterbank: DCT type 1 needs at least 2 bands"); return PVX_ERR_INVALID; }
    if ((cep_mode != PVX_CEP_NONE && !cep) || (!spec && !cep)) { pvx_set_error("null filter-bank output"); return PVX_ERR_INVALID; }
    return PVX_OK;
}

extern "C" int64_t pvx_filterbank_dev(const void* d_x, int x_dtype, int64_t n, const double* wind, int nwind, int hop, const double* fb,
                                      int nband, int cep_mode, double* d_spec, double* d_cep, void* stream) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    if ((rc = fbank_args(x_dtype, n, wind, nwind, hop, fb, nband, cep_mode, d_spec, d_cep)) != PVX_OK) return rc;
    t_fbank_kernels = "";
    const int64_t nfr = pvx_nframes(n, nwind, hop);                   // FFTFilters.py:280: n < len(w) - nwind, the analysis framing
    if (nfr == 0) return 0;
    if (!d_x) { pvx_set_error("null filter-bank signal"); return PVX_ERR_INVALID; }
    if ((rc = pvx_fbank_run(d_x, x_dtype, nfr, wind, nwind, hop, fb, nband, cep_mode, d_spec, cep_mode ? d_cep : nullptr,
                            (hipStream_t)stream, &t_fbank_kernels)) != PVX_OK) return rc;   // synchronises the stream
    return nfr;
}

extern "C" int64_t pvx_filterbank(const void* x, int x_dtype, int64_t n, const double* wind, int nwind, int hop, const double* fb,
                                  int nband, int cep_mode, double* spec, double* cep) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    if ((rc = fbank_args(x_dtype, n, wind, nwind, hop, fb, nband, cep_mode, spec, cep)) != PVX_OK) return rc;
    t_fbank_kernels = "";
    const int64_t nfr = pvx_nframes(n, nwind, hop);
    if (nfr == 0) return 0;
    if (!x) { pvx_set_error("null filter-bank signal"); return PVX_ERR_INVALID; }
    if (!cep_mode) cep = nullptr;
    // frames do not depend on each other: a chunk of frames needs its own samples only (neighbouring chunks overlap by
    // nwind - hop), so the device holds one chunk of input and its results whatever the signal's length
    const size_t limit = pvx_device_bytes_limit((size_t)2 << 30);   // per buffer
    const size_t es = dtype_size(x_dtype);
    const size_t sb = (size_t)nband * 8, cb = cep ? sb * (cep_mode == PVX_CEP_IFFT ? 2 : 1) : 0;
    int64_t fc = (int64_t)(limit / es) > nwind ? ((int64_t)(limit / es) - nwind) / hop + 1 : 1;
    fc = std::min<int64_t>(fc, std::max<int64_t>(1, (int64_t)(limit / std::max(sb, cb))));
    fc = std::min(fc, nfr);
    DevMem dx, ds, dc;
    if ((rc = dx.alloc((size_t)((fc - 1) * hop + nwind) * es)) != PVX_OK || (spec && (rc = ds.alloc((size_t)fc * sb)) != PVX_OK) ||
        (cep && (rc = dc.alloc((size_t)fc * cb)) != PVX_OK)) return rc;
    for (int64_t f0 = 0; f0 < nfr; f0 += fc) {
        const int64_t cnt = std::min(fc, nfr - f0);
        if ((rc = pvx_host_to_device(dx.get(), (const char*)x + (size_t)(f0 * hop) * es, (size_t)((cnt - 1) * hop + nwind) * es)) != PVX_OK) return rc;
        if ((rc = pvx_fbank_run(dx.get(), x_dtype, cnt, wind, nwind, hop, fb, nband, cep_mode, spec ? ds.as<double>() : nullptr,
                                cep ? dc.as<double>() : nullptr, nullptr, &t_fbank_kernels)) != PVX_OK) return rc;
        if (spec && (rc = pvx_device_to_host((char*)spec + (size_t)f0 * sb, ds.get(), (size_t)cnt * sb)) != PVX_OK) return rc;
        if (cep && (rc = pvx_device_to_host((char*)cep + (size_t)f0 * cb, dc.get(), (size_t)cnt * cb)) != PVX_OK) return rc;
    }
    return nfr;
}

// ---- windowed spectral measures (k_specdesc.hip) ------------------------------------------------
static thread_local const char* t_specdesc_kernels = "";
extern "C" const char* pvx_specdesc_last_kernels(void) { return t_specdesc_kernels; }

// frames read: 0 .. nfr - 1, and frame nfr too for the flux
static int specdesc_args(int x_dtype, int64_t n, const double* wind, int nwind, int hop, int64_t nfr, int measure, const double* a,
                         const double* b, const double* out) {
    if (n < 0 || !wind || nwind < 2 || hop < 1 || nfr < 0) { pvx_set_error("bad pvx_specdesc argument"); return PVX_ERR_INVALID; }
    if (x_dtype != PVX_F32 && x_dtype != PVX_F64 && x_dtype != PVX_I16) { pvx_set_error("bad x_dtype %d", x_dtype); return PVX_ERR_INVALID; }
    if (measure < PVX_SD_RATIO || measure > PVX_SD_PSD) { pvx_set_error("pvx_specdesc: unknown measure %d", measure); return PVX_ERR_INVALID; }
    if ((measure != PVX_SD_PSD && !a) || (measure == PVX_SD_RATIO && !b)) { pvx_set_error("pvx_specdesc: null weights"); return PVX_ERR_INVALID; }
    const int64_t last = measure == PVX_SD_FLUX ? nfr : nfr - 1;
    if (nfr > 0 && (last > (INT64_MAX - nwind) / hop || last * hop + nwind > n)) {
        pvx_set_error("pvx_specdesc: frame %lld of %d samples at hop %d ends beyond the %lld samples of the signal", (long long)last, nwind, hop,
                      (long long)n);
        return PVX_ERR_SIZE;
    }
    if (nfr > 0 && !out) { pvx_set_error("null pvx_specdesc output"); return PVX_ERR_INVALID; }
    return PVX_OK;
}

extern "C" int64_t pvx_specdesc_dev(const void* d_x, int x_dtype, int64_t n, const double* wind, int nwind, int hop, int64_t nfr, int measure,
                                    const double* a, const double* b, double* d_out, void* stream) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    if ((rc = specdesc_args(x_dtype, n, wind, nwind, hop, nfr, measure, a, b, d_out)) != PVX_OK) return rc;
    t_specdesc_kernels = "";
    if (nfr == 0) return 0;
    if (!d_x) { pvx_set_error("null pvx_specdesc signal"); return PVX_ERR_INVALID; }
    if ((rc = pvx_specdesc_run(d_x, x_dtype, nfr, wind, nwind, hop, measure, a, b, d_out, true, nfr, (hipStream_t)stream,
                               &t_specdesc_kernels)) != PVX_OK) return rc;   // synchronises the stream
    return nfr;
}

extern "C" int64_t pvx_specdesc(const void* x, int x_dtype, int64_t n, const double* wind, int nwind, int hop, int64_t nfr, int measure,
                                const double* a, const double* b, double* out) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    if ((rc = specdesc_args(x_dtype, n, wind, nwind, hop, nfr, measure, a, b, out)) != PVX_OK) return rc;
    t_specdesc_kernels = "";
    if (nfr == 0) return 0;
    if (!x) { pvx_set_error("null pvx_specdesc signal"); return PVX_ERR_INVALID; }
    // a chunk of values needs its own samples only (a flux chunk: one frame more); the periodogram's chunks are whole
    // blocks, so that the block sums -- and with them the bits -- are those of the unchunked call
    const size_t limit = pvx_device_bytes_limit((size_t)2 << 30);   // per buffer
    const size_t es = dtype_size(x_dtype);
    const bool psd = measure == PVX_SD_PSD;
    const int64_t extra = measure == PVX_SD_FLUX ? 1 : 0;
    const int64_t room = (int64_t)(limit / es);                       // samples
    int64_t fc = room > nwind + extra * hop ? (room - nwind) / hop + 1 - extra : 1;
    fc = std::min<int64_t>(fc, std::max<int64_t>(1, (int64_t)(limit / 8)));
    if (psd) fc = std::max<int64_t>(fc - fc % PVX_SPECDESC_BLOCK, PVX_SPECDESC_BLOCK);
    fc = std::min(fc, nfr);
    DevMem dx, dout;
    if ((rc = dx.alloc((size_t)((fc - 1 + extra) * hop + nwind) * es)) != PVX_OK ||
        (rc = dout.alloc((size_t)(psd ? nwind / 2 : fc) * 8)) != PVX_OK) return rc;
    for (int64_t f0 = 0; f0 < nfr; f0 += fc) {
        const int64_t cnt = std::min(fc, nfr - f0);
        if ((rc = pvx_host_to_device(dx.get(), (const char*)x + (size_t)(f0 * hop) * es, (size_t)((cnt - 1 + extra) * hop + nwind) * es)) != PVX_OK) return rc;
        if ((rc = pvx_specdesc_run(dx.get(), x_dtype, cnt, wind, nwind, hop, measure, a, b, dout.as<double>(), f0 == 0,
                                   f0 + cnt == nfr ? nfr : 0, nullptr, &t_specdesc_kernels)) != PVX_OK) return rc;
        if (!psd && (rc = pvx_device_to_host((char*)out + (size_t)f0 * 8, dout.get(), (size_t)cnt * 8)) != PVX_OK) return rc;
    }
    if (psd && (rc = pvx_device_to_host(out, dout.get(), (size_t)(nwind / 2) * 8)) != PVX_OK) return rc;
    return nfr;
}

// ---- cross and auto spectra block by block (k_xspec.hip) ---------------------------------------
static thread_local const char* t_xspec_kernels = "";
extern "C" const char* pvx_xspec_last_kernels(void) { return t_xspec_kernels; }

// samples read: start .. start + (nblk-1)*delta + (nseg-1)*step + nwind - 1
static int xspec_args(const void* y, int x_dtype, int64_t n, const double* wind, int nwind, int step, int64_t start, int64_t delta,
                      int64_t nblk, int nseg, const double* sxy, const double* sxx, const double* syy) {
    if (n < 0 || !wind || nwind < 2 || step < 1 || start < 0 || delta < 1 || nblk < 0 || nseg < 1) {
        pvx_set_error("bad pvx_xspec argument");
        return PVX_ERR_INVALID;
    }
    if (x_dtype != PVX_F32 && x_dtype != PVX_F64 && x_dtype != PVX_I16) { pvx_set_error("bad x_dtype %d", x_dtype); return PVX_ERR_INVALID; }
    if (nblk > 0) {
        const __int128 end = (__int128)start + (__int128)(nblk - 1) * delta + (__int128)(nseg - 1) * step + nwind;
        if (end > (__int128)n) {
            pvx_set_error("pvx_xspec: block %lld (%d segments of %d samples at step %d, blocks %lld apart from %lld) ends beyond the %lld samples of the signals",
                          (long long)(nblk - 1), nseg, nwind, step, (long long)delta, (long long)start, (long long)n);
            return PVX_ERR_SIZE;
        }
        if ((__int128)nblk * (nwind / 2 + 1) > ((__int128)1 << 56)) { pvx_set_error("pvx_xspec: too many blocks"); return PVX_ERR_INVALID; }
        if (!sxx || (y && (!sxy || !syy))) { pvx_set_error("null pvx_xspec output"); return PVX_ERR_INVALID; }
    }
    return PVX_OK;
}

extern "C" int64_t pvx_xspec_dev(const void* d_x, const void* d_y, int x_dtype, int64_t n, const double* wind, int nwind, int step,
                                 int64_t start, int64_t delta, int64_t nblk, int nseg, double* d_sxy, double* d_sxx, double* d_syy,
                                 void* stream) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    if ((rc = xspec_args(d_y, x_dtype, n, wind, nwind, step, start, delta, nblk, nseg, d_sxy, d_sxx, d_syy)) != PVX_OK) return rc;
    t_xspec_kernels = "";
    if (nblk == 0) return 0;
    if (!d_x) { pvx_set_error("null pvx_xspec signal"); return PVX_ERR_INVALID; }
    const size_t es = dtype_size(x_dtype);
    if ((rc = pvx_xspec_run((const char*)d_x + (size_t)start * es, d_y ? (const char*)d_y + (size_t)start * es : nullptr, x_dtype, wind, nwind,
                            step, delta, nblk, nseg, d_sxy, d_sxx, d_syy, (hipStream_t)stream, &t_xspec_kernels)) != PVX_OK) return rc;   // synchronises the stream
    return nblk;
}

extern "C" int64_t pvx_xspec(const void* x, const void* y, int x_dtype, int64_t n, const double* wind, int nwind, int step, int64_t start,
                             int64_t delta, int64_t nblk, int nseg, double* sxy, double* sxx, double* syy) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    if ((rc = xspec_args(y, x_dtype, n, wind, nwind, step, start, delta, nblk, nseg, sxy, sxx, syy)) != PVX_OK) return rc;
    t_xspec_kernels = "";
    if (nblk == 0) return 0;
    if (!x) { pvx_set_error("null pvx_xspec signal"); return PVX_ERR_INVALID; }
    // a chunk is whole blocks with the samples they read, the same cut for both signals: a block's bits are those of the
    // unchunked call
    const size_t limit = pvx_device_bytes_limit((size_t)2 << 30);   // per buffer
    const size_t es = dtype_size(x_dtype);
    const int64_t nhalf = nwind / 2 + 1;
    const int64_t span = (int64_t)(nseg - 1) * step + nwind;          // samples of a block
    const int64_t room = (int64_t)(limit / es);
    int64_t bc = room > span ? (room - span) / delta + 1 : 1;
    bc = std::min<int64_t>(bc, std::max<int64_t>(1, (int64_t)(limit / ((size_t)nhalf * 16))));
    bc = std::min(bc, nblk);
    const size_t chunk_samples = (size_t)((bc - 1) * delta + span);
    DevMem dx, dy, dxy, dxx, dyy;
    if ((rc = dx.alloc(chunk_samples * es)) != PVX_OK || (rc = dxx.alloc((size_t)(bc * nhalf) * 8)) != PVX_OK) return rc;
    if (y && ((rc = dy.alloc(chunk_samples * es)) != PVX_OK || (rc = dxy.alloc((size_t)(bc * nhalf) * 16)) != PVX_OK ||
              (rc = dyy.alloc((size_t)(bc * nhalf) * 8)) != PVX_OK)) return rc;
    for (int64_t b0 = 0; b0 < nblk; b0 += bc) {
        const int64_t cnt = std::min(bc, nblk - b0);
        const size_t off = (size_t)(start + b0 * delta) * es, bytes = (size_t)((cnt - 1) * delta + span) * es;
        if ((rc = pvx_host_to_device(dx.get(), (const char*)x + off, bytes)) != PVX_OK) return rc;
        if (y && (rc = pvx_host_to_device(dy.get(), (const char*)y + off, bytes)) != PVX_OK) return rc;
        if ((rc = pvx_xspec_run(dx.get(), y ? dy.get() : nullptr, x_dtype, wind, nwind, step, delta, cnt, nseg, dxy.as<double>(), dxx.as<double>(),
                                dyy.as<double>(), nullptr, &t_xspec_kernels)) != PVX_OK) return rc;
        if ((rc = pvx_device_to_host((char*)sxx + (size_t)(b0 * nhalf) * 8, dxx.get(), (size_t)(cnt * nhalf) * 8)) != PVX_OK) return rc;
        if (y && ((rc = pvx_device_to_host((char*)syy + (size_t)(b0 * nhalf) * 8, dyy.get(), (size_t)(cnt * nhalf) * 8)) != PVX_OK ||
                  (rc = pvx_device_to_host((char*)sxy + (size_t)(b0 * nhalf) * 16, dxy.get(), (size_t)(cnt * nhalf) * 16)) != PVX_OK)) return rc;
    }
    return nblk;
}

// ---- fricative descriptors of many snippets of one signal (k_fric.hip) ---------------------------
static thread_local const char* t_fric_kernels = "";
extern "C" const char* pvx_fric_last_kernels(void) { return t_fric_kernels; }

// what: 1 the spectra, 2 the descriptors and the RMS
static int fric_args(int x_dtype, int64_t n, const int64_t* starts, int64_t nrows, int L, int nwind, double sr, const double* freq,
                     const double* psd, const double* desc, const int32_t* imax, const int32_t* status, const double* rms, int what) {
    if (nrows < 0) { pvx_set_error("pvx_fricative: nrows %lld", (long long)nrows); return PVX_ERR_SIZE; }
    if (L < 2) { pvx_set_error("pvx_fricative: snippets of %d samples (at least 2 are needed)", L); return PVX_ERR_SIZE; }
    if (n < 0 || nwind < 2 || !(sr > 0.0)) { pvx_set_error("bad pvx_fricative argument"); return PVX_ERR_INVALID; }
    if (x_dtype != PVX_F32 && x_dtype != PVX_F64 && x_dtype != PVX_I16) { pvx_set_error("bad x_dtype %d", x_dtype); return PVX_ERR_INVALID; }
    if (nrows > 0) {
        if (!starts) { pvx_set_error("null pvx_fricative starts"); return PVX_ERR_INVALID; }
        for (int64_t r = 0; r < nrows; r++)
            if (starts[r] < 0 || starts[r] > n - L) {
                pvx_set_error("pvx_fricative: row %lld (samples %lld .. %lld) does not lie inside the %lld samples of the signal", (long long)r,
                              (long long)starts[r], (long long)starts[r] + L - 1, (long long)n);
                return PVX_ERR_SIZE;
            }
        if ((__int128)nrows * (std::min(nwind, L) / 2 + 1) > ((__int128)1 << 56)) { pvx_set_error("pvx_fricative: too many rows"); return PVX_ERR_INVALID; }
        if (((what & 2) && (!freq || !desc || !imax || !status || !rms)) || (!(what & 2) && !psd)) {
            pvx_set_error("null pvx_fricative output");
            return PVX_ERR_INVALID;
        }
    }
    return PVX_OK;
}

static int64_t fric_dev(const void* d_x, int x_dtype, int64_t n, const int64_t* starts, int64_t nrows, int L, int nwind, const double* win,
                        double sr, const double* freq, double* d_psd, double* d_desc, int32_t* d_imax, int32_t* d_status, double* d_rms,
                        void* stream, int what) {
    int rc;
    if ((rc = fric_args(x_dtype, n, starts, nrows, L, nwind, sr, freq, d_psd, d_desc, d_imax, d_status, d_rms, what)) != PVX_OK) return rc;
    if ((rc = pvx_require_device()) != PVX_OK) return rc;
    t_fric_kernels = "";
    if (nrows == 0) return 0;
    if (!d_x) { pvx_set_error("null pvx_fricative signal"); return PVX_ERR_INVALID; }
    if ((rc = pvx_fric_run(d_x, x_dtype, starts, nrows, L, nwind, win, sr, freq, d_psd, (what & 2) ? d_desc : nullptr, d_imax, d_status, d_rms,
                           (hipStream_t)stream, &t_fric_kernels)) != PVX_OK) return rc;   // synchronises the stream
    return nrows;
}

static int64_t fric_host(const void* x, int x_dtype, int64_t n, const int64_t* starts, int64_t nrows, int L, int nwind, const double* win,
                         double sr, const double* freq, double* psd, double* desc, int32_t* imax, int32_t* status, double* rms, int what) {
    int rc;
    if ((rc = fric_args(x_dtype, n, starts, nrows, L, nwind, sr, freq, psd, desc, imax, status, rms, what)) != PVX_OK) return rc;
    if ((rc = pvx_require_device()) != PVX_OK) return rc;
    t_fric_kernels = "";
    if (nrows == 0) return 0;
    if (!x) { pvx_set_error("null pvx_fricative signal"); return PVX_ERR_INVALID; }
    // a group is consecutive rows of the call with the span of samples they cover: a row's bits are those of the unchunked call
    const size_t limit = pvx_device_bytes_limit((size_t)2 << 30);
    const size_t es = dtype_size(x_dtype);
    const int64_t nhalf = std::min(nwind, L) / 2 + 1;
    const int64_t room = std::max<int64_t>((int64_t)(limit / es), L);  // samples of a group's span
    const int64_t maxrows = std::max<int64_t>(1, (int64_t)(limit / ((size_t)nhalf * 8)));
    const bool tail = (what & 2) != 0;
    DevMem dx, dpsd, ddesc, dim, dst, drms;
    std::vector<int64_t> rel;
    for (int64_t r0 = 0; r0 < nrows;) {
        int64_t lo = starts[r0], hi = starts[r0] + L, r1 = r0 + 1;
        while (r1 < nrows && r1 - r0 < maxrows) {
            const int64_t nlo = std::min(lo, starts[r1]), nhi = std::max(hi, starts[r1] + L);
            if (nhi - nlo > room) break;
            lo = nlo; hi = nhi; r1++;
        }
        const int64_t cnt = r1 - r0;
        rel.resize((size_t)cnt);
        for (int64_t i = 0; i < cnt; i++) rel[(size_t)i] = starts[r0 + i] - lo;
        if ((rc = dx.grow((size_t)(hi - lo) * es, Sizing::exact)) != PVX_OK) return rc;
        if (psd && (rc = dpsd.grow((size_t)(cnt * nhalf) * 8, Sizing::exact)) != PVX_OK) return rc;
        if (tail && ((rc = ddesc.grow((size_t)cnt * 56, Sizing::exact)) != PVX_OK || (rc = dim.grow((size_t)cnt * 4, Sizing::exact)) != PVX_OK ||
                     (rc = dst.grow((size_t)cnt * 4, Sizing::exact)) != PVX_OK || (rc = drms.grow((size_t)cnt * 8, Sizing::exact)) != PVX_OK)) return rc;
        if ((rc = pvx_host_to_device(dx.get(), (const char*)x + (size_t)lo * es, (size_t)(hi - lo) * es)) != PVX_OK) return rc;
        if ((rc = pvx_fric_run(dx.get(), x_dtype, rel.data(), cnt, L, nwind, win, sr, freq, psd ? dpsd.as<double>() : nullptr,
                               tail ? ddesc.as<double>() : nullptr, dim.as<int32_t>(), dst.as<int32_t>(), drms.as<double>(), nullptr,
                               &t_fric_kernels)) != PVX_OK) return rc;
        if (psd && (rc = pvx_device_to_host((char*)psd + (size_t)(r0 * nhalf) * 8, dpsd.get(), (size_t)(cnt * nhalf) * 8)) != PVX_OK) return rc;
        if (tail && ((rc = pvx_device_to_host((char*)desc + (size_t)r0 * 56, ddesc.get(), (size_t)cnt * 56)) != PVX_OK ||
                     (rc = pvx_device_to_host((char*)imax + (size_t)r0 * 4, dim.get(), (size_t)cnt * 4)) != PVX_OK ||
                     (rc = pvx_device_to_host((char*)status + (size_t)r0 * 4, dst.get(), (size_t)cnt * 4)) != PVX_OK ||
                     (rc = pvx_device_to_host((char*)rms + (size_t)r0 * 8, drms.get(), (size_t)cnt * 8)) != PVX_OK)) return rc;
        r0 = r1;
    }
    return nrows;
}

extern "C" int64_t pvx_welch(const void* x, int x_dtype, int64_t n, const int64_t* starts, int64_t nrows, int L, int nwind, const double* win,
                             double sr, double* psd) {
    return fric_host(x, x_dtype, n, starts, nrows, L, nwind, win, sr, nullptr, psd, nullptr, nullptr, nullptr, nullptr, 1);
}
extern "C" int64_t pvx_welch_dev(const void* d_x, int x_dtype, int64_t n, const int64_t* starts, int64_t nrows, int L, int nwind,
                                 const double* win, double sr, double* d_psd, void* stream) {
    return fric_dev(d_x, x_dtype, n, starts, nrows, L, nwind, win, sr, nullptr, d_psd, nullptr, nullptr, nullptr, nullptr, stream, 1);
}
extern "C" int64_t pvx_fricative(const void* x, int x_dtype, int64_t n, const int64_t* starts, int64_t nrows, int L, int nwind,
                                 const double* win, double sr, const double* freq, double* psd, double* desc, int32_t* imax, int32_t* status,
                                 double* rms) {
    return fric_host(x, x_dtype, n, starts, nrows, L, nwind, win, sr, freq, psd, desc, imax, status, rms, 3);
}
extern "C" int64_t pvx_fricative_dev(const void* d_x, int x_dtype, int64_t n, const int64_t* starts, int64_t nrows, int L, int nwind,
                                     const double* win, double sr, const double* freq, double* d_psd, double* d_desc, int32_t* d_imax,
                                     int32_t* d_status, double* d_rms, void* stream) {
    return fric_dev(d_x, x_dtype, n, starts, nrows, L, nwind, win, sr, freq, d_psd, d_desc, d_imax, d_status, d_rms, stream, 3);
}

static int fric_desc_args(int64_t nrows, int nb, const double* psd, const double* freq, const double* desc, const int32_t* imax,
                          const int32_t* status) {
    if (nrows < 0 || nb < 2) { pvx_set_error("pvx_fric_desc: %lld rows of %d bins (at least 2 are needed)", (long long)nrows, nb); return PVX_ERR_SIZE; }
    if (nrows > 0 && (!psd || !freq || !desc || !imax || !status)) { pvx_set_error("null pvx_fric_desc argument"); return PVX_ERR_INVALID; }
    if ((__int128)nrows * nb > ((__int128)1 << 56)) { pvx_set_error("pvx_fric_desc: too many rows"); return PVX_ERR_INVALID; }
    return PVX_OK;
}

extern "C" int64_t pvx_fric_desc_dev(const double* d_psd, int64_t nrows, int nb, const double* freq, double* d_desc, int32_t* d_imax,
                                     int32_t* d_status, void* stream) {
    int rc;
    if ((rc = fric_desc_args(nrows, nb, d_psd, freq, d_desc, d_imax, d_status)) != PVX_OK) return rc;
    if ((rc = pvx_require_device()) != PVX_OK) return rc;
    t_fric_kernels = "";
    if (nrows == 0) return 0;
    // (a row of nb bins is the half spectrum of segments of 2 (nb - 1) samples: the geometry the run derives its bin count from)
    const int nper = 2 * (nb - 1);
    if ((rc = pvx_fric_run(nullptr, PVX_F64, nullptr, nrows, nper, nper, nullptr, 1.0, freq, (double*)d_psd, d_desc, d_imax, d_status, nullptr,
                           (hipStream_t)stream, &t_fric_kernels)) != PVX_OK) return rc;
    return nrows;
}

extern "C" int64_t pvx_fric_desc(const double* psd, int64_t nrows, int nb, const double* freq, double* desc, int32_t* imax, int32_t* status) {
    int rc;
    if ((rc = fric_desc_args(nrows, nb, psd, freq, desc, imax, status)) != PVX_OK) return rc;
    if ((rc = pvx_require_device()) != PVX_OK) return rc;
    t_fric_kernels = "";
    if (nrows == 0) return 0;
    const size_t limit = pvx_device_bytes_limit((size_t)2 << 30);
    const int64_t rc_rows = std::min<int64_t>(nrows, std::max<int64_t>(1, (int64_t)(limit / ((size_t)nb * 8))));
    DevMem dpsd, ddesc, dim, dst;
    if ((rc = dpsd.alloc((size_t)(rc_rows * nb) * 8)) != PVX_OK || (rc = ddesc.alloc((size_t)rc_rows * 56)) != PVX_OK ||
        (rc = dim.alloc((size_t)rc_rows * 4)) != PVX_OK || (rc = dst.alloc((size_t)rc_rows * 4)) != PVX_OK) return rc;
    const int nper = 2 * (nb - 1);
    for (int64_t r0 = 0; r0 < nrows; r0 += rc_rows) {
        const int64_t cnt = std::min(rc_rows, nrows - r0);
        if ((rc = pvx_host_to_device(dpsd.get(), (const char*)psd + (size_t)(r0 * nb) * 8, (size_t)(cnt * nb) * 8)) != PVX_OK) return rc;
        if ((rc = pvx_fric_run(nullptr, PVX_F64, nullptr, cnt, nper, nper, nullptr, 1.0, freq, dpsd.as<double>(), ddesc.as<double>(),
                               dim.as<int32_t>(), dst.as<int32_t>(), nullptr, nullptr, &t_fric_kernels)) != PVX_OK) return rc;
        if ((rc = pvx_device_to_host((char*)desc + (size_t)r0 * 56, ddesc.get(), (size_t)cnt * 56)) != PVX_OK ||
            (rc = pvx_device_to_host((char*)imax + (size_t)r0 * 4, dim.get(), (size_t)cnt * 4)) != PVX_OK ||
            (rc = pvx_device_to_host((char*)status + (size_t)r0 * 4, dst.get(), (size_t)cnt * 4)) != PVX_OK) return rc;
    }
    return nrows;
}

// ---- full cross-correlations and their peaks block by block (k_xcorr.hip) -----------------------
static thread_local const char* t_xcorr_kernels = "";
extern "C" const char* pvx_xcorr_last_kernels(void) { return t_xcorr_kernels; }

// samples read: start .. start + (nblk-1)*delta + la - 1 of a, .. + lv - 1 of v
static int xcorr_args(int x_dtype, int64_t na, int64_t nv, int la, int lv, int64_t start, int64_t delta, int64_t nblk, int detrend,
                      const int32_t* lag, const double* peak) {
    if (na < 0 || nv < 0 || la < 1 || lv < 1 || start < 0 || delta < 0 || nblk < 0) { pvx_set_error("bad pvx_xcorr_peak argument"); return PVX_ERR_INVALID; }
    if (detrend != PVX_DETREND_NONE && detrend != PVX_DETREND_CONSTANT && detrend != PVX_DETREND_LINEAR) {
        pvx_set_error("pvx_xcorr_peak: unknown detrend code %d", detrend);
        return PVX_ERR_INVALID;
    }
    if (x_dtype != PVX_F32 && x_dtype != PVX_F64 && x_dtype != PVX_I16) { pvx_set_error("bad x_dtype %d", x_dtype); return PVX_ERR_INVALID; }
    if (nblk > 0) {
        const __int128 first = (__int128)start + (__int128)(nblk - 1) * delta;
        if (first + la > (__int128)na || first + lv > (__int128)nv) {
            pvx_set_error("pvx_xcorr_peak: block %lld (%d and %d samples, blocks %lld apart from %lld) ends beyond the %lld and %lld samples of the signals",
                          (long long)(nblk - 1), la, lv, (long long)delta, (long long)start, (long long)na, (long long)nv);
            return PVX_ERR_SIZE;
        }
        if (pvx_xcorr_fft_route(la, lv) && ((int64_t)la + lv - 1 > (int64_t)PVX_XCORR_MAX_P || pvx_xcorr_padded(la, lv) == 0)) {
            pvx_set_error("pvx_xcorr_peak: %d + %d - 1 lags need a transform longer than %d", la, lv, (int)PVX_XCORR_MAX_P);
            return PVX_ERR_UNSUPPORTED;
        }
        if ((__int128)nblk * ((int64_t)la + lv - 1) > ((__int128)1 << 56)) { pvx_set_error("pvx_xcorr_peak: too many blocks"); return PVX_ERR_INVALID; }
        if (!lag || !peak) { pvx_set_error("null pvx_xcorr_peak output"); return PVX_ERR_INVALID; }
    }
    return PVX_OK;
}

extern "C" int64_t pvx_xcorr_peak_dev(const void* d_a, const void* d_v, int x_dtype, int64_t na, int64_t nv, int la, int lv, int64_t start,
                                      int64_t delta, int64_t nblk, int detrend, const double* win_a, const double* win_v, int use_abs,
                                      int32_t* d_lag, double* d_peak, double* d_corr, void* stream) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    t_xcorr_kernels = "";
    if ((rc = xcorr_args(x_dtype, na, nv, la, lv, start, delta, nblk, detrend, d_lag, d_peak)) != PVX_OK) return rc;
    if (nblk == 0) return 0;
    if (!d_a || !d_v) { pvx_set_error("null pvx_xcorr_peak signal"); return PVX_ERR_INVALID; }
    const size_t es = dtype_size(x_dtype);
    if ((rc = pvx_xcorr_run((const char*)d_a + (size_t)start * es, (const char*)d_v + (size_t)start * es, x_dtype, la, lv, delta, nblk, detrend, win_a,
                            win_v, use_abs, d_lag, d_peak, d_corr, (hipStream_t)stream, &t_xcorr_kernels)) != PVX_OK) return rc;   // synchronises the stream
    return nblk;
}

extern "C" int64_t pvx_xcorr_peak(const void* a, const void* v, int x_dtype, int64_t na, int64_t nv, int la, int lv, int64_t start, int64_t delta,
                                  int64_t nblk, int detrend, const double* win_a, const double* win_v, int use_abs, int32_t* lag, double* peak,
                                  double* corr) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    t_xcorr_kernels = "";
    if ((rc = xcorr_args(x_dtype, na, nv, la, lv, start, delta, nblk, detrend, lag, peak)) != PVX_OK) return rc;
    if (nblk == 0) return 0;
    if (!a || !v) { pvx_set_error("null pvx_xcorr_peak signal"); return PVX_ERR_INVALID; }
    // a chunk is whole blocks with the samples they read, the same cut for both signals: a block's bits are those of the
    // unchunked call
    const size_t limit = pvx_device_bytes_limit((size_t)2 << 30);   // per buffer
    const size_t es = dtype_size(x_dtype);
    const int64_t nlag = (int64_t)la + lv - 1;
    const int64_t span = std::max(la, lv);                            // samples of the longer block
    const int64_t room = (int64_t)(limit / es);
    int64_t bc = nblk;
    if (delta > 0) bc = std::min<int64_t>(bc, room > span ? (room - span) / delta + 1 : 1);
    bc = std::min<int64_t>(bc, std::max<int64_t>(1, (int64_t)(limit / ((size_t)(corr ? nlag : 1) * 8))));
    DevMem da, dv, dlag, dpeak, dcorr;
    if ((rc = da.alloc((size_t)((bc - 1) * delta + la) * es)) != PVX_OK || (rc = dv.alloc((size_t)((bc - 1) * delta + lv) * es)) != PVX_OK ||
        (rc = dlag.alloc((size_t)bc * 4)) != PVX_OK || (rc = dpeak.alloc((size_t)bc * 8)) != PVX_OK ||
        (corr && (rc = dcorr.alloc((size_t)(bc * nlag) * 8)) != PVX_OK)) return rc;
    for (int64_t b0 = 0; b0 < nblk; b0 += bc) {
        const int64_t cnt = std::min(bc, nblk - b0);
        const size_t off = (size_t)(start + b0 * delta) * es;
        if ((rc = pvx_host_to_device(da.get(), (const char*)a + off, (size_t)((cnt - 1) * delta + la) * es)) != PVX_OK ||
            (rc = pvx_host_to_device(dv.get(), (const char*)v + off, (size_t)((cnt - 1) * delta + lv) * es)) != PVX_OK) return rc;
        if ((rc = pvx_xcorr_run(da.get(), dv.get(), x_dtype, la, lv, delta, cnt, detrend, win_a, win_v, use_abs, dlag.as<int32_t>(), dpeak.as<double>(),
                                corr ? dcorr.as<double>() : nullptr, nullptr, &t_xcorr_kernels)) != PVX_OK) return rc;
        if ((rc = pvx_device_to_host((char*)lag + (size_t)b0 * 4, dlag.get(), (size_t)cnt * 4)) != PVX_OK ||
            (rc = pvx_device_to_host((char*)peak + (size_t)b0 * 8, dpeak.get(), (size_t)cnt * 8)) != PVX_OK) return rc;
        if (corr && (rc = pvx_device_to_host((char*)corr + (size_t)(b0 * nlag) * 8, dcorr.get(), (size_t)(cnt * nlag) * 8)) != PVX_OK) return rc;
    }
    return nblk;
}

// ---- linear prediction and glottal inverse filtering (k_iaif.hip) -------------------------------
static thread_local const char* t_iaif_kernels = "";
extern "C" const char* pvx_iaif_last_kernels(void) { return t_iaif_kernels; }

static const size_t kIaifLimit = (size_t)256 << 20;   // per buffer, unless PVX_MAX_DEVICE_BYTES says otherwise

// frames read: 0 .. nfr - 1
static int lpc_frames_args(const char* what, int x_dtype, int64_t n, int nwind, int hop, int64_t nfr) {
    if (n < 0 || nwind < 1 || hop < 1 || nfr < 0) { pvx_set_error("bad %s argument", what); return PVX_ERR_INVALID; }
    if (x_dtype != PVX_F32 && x_dtype != PVX_F64 && x_dtype != PVX_I16) { pvx_set_error("bad x_dtype %d", x_dtype); return PVX_ERR_INVALID; }
    if (nfr > 0 && (nfr - 1 > (INT64_MAX - nwind) / hop || (nfr - 1) * hop + nwind > n)) {
        pvx_set_error("%s: frame %lld of %d samples at hop %d ends beyond the %lld samples of the signal", what, (long long)(nfr - 1), nwind, hop,
                      (long long)n);
        return PVX_ERR_SIZE;
    }
    return PVX_OK;
}

// Frames in groups of `own`: a group computes its own frames and, for an overlap-add, the `ov` frames before them that reach
// into its first output samples (frames only reach forwards: none after them does).  A frame's values do not depend on its
// group, a sample adds its frames in ascending order whatever the group: the bits are those of one group.
template <bool DEV>
static int64_t iaif_body(const void* x, int x_dtype, int64_t n, int nwind, int hop, int64_t nfr, const double* hp_b, int ntaps,
                         const double* lpc_wind, const double* ola_wind, int pt, int pg, double leak, int n_it, double* glot, double* dglot,
                         double* g, double* dg, double* vt, double* gc, int64_t* singular_frame, hipStream_t s) {
    if (singular_frame) *singular_frame = -1;
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    t_iaif_kernels = "";
    if ((rc = lpc_frames_args("pvx_iaif", x_dtype, n, nwind, hop, nfr)) != PVX_OK) return rc;
    const bool ola = glot || dglot;
    if (!hp_b || !lpc_wind || (ola && !ola_wind) || nwind < 2 || ntaps < 1 || pt < 0 || pg < 0 || n_it < 0) {
        pvx_set_error("bad pvx_iaif argument");
        return PVX_ERR_INVALID;
    }
    if (nwind > PVX_IAIF_MAX_NWIND || ntaps > PVX_IAIF_MAX_TAPS || pt > PVX_LPC_MAX_ORDER || pg > PVX_LPC_MAX_ORDER) {
        pvx_set_error("pvx_iaif: nwind %d, %d taps, orders %d / %d: the kernel takes nwind <= %d, <= %d taps, orders <= %d", nwind, ntaps, pt, pg,
                      PVX_IAIF_MAX_NWIND, PVX_IAIF_MAX_TAPS, PVX_LPC_MAX_ORDER);
        return PVX_ERR_UNSUPPORTED;
    }
    if (nfr == 0) {
        if ((rc = zero_out<DEV>(glot, n, s)) != PVX_OK || (rc = zero_out<DEV>(dglot, n, s)) != PVX_OK) return rc;
        if (DEV) PVX_HIP_CHECK(hipStreamSynchronize(s));
        return 0;
    }
    if (!x) { pvx_set_error("null pvx_iaif signal"); return PVX_ERR_INVALID; }
    const size_t es = dtype_size(x_dtype), limit = pvx_device_bytes_limit(kIaifLimit);
    const int64_t ov = ola ? (nwind - 1 + hop - 1) / hop : 0;
    int64_t cap = std::max<int64_t>(1, (int64_t)(limit / ((size_t)nwind * 8)));                 // rows of g / dg
    cap = std::min<int64_t>(cap, (int64_t)(limit / es) > nwind ? ((int64_t)(limit / es) - nwind) / hop + 1 : 1);   // frames of samples
    const int64_t own = std::min(nfr, std::max<int64_t>(1, cap - ov));
    const int64_t rows = std::min(nfr, own + ov);
    const int gcw = (n_it > 0 ? pg : 1) + 1;
    DevMem dx, wg, wdg, wvt, wgc, og, odg;
    if ((rc = wg.alloc((size_t)rows * nwind * 8)) != PVX_OK || (rc = wdg.alloc((size_t)rows * nwind * 8)) != PVX_OK ||
        (rc = wvt.alloc((size_t)rows * (pt + 1) * 8)) != PVX_OK || (rc = wgc.alloc((size_t)rows * gcw * 8)) != PVX_OK) return rc;
    if (!DEV) {
        if ((rc = dx.alloc((size_t)((rows - 1) * hop + nwind) * es)) != PVX_OK) return rc;
        if (glot && (rc = og.alloc((size_t)(own * hop + nwind) * 8)) != PVX_OK) return rc;
        if (dglot && (rc = odg.alloc((size_t)(own * hop + nwind) * 8)) != PVX_OK) return rc;
    }
    const IaifCall call = {x_dtype, nwind, hop, ntaps, pt, pg, n_it, leak, hp_b, lpc_wind, ola_wind};
    const int64_t cover = (nfr - 1) * hop + nwind;                    // the samples beyond the last frame stay zero
    for (int64_t o0 = 0; o0 < nfr; o0 += own) {
        const int64_t o1 = std::min(nfr, o0 + own);
        const int64_t s0 = o0 * hop, s1 = o1 == nfr ? cover : o1 * hop;
        const int64_t lo = s0 - nwind + 1;
        const int64_t fa = ola ? (lo <= 0 ? 0 : (lo + hop - 1) / hop) : o0, nf = o1 - fa;
        const void* cx = (const char*)x + (size_t)(fa * hop) * es;
        if (!DEV) {
            if ((rc = pvx_host_to_device(dx.get(), cx, (size_t)((nf - 1) * hop + nwind) * es)) != PVX_OK) return rc;
            cx = dx.get();
        }
        double* pgl = glot ? (DEV ? glot + s0 : og.as<double>()) : nullptr;
        double* pdg = dglot ? (DEV ? dglot + s0 : odg.as<double>()) : nullptr;
        int64_t sing = -1;
        if ((rc = pvx_iaif_run(call, cx, fa, nf, wg.as<double>(), wdg.as<double>(), wvt.as<double>(), wgc.as<double>(), s0, s1 - s0, pgl, pdg,
                               &sing, s, &t_iaif_kernels)) != PVX_OK) return rc;   // synchronises the stream
        if (sing >= 0) {
            if (singular_frame) *singular_frame = fa + sing;
            pvx_set_error("pvx_iaif: frame %lld: Singular principal minor (a prediction error of exactly 0)", (long long)(fa + sing));
            return PVX_ERR_SINGULAR;
        }
        const size_t r0 = (size_t)(o0 - fa), cnt = (size_t)(o1 - o0);
        if ((rc = rows_out<DEV>(g ? g + (size_t)o0 * nwind : nullptr, wg.as<double>() + r0 * nwind, cnt * nwind * 8, s)) != PVX_OK ||
            (rc = rows_out<DEV>(dg ? dg + (size_t)o0 * nwind : nullptr, wdg.as<double>() + r0 * nwind, cnt * nwind * 8, s)) != PVX_OK ||
            (rc = rows_out<DEV>(vt ? vt + (size_t)o0 * (pt + 1) : nullptr, wvt.as<double>() + r0 * (pt + 1), cnt * (pt + 1) * 8, s)) != PVX_OK ||
            (rc = rows_out<DEV>(gc ? gc + (size_t)o0 * gcw : nullptr, wgc.as<double>() + r0 * gcw, cnt * gcw * 8, s)) != PVX_OK) return rc;
        if (!DEV) {
            if ((rc = rows_out<false>(glot ? glot + s0 : nullptr, og.get(), (size_t)(s1 - s0) * 8, s)) != PVX_OK ||
                (rc = rows_out<false>(dglot ? dglot + s0 : nullptr, odg.get(), (size_t)(s1 - s0) * 8, s)) != PVX_OK) return rc;
        }
    }
    if ((rc = zero_out<DEV>(glot ? glot + cover : nullptr, n - cover, s)) != PVX_OK ||
        (rc = zero_out<DEV>(dglot ? dglot + cover : nullptr, n - cover, s)) != PVX_OK) return rc;
    if (DEV) PVX_HIP_CHECK(hipStreamSynchronize(s));                  // (before the buffers of this call are freed, too)
    return nfr;
}

extern "C" int64_t pvx_iaif(const void* x, int x_dtype, int64_t n, int nwind, int hop, int64_t nfr, const double* hp_b, int ntaps,
                            const double* lpc_wind, const double* ola_wind, int tract_order, int glottal_order, double leak, int n_it,
                            double* glot, double* dglot, double* g, double* dg, double* vt, double* gc, int64_t* singular_frame) {
    return iaif_body<false>(x, x_dtype, n, nwind, hop, nfr, hp_b, ntaps, lpc_wind, ola_wind, tract_order, glottal_order, leak, n_it, glot, dglot,
                            g, dg, vt, gc, singular_frame, nullptr);
}

extern "C" int64_t pvx_iaif_dev(const void* d_x, int x_dtype, int64_t n, int nwind, int hop, int64_t nfr, const double* hp_b, int ntaps,
                                const double* lpc_wind, const double* ola_wind, int tract_order, int glottal_order, double leak, int n_it,
                                double* d_glot, double* d_dglot, double* d_g, double* d_dg, double* d_vt, double* d_gc,
                                int64_t* singular_frame, void* stream) {
    return iaif_body<true>(d_x, x_dtype, n, nwind, hop, nfr, hp_b, ntaps, lpc_wind, ola_wind, tract_order, glottal_order, leak, n_it, d_glot,
                           d_dglot, d_g, d_dg, d_vt, d_gc, singular_frame, (hipStream_t)stream);
}

template <bool DEV>
static int64_t lpc_body(const void* x, int x_dtype, int64_t n, const double* wind, int nwind, int hop, int64_t nfr, int order, double* coef,
                        int64_t* singular_frame, hipStream_t s) {
    if (singular_frame) *singular_frame = -1;
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    t_iaif_kernels = "";
    if ((rc = lpc_frames_args("pvx_lpc", x_dtype, n, nwind, hop, nfr)) != PVX_OK) return rc;
    if (order < 0) { pvx_set_error("bad pvx_lpc argument"); return PVX_ERR_INVALID; }
    if (nwind > PVX_LPC_MAX_NWIND || order > PVX_LPC_MAX_ORDER) {
        pvx_set_error("pvx_lpc: nwind %d, order %d: the kernel takes nwind <= %d and orders <= %d", nwind, order, PVX_LPC_MAX_NWIND, PVX_LPC_MAX_ORDER);
        return PVX_ERR_UNSUPPORTED;
    }
    if (nfr == 0) return 0;
    if (!x || !coef) { pvx_set_error("null pvx_lpc signal or output"); return PVX_ERR_INVALID; }
    const size_t es = dtype_size(x_dtype), limit = pvx_device_bytes_limit(kIaifLimit), rb = (size_t)(order + 1) * 8;
    int64_t fc = nfr;
    DevMem dx, dc;
    if (!DEV) {                                                       // whole frames per chunk; the device form reads and writes in place
        fc = (int64_t)(limit / es) > nwind ? ((int64_t)(limit / es) - nwind) / hop + 1 : 1;
        fc = std::min(nfr, std::min<int64_t>(fc, std::max<int64_t>(1, (int64_t)(limit / rb))));
        if ((rc = dx.alloc((size_t)((fc - 1) * hop + nwind) * es)) != PVX_OK || (rc = dc.alloc((size_t)fc * rb)) != PVX_OK) return rc;
    }
    for (int64_t f0 = 0; f0 < nfr; f0 += fc) {
        const int64_t cnt = std::min(fc, nfr - f0);
        const void* cx = (const char*)x + (size_t)(f0 * hop) * es;
        if (!DEV) {
            if ((rc = pvx_host_to_device(dx.get(), cx, (size_t)((cnt - 1) * hop + nwind) * es)) != PVX_OK) return rc;
            cx = dx.get();
        }
        int64_t sing = -1;
        if ((rc = pvx_lpc_run(cx, x_dtype, cnt, wind, nwind, hop, order, DEV ? coef + (size_t)f0 * (order + 1) : dc.as<double>(), &sing, s,
                              &t_iaif_kernels)) != PVX_OK) return rc;   // synchronises the stream
        if (sing >= 0) {
            if (singular_frame) *singular_frame = f0 + sing;
            pvx_set_error("pvx_lpc: frame %lld: Singular principal minor (a prediction error of exactly 0)", (long long)(f0 + sing));
            return PVX_ERR_SINGULAR;
        }
        if (!DEV && (rc = pvx_device_to_host((char*)coef + (size_t)f0 * rb, dc.get(), (size_t)cnt * rb)) != PVX_OK) return rc;
    }
    return nfr;
}

extern "C" int64_t pvx_lpc(const void* x, int x_dtype, int64_t n, const double* wind, int nwind, int hop, int64_t nfr, int order, double* coef,
                           int64_t* singular_frame) {
    return lpc_body<false>(x, x_dtype, n, wind, nwind, hop, nfr, order, coef, singular_frame, nullptr);
}

extern "C" int64_t pvx_lpc_dev(const void* d_x, int x_dtype, int64_t n, const double* wind, int nwind, int hop, int64_t nfr, int order,
                               double* d_coef, int64_t* singular_frame, void* stream) {
    return lpc_body<true>(d_x, x_dtype, n, wind, nwind, hop, nfr, order, d_coef, singular_frame, (hipStream_t)stream);
}

// ---- formants and polynomial roots (k_formant.hip) -------------------------------
static thread_local const char* t_formants_kernels = "";
extern "C" const char* pvx_formants_last_kernels(void) { return t_formants_kernels; }

// Frames in groups sized by PVX_MAX_DEVICE_BYTES (per buffer, as iaif_body): a group decimates the samples its own frames read
// and nothing else.  A decimated sample's value depends on its index and the signal alone, a frame's on its samples alone: the
// bits are those of one group.
template <bool DEV>
static int64_t formants_body(const void* x, int x_dtype, int64_t n, int preemph, int down, const double* taps, int ntaps, const double* wind,
                             int nwind, int hop, int64_t nfr, int order, double fs, int32_t* nkept, double* freq, double* bw, double* re,
                             double* im, double* lpc, int64_t* singular_frame, int64_t* noconv_row, hipStream_t s) {
    if (singular_frame) *singular_frame = -1;
    if (noconv_row) *noconv_row = -1;
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    t_formants_kernels = "";
    if (down < 1 || n < 0 || n > INT64_MAX - down) { pvx_set_error("bad pvx_formants argument"); return PVX_ERR_INVALID; }
    const int64_t nd = (n + down - 1) / down;                         // the decimated signal: ceil(n / down) samples
    if ((rc = lpc_frames_args("pvx_formants", x_dtype, nd, nwind, hop, nfr)) != PVX_OK) return rc;
    if (!wind || order < 1 || (down > 1 && (!taps || ntaps < 1 || ntaps % 2 == 0))) {
        pvx_set_error("bad pvx_formants argument (order >= 1, a window, and an odd number of taps at down > 1)");
        return PVX_ERR_INVALID;
    }
    if (nwind > PVX_LPC_MAX_NWIND || order > PVX_ROOTS_MAX_ORDER) {
        pvx_set_error("pvx_formants: nwind %d, order %d: the kernel takes nwind <= %d and orders <= %d", nwind, order, PVX_LPC_MAX_NWIND,
                      PVX_ROOTS_MAX_ORDER);
        return PVX_ERR_UNSUPPORTED;
    }
    if (nfr == 0) return 0;
    if (!x) { pvx_set_error("null pvx_formants signal"); return PVX_ERR_INVALID; }
    const size_t es = dtype_size(x_dtype), limit = pvx_device_bytes_limit(kIaifLimit);
    const int nt = down > 1 ? ntaps : 1, half = (nt - 1) / 2;
    // samples a group of k frames reads: ((k - 1) hop + nwind - 1) down + nt + 1 (the last one for the difference)
    const int64_t span1 = (int64_t)(nwind - 1) * down + nt + 1, step = (int64_t)hop * down;
    int64_t cap = (int64_t)(limit / 8) > nwind ? ((int64_t)(limit / 8) - nwind) / hop + 1 : 1;
    cap = std::min<int64_t>(cap, (int64_t)(limit / es) > span1 ? ((int64_t)(limit / es) - span1) / step + 1 : 1);
    const int64_t own = std::min(nfr, std::max<int64_t>(1, cap));
    const size_t P = (size_t)order;
    DevMem dx, dy, wk, wf, wb, wr, wi, wl;
    if ((rc = dy.alloc((size_t)((own - 1) * hop + nwind) * 8)) != PVX_OK) return rc;
    if (!DEV) {
        if ((rc = dx.alloc((size_t)std::min<int64_t>(n, (own - 1) * step + span1) * es)) != PVX_OK || (rc = wk.alloc((size_t)own * 4)) != PVX_OK ||
            (rc = wf.alloc((size_t)own * P * 8)) != PVX_OK || (rc = wb.alloc((size_t)own * P * 8)) != PVX_OK ||
            (rc = wr.alloc((size_t)own * P * 8)) != PVX_OK || (rc = wi.alloc((size_t)own * P * 8)) != PVX_OK ||
            (rc = wl.alloc((size_t)own * (P + 1) * 8)) != PVX_OK) return rc;
    }
    const FormantCall call = {x_dtype, n, preemph != 0, down, nt, nwind, hop, order, fs, taps, wind};
    for (int64_t fa = 0; fa < nfr; fa += own) {
        const int64_t nf = std::min(own, nfr - fa);
        const int64_t m0 = fa * hop, m1 = m0 + (nf - 1) * hop + nwind;
        const int64_t lo = std::max<int64_t>(0, m0 * down - half), hi = std::min<int64_t>(n, (m1 - 1) * down - half + nt + 1);
        const void* cx = x;
        int64_t x0 = 0;
        if (!DEV) {
            if ((rc = pvx_host_to_device(dx.get(), (const char*)x + (size_t)lo * es, (size_t)(hi - lo) * es)) != PVX_OK) return rc;
            cx = dx.get();
            x0 = lo;
        }
        const size_t r0 = (size_t)fa;
        const FormantRows rows = DEV ? FormantRows{nkept ? nkept + r0 : nullptr, freq ? freq + r0 * P : nullptr, bw ? bw + r0 * P : nullptr,
                                                   re ? re + r0 * P : nullptr, im ? im + r0 * P : nullptr, lpc ? lpc + r0 * (P + 1) : nullptr}
                                     : FormantRows{wk.as<int>(), wf.as<double>(), wb.as<double>(), wr.as<double>(), wi.as<double>(), wl.as<double>()};
        int64_t sing = -1, noc = -1;
        if ((rc = pvx_formants_run(call, cx, x0, fa, nf, dy.as<double>(), rows, &sing, &noc, s, &t_formants_kernels)) != PVX_OK) return rc;
        if (sing >= 0) {
            if (singular_frame) *singular_frame = fa + sing;
            pvx_set_error("pvx_formants: frame %lld: Singular principal minor (a prediction error of exactly 0)", (long long)(fa + sing));
            return PVX_ERR_SINGULAR;
        }
        if (noc >= 0) {
            if (noconv_row) *noconv_row = fa + noc;
            pvx_set_error("pvx_formants: frame %lld: the root iteration met its bound of iterations", (long long)(fa + noc));
            return PVX_ERR_NOCONV;
        }
        if (!DEV) {
            const size_t k = (size_t)nf;
            if ((nkept && (rc = pvx_device_to_host(nkept + r0, wk.get(), k * 4)) != PVX_OK) ||
                (freq && (rc = pvx_device_to_host(freq + r0 * P, wf.get(), k * P * 8)) != PVX_OK) ||
                (bw && (rc = pvx_device_to_host(bw + r0 * P, wb.get(), k * P * 8)) != PVX_OK) ||
                (re && (rc = pvx_device_to_host(re + r0 * P, wr.get(), k * P * 8)) != PVX_OK) ||
                (im && (rc = pvx_device_to_host(im + r0 * P, wi.get(), k * P * 8)) != PVX_OK) ||
                (lpc && (rc = pvx_device_to_host(lpc + r0 * (P + 1), wl.get(), k * (P + 1) * 8)) != PVX_OK)) return rc;
        }
    }
    return nfr;
}

extern "C" int64_t pvx_formants(const void* x, int x_dtype, int64_t n, int preemph, int down, const double* taps, int ntaps, const double* wind,
                                int nwind, int hop, int64_t nfr, int order, double fs, int32_t* nkept, double* freq, double* bw, double* re,
                                double* im, double* lpc, int64_t* singular_frame, int64_t* noconv_row) {
    return formants_body<false>(x, x_dtype, n, preemph, down, taps, ntaps, wind, nwind, hop, nfr, order, fs, nkept, freq, bw, re, im, lpc,
                                singular_frame, noconv_row, nullptr);
}

extern "C" int64_t pvx_formants_dev(const void* d_x, int x_dtype, int64_t n, int preemph, int down, const double* taps, int ntaps,
                                    const double* wind, int nwind, int hop, int64_t nfr, int order, double fs, int32_t* d_nkept, double* d_freq,
                                    double* d_bw, double* d_re, double* d_im, double* d_lpc, int64_t* singular_frame, int64_t* noconv_row,
                                    void* stream) {
    return formants_body<true>(d_x, x_dtype, n, preemph, down, taps, ntaps, wind, nwind, hop, nfr, order, fs, d_nkept, d_freq, d_bw, d_re, d_im,
                               d_lpc, singular_frame, noconv_row, (hipStream_t)stream);
}

template <bool DEV>
static int64_t polyroots_body(const double* coef, int64_t n, int order, double* re, double* im, int32_t* nkept, int32_t* status,
                              int64_t* noconv_row, hipStream_t s) {
    if (noconv_row) *noconv_row = -1;
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    t_formants_kernels = "";
    if (n < 0 || order < 1) { pvx_set_error("bad pvx_polyroots argument"); return PVX_ERR_INVALID; }
    if (order > PVX_ROOTS_MAX_ORDER) {
        pvx_set_error("pvx_polyroots: degree %d: the kernel takes degrees <= %d", order, PVX_ROOTS_MAX_ORDER);
        return PVX_ERR_UNSUPPORTED;
    }
    if (n == 0) return 0;
    if (!coef) { pvx_set_error("null pvx_polyroots coefficients"); return PVX_ERR_INVALID; }
    const size_t P = (size_t)order, rb = (P + 1) * 8;
    if (!DEV)
        for (int64_t i = 0; i < n; i++)
            if (coef[(size_t)i * (P + 1)] == 0.0) { pvx_set_error("pvx_polyroots: row %lld has a zero leading coefficient", (long long)i); return PVX_ERR_INVALID; }
    int64_t rc_rows = n;
    DevMem dc, wr, wi, wk, wst;
    if (!DEV) {
        rc_rows = std::min(n, std::max<int64_t>(1, (int64_t)(pvx_device_bytes_limit(kIaifLimit) / rb)));
        if ((rc = dc.alloc((size_t)rc_rows * rb)) != PVX_OK || (rc = wr.alloc((size_t)rc_rows * P * 8)) != PVX_OK ||
            (rc = wi.alloc((size_t)rc_rows * P * 8)) != PVX_OK || (rc = wk.alloc((size_t)rc_rows * 4)) != PVX_OK ||
            (rc = wst.alloc((size_t)rc_rows * 4)) != PVX_OK) return rc;
    }
    for (int64_t r0 = 0; r0 < n; r0 += rc_rows) {
        const int64_t cnt = std::min(rc_rows, n - r0);
        const size_t o = (size_t)r0, k = (size_t)cnt;
        int64_t noc = -1, lead = -1;
        if (!DEV) {
            if ((rc = pvx_host_to_device(dc.get(), coef + o * (P + 1), k * rb)) != PVX_OK) return rc;
            rc = pvx_polyroots_run(dc.as<double>(), cnt, order, wr.as<double>(), wi.as<double>(), wk.as<int>(), wst.as<int>(), &noc, &lead, s,
                                   &t_formants_kernels);
        } else {
            rc = pvx_polyroots_run(coef + o * (P + 1), cnt, order, re ? re + o * P : nullptr, im ? im + o * P : nullptr, nkept ? nkept + o : nullptr,
                                   status ? status + o : nullptr, &noc, &lead, s, &t_formants_kernels);
        }
        if (rc != PVX_OK) return rc;
        if (!DEV) {
            if ((re && (rc = pvx_device_to_host(re + o * P, wr.get(), k * P * 8)) != PVX_OK) ||
                (im && (rc = pvx_device_to_host(im + o * P, wi.get(), k * P * 8)) != PVX_OK) ||
                (nkept && (rc = pvx_device_to_host(nkept + o, wk.get(), k * 4)) != PVX_OK) ||
                (status && (rc = pvx_device_to_host(status + o, wst.get(), k * 4)) != PVX_OK)) return rc;
        }
        if (lead >= 0) {
            pvx_set_error("pvx_polyroots: row %lld has a zero leading coefficient", (long long)(r0 + lead));
            return PVX_ERR_INVALID;
        }
        if (noc >= 0) {
            if (noconv_row) *noconv_row = r0 + noc;
            pvx_set_error("pvx_polyroots: row %lld: the root iteration met its bound of iterations", (long long)(r0 + noc));
            return PVX_ERR_NOCONV;
        }
    }
    return n;
}

extern "C" int64_t pvx_polyroots(const double* coef, int64_t n, int order, double* re, double* im, int32_t* nkept, int32_t* status,
                                 int64_t* noconv_row) {
    return polyroots_body<false>(coef, n, order, re, im, nkept, status, noconv_row, nullptr);
}

extern "C" int64_t pvx_polyroots_dev(const double* d_coef, int64_t n, int order, double* d_re, double* d_im, int32_t* d_nkept, int32_t* d_status,
                                     int64_t* noconv_row, void* stream) {
    return polyroots_body<true>(d_coef, n, order, d_re, d_im, d_nkept, d_status, noconv_row, (hipStream_t)stream);
}

// ---- LPC spectral envelopes and refined peaks (k_lpcenv.hip) -------------------------------
static thread_local const char* t_envelope_kernels = "";
extern "C" const char* pvx_envelope_last_kernels(void) { return t_envelope_kernels; }

static int envelope_limits(const char* what, int64_t n, int order, int npts, int maxpk) {
    if (order < 1 || order > PVX_ROOTS_MAX_ORDER || npts < 1 || npts > PVX_ENV_MAX_NPTS) {
        pvx_set_error("%s: order %d, npts %d: the kernel takes orders 1 .. %d and 3 .. %d points", what, order, npts, PVX_ROOTS_MAX_ORDER,
                      PVX_ENV_MAX_NPTS);
        return PVX_ERR_UNSUPPORTED;
    }
    if (npts < 3 || n < 0 || maxpk < 0) { pvx_set_error("bad %s argument (npts >= 3, n >= 0, maxpk >= 0)", what); return PVX_ERR_INVALID; }
    return PVX_OK;
}

// the device lists of a group of rows of a host call, and their way back
struct PeakLists {
    DevMem k, i, p, v;
    int alloc(size_t rows, size_t maxpk, bool npk, bool idx, bool pos, bool val) {
        int rc;
        if ((npk && (rc = k.alloc(rows * 4)) != PVX_OK) || (idx && (rc = i.alloc(rows * maxpk * 4)) != PVX_OK) ||
            (pos && (rc = p.alloc(rows * maxpk * 8)) != PVX_OK) || (val && (rc = v.alloc(rows * maxpk * 8)) != PVX_OK)) return rc;
        return PVX_OK;
    }
};

static int peak_lists_to_host(const PeakLists& d, size_t o, size_t k, size_t maxpk, int32_t* npk, int32_t* idx, double* pos, double* val) {
    int rc;
    if ((npk && (rc = pvx_device_to_host(npk + o, d.k.get(), k * 4)) != PVX_OK) ||
        (idx && maxpk && (rc = pvx_device_to_host(idx + o * maxpk, d.i.get(), k * maxpk * 4)) != PVX_OK) ||
        (pos && maxpk && (rc = pvx_device_to_host(pos + o * maxpk, d.p.get(), k * maxpk * 8)) != PVX_OK) ||
        (val && maxpk && (rc = pvx_device_to_host(val + o * maxpk, d.v.get(), k * maxpk * 8)) != PVX_OK)) return rc;
    return PVX_OK;
}

// Rows in groups sized by PVX_MAX_DEVICE_BYTES (per buffer, as polyroots_body): a row's bits depend on the row alone.
template <bool DEV>
static int64_t lpc_envelope_body(const double* coef, int64_t n, int order, int npts, double fs, int maxpk, double* env, int32_t* npk,
                                 int32_t* idx, double* pos, double* val, int64_t* overflow_row, hipStream_t s) {
    if (overflow_row) *overflow_row = -1;
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    t_envelope_kernels = "";
    if ((rc = envelope_limits("pvx_lpc_envelope", n, order, npts, maxpk)) != PVX_OK) return rc;
    if (n == 0) return 0;
    if (!coef) { pvx_set_error("null pvx_lpc_envelope coefficients"); return PVX_ERR_INVALID; }
    const size_t P = (size_t)order, N = (size_t)npts, K = (size_t)maxpk, rb = (P + 1) * 8;
    if (!DEV)
        for (int64_t i = 0; i < n; i++)
            if (coef[(size_t)i * (P + 1)] == 0.0) { pvx_set_error("pvx_lpc_envelope: row %lld has a zero leading coefficient", (long long)i); return PVX_ERR_INVALID; }
    int64_t own = n;
    DevMem dc, de;
    PeakLists dl;
    if (!DEV) {
        own = std::min(n, std::max<int64_t>(1, (int64_t)(pvx_device_bytes_limit(kIaifLimit) / std::max(std::max(rb, K * 8), env ? N * 8 : (size_t)8))));
        if ((rc = dc.alloc((size_t)own * rb)) != PVX_OK || (env && (rc = de.alloc((size_t)own * N * 8)) != PVX_OK) ||
            (rc = dl.alloc((size_t)own, K, npk != nullptr, idx != nullptr, pos != nullptr, val != nullptr)) != PVX_OK) return rc;
    }
    for (int64_t r0 = 0; r0 < n; r0 += own) {
        const int64_t cnt = std::min(own, n - r0);
        const size_t o = (size_t)r0, k = (size_t)cnt;
        int64_t over = -1, bad = -1;
        if (!DEV) {
            if ((rc = pvx_host_to_device(dc.get(), coef + o * (P + 1), k * rb)) != PVX_OK) return rc;
            rc = pvx_lpcenv_run(dc.as<double>(), cnt, order, npts, fs, maxpk, env ? de.as<double>() : nullptr, npk ? dl.k.as<int>() : nullptr,
                                idx ? dl.i.as<int>() : nullptr, pos ? dl.p.as<double>() : nullptr, val ? dl.v.as<double>() : nullptr, &over, &bad,
                                s, &t_envelope_kernels);
        } else {
            rc = pvx_lpcenv_run(coef + o * (P + 1), cnt, order, npts, fs, maxpk, env ? env + o * N : nullptr, npk ? npk + o : nullptr,
                                idx ? idx + o * K : nullptr, pos ? pos + o * K : nullptr, val ? val + o * K : nullptr, &over, &bad, s,
                                &t_envelope_kernels);
        }
        if (rc != PVX_OK) return rc;
        if (!DEV) {
            if ((env && (rc = pvx_device_to_host(env + o * N, de.get(), k * N * 8)) != PVX_OK) ||
                (rc = peak_lists_to_host(dl, o, k, K, npk, idx, pos, val)) != PVX_OK) return rc;
        }
        if (bad >= 0) {
            pvx_set_error("pvx_lpc_envelope: row %lld has a zero leading coefficient", (long long)(r0 + bad));
            return PVX_ERR_INVALID;
        }
        if (over >= 0) {
            if (overflow_row) *overflow_row = r0 + over;
            pvx_set_error("pvx_lpc_envelope: row %lld has more than maxpk = %d peaks", (long long)(r0 + over), maxpk);
            return PVX_ERR_SIZE;
        }
    }
    return n;
}

extern "C" int64_t pvx_lpc_envelope(const double* coef, int64_t n, int order, int npts, double fs, int maxpk, double* env, int32_t* npk,
                                    int32_t* idx, double* pos, double* val, int64_t* overflow_row) {
    return lpc_envelope_body<false>(coef, n, order, npts, fs, maxpk, env, npk, idx, pos, val, overflow_row, nullptr);
}

extern "C" int64_t pvx_lpc_envelope_dev(const double* d_coef, int64_t n, int order, int npts, double fs, int maxpk, double* d_env,
                                        int32_t* d_npk, int32_t* d_idx, double* d_pos, double* d_val, int64_t* overflow_row, void* stream) {
    return lpc_envelope_body<true>(d_coef, n, order, npts, fs, maxpk, d_env, d_npk, d_idx, d_pos, d_val, overflow_row, (hipStream_t)stream);
}

template <bool DEV>
static int64_t peaks_refine_body(const double* y, int64_t n, int npts, const double* x, int maxpk, const int32_t* sel, int32_t* npk,
                                 int32_t* idx, double* pos, double* val, int64_t* overflow_row, hipStream_t s) {
    if (overflow_row) *overflow_row = -1;
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    t_envelope_kernels = "";
    if ((rc = envelope_limits("pvx_peaks_refine", n, 1, npts, maxpk)) != PVX_OK) return rc;
    if (n == 0) return 0;
    if (!y) { pvx_set_error("null pvx_peaks_refine rows"); return PVX_ERR_INVALID; }
    const size_t N = (size_t)npts, K = (size_t)maxpk;
    if (!DEV && sel)
        for (size_t t = 0; t < (size_t)n * K; t++)
            if (sel[t] != -1 && (sel[t] < 1 || sel[t] > npts - 2)) {
                pvx_set_error("pvx_peaks_refine: row %lld: index %d is outside 1 .. npts - 2", (long long)(t / K), (int)sel[t]);
                return PVX_ERR_INVALID;
            }
    int64_t own = n;
    DevMem dy, dx, ds;
    PeakLists dl;
    if (!DEV) {
        own = std::min(n, std::max<int64_t>(1, (int64_t)(pvx_device_bytes_limit(kIaifLimit) / std::max(N * 8, K * 8))));
        if ((rc = dy.alloc((size_t)own * N * 8)) != PVX_OK || (x && (rc = dx.alloc(N * 8)) != PVX_OK) ||
            (sel && (rc = ds.alloc((size_t)own * K * 4)) != PVX_OK) ||
            (rc = dl.alloc((size_t)own, K, npk != nullptr, idx != nullptr, pos != nullptr, val != nullptr)) != PVX_OK) return rc;
        if (x && (rc = pvx_host_to_device(dx.get(), x, N * 8)) != PVX_OK) return rc;
    }
    for (int64_t r0 = 0; r0 < n; r0 += own) {
        const int64_t cnt = std::min(own, n - r0);
        const size_t o = (size_t)r0, k = (size_t)cnt;
        int64_t over = -1, bad = -1;
        if (!DEV) {
            if ((rc = pvx_host_to_device(dy.get(), y + o * N, k * N * 8)) != PVX_OK ||
                (sel && K && (rc = pvx_host_to_device(ds.get(), sel + o * K, k * K * 4)) != PVX_OK)) return rc;
            rc = pvx_peaks_refine_run(dy.as<double>(), cnt, npts, x ? dx.as<double>() : nullptr, maxpk, sel ? ds.as<int>() : nullptr,
                                      npk ? dl.k.as<int>() : nullptr, idx ? dl.i.as<int>() : nullptr, pos ? dl.p.as<double>() : nullptr,
                                      val ? dl.v.as<double>() : nullptr, &over, &bad, s, &t_envelope_kernels);
        } else {
            rc = pvx_peaks_refine_run(y + o * N, cnt, npts, x, maxpk, sel ? sel + o * K : nullptr, npk ? npk + o : nullptr,
                                      idx ? idx + o * K : nullptr, pos ? pos + o * K : nullptr, val ? val + o * K : nullptr, &over, &bad, s,
                                      &t_envelope_kernels);
        }
        if (rc != PVX_OK) return rc;
        if (!DEV && (rc = peak_lists_to_host(dl, o, k, K, npk, idx, pos, val)) != PVX_OK) return rc;
        if (bad >= 0) {
            pvx_set_error("pvx_peaks_refine: row %lld: a given index is outside 1 .. npts - 2", (long long)(r0 + bad));
            return PVX_ERR_INVALID;
        }
        if (over >= 0) {
            if (overflow_row) *overflow_row = r0 + over;
            pvx_set_error("pvx_peaks_refine: row %lld has more than maxpk = %d peaks", (long long)(r0 + over), maxpk);
            return PVX_ERR_SIZE;
        }
    }
    return n;
}

extern "C" int64_t pvx_peaks_refine(const double* y, int64_t n, int npts, const double* x, int maxpk, const int32_t* sel, int32_t* npk,
                                    int32_t* idx, double* pos, double* val, int64_t* overflow_row) {
    return peaks_refine_body<false>(y, n, npts, x, maxpk, sel, npk, idx, pos, val, overflow_row, nullptr);
}

extern "C" int64_t pvx_peaks_refine_dev(const double* d_y, int64_t n, int npts, const double* d_x, int maxpk, const int32_t* d_sel,
                                        int32_t* d_npk, int32_t* d_idx, double* d_pos, double* d_val, int64_t* overflow_row, void* stream) {
    return peaks_refine_body<true>(d_y, n, npts, d_x, maxpk, d_sel, d_npk, d_idx, d_pos, d_val, overflow_row, (hipStream_t)stream);
}

// ---- speech segmentation on band energies (k_segment.hip) ----------------------------------
static thread_local const char* t_segment_kernels = "";
extern "C" const char* pvx_segment_last_kernels(void) { return t_segment_kernels; }

static int seg_bands(const char* what, int nband) {
    if (nband < 1) { pvx_set_error("%s: a table without bands", what); return PVX_ERR_INVALID; }
    if (nband > PVX_FBANK_MAX_NBAND) { pvx_set_error("%s: %d bands (the kernels take up to %d)", what, nband, PVX_FBANK_MAX_NBAND); return PVX_ERR_UNSUPPORTED; }
    return PVX_OK;
}

template <bool DEV>
static int64_t seg_detect_body(const double* spec, int64_t nfr, int nband, double thresh, int maxseg, double* det, int32_t* idx, double* fpos,
                               int64_t* count, hipStream_t s) {
    if (count) *count = 0;
    int rc;                                                          // (arguments first: the limits answer without a device too)
    t_segment_kernels = "";
    if ((rc = seg_bands("pvx_seg_detect", nband)) != PVX_OK) return rc;
    if (nfr < 1 || nfr > 0x7fffffffLL || maxseg < 0) { pvx_set_error("bad pvx_seg_detect argument (1 <= nfr < 2^31, maxseg >= 0)"); return PVX_ERR_INVALID; }
    if (!spec) { pvx_set_error("null pvx_seg_detect table"); return PVX_ERR_INVALID; }
    if ((rc = pvx_require_device()) != PVX_OK) return rc;
    if (nfr < 2) return 0;
    const size_t nd = (size_t)nfr - 1, K = (size_t)maxseg;
    int64_t total = 0;
    if (DEV) {
        if ((rc = pvx_seg_detect_run(spec, nfr, nband, thresh, maxseg, det, idx, fpos, &total, s, &t_segment_kernels)) != PVX_OK) return rc;
    } else {
        DevMem ds, dd, di, dp;
        const size_t sb = (size_t)nfr * nband * 8;
        if ((rc = ds.alloc(sb)) != PVX_OK || (det && (rc = dd.alloc(nd * 8)) != PVX_OK) || (idx && (rc = di.alloc(K * 4)) != PVX_OK) ||
            (fpos && (rc = dp.alloc(K * 8)) != PVX_OK)) return rc;
        if ((rc = pvx_host_to_device(ds.get(), spec, sb)) != PVX_OK) return rc;
        if ((rc = pvx_seg_detect_run(ds.as<double>(), nfr, nband, thresh, maxseg, det ? dd.as<double>() : nullptr, idx ? di.as<int>() : nullptr,
                                     fpos ? dp.as<double>() : nullptr, &total, s, &t_segment_kernels)) != PVX_OK) return rc;
        const size_t got = (size_t)std::min<int64_t>(total, maxseg);
        if ((det && (rc = pvx_device_to_host(det, dd.get(), nd * 8)) != PVX_OK) || (idx && got && (rc = pvx_device_to_host(idx, di.get(), got * 4)) != PVX_OK) ||
            (fpos && got && (rc = pvx_device_to_host(fpos, dp.get(), got * 8)) != PVX_OK)) return rc;
    }
    if (count) *count = total;
    if (total > maxseg && (idx || fpos)) {
        pvx_set_error("pvx_seg_detect: %lld peaks above the threshold, the lists hold maxseg = %d", (long long)total, maxseg);
        return PVX_ERR_SIZE;
    }
    return std::min<int64_t>(total, maxseg);
}

extern "C" int64_t pvx_seg_detect(const double* spec, int64_t nfr, int nband, double thresh, int maxseg, double* det, int32_t* idx, double* fpos,
                                  int64_t* count) {
    return seg_detect_body<false>(spec, nfr, nband, thresh, maxseg, det, idx, fpos, count, nullptr);
}

extern "C" int64_t pvx_seg_detect_dev(const double* d_spec, int64_t nfr, int nband, double thresh, int maxseg, double* d_det, int32_t* d_idx,
                                      double* d_fpos, int64_t* count, void* stream) {
    return seg_detect_body<true>(d_spec, nfr, nband, thresh, maxseg, d_det, d_idx, d_fpos, count, (hipStream_t)stream);
}

template <bool DEV>
static int64_t seg_refine_body(const double* spec, int64_t nfine, int nband, const int32_t* ranges, const double* tseg, int64_t nseg, int hop,
                               double half, double tsr, double sr, double thr, int has_thr, double* valb, double* vala, int32_t* cross, double* out,
                               hipStream_t s) {
    int rc;
    t_segment_kernels = "";
    if ((rc = seg_bands("pvx_seg_refine", nband)) != PVX_OK) return rc;
    if (nfine < 0 || nfine > 0x7fffffffLL || nseg < 0 || hop < 1) { pvx_set_error("bad pvx_seg_refine argument (0 <= nfine < 2^31, nseg >= 0, hop >= 1)"); return PVX_ERR_INVALID; }
    if (nseg == 0) return 0;
    if (!ranges || !tseg || (nfine > 0 && !spec)) { pvx_set_error("null pvx_seg_refine table"); return PVX_ERR_INVALID; }
    for (int64_t i = 0; i < nseg; i++) {
        const int32_t* r = ranges + i * 6;
        const bool inside = r[4] >= 0 && r[4] <= r[5] && r[5] <= nfine && r[0] >= r[4] && r[0] <= r[1] && r[1] <= r[5] && r[2] >= r[4] &&
                            r[2] <= r[3] && r[3] <= r[5];
        if (!inside) { pvx_set_error("pvx_seg_refine: segment %lld: a range outside 0 .. nfine, or a side outside iall", (long long)i); return PVX_ERR_INVALID; }
        if (r[1] - r[0] > PVX_SEG_MAX_SIDE || r[3] - r[2] > PVX_SEG_MAX_SIDE || r[5] - r[4] > 2 * PVX_SEG_MAX_SIDE + 1) {
            pvx_set_error("pvx_seg_refine: segment %lld: a side of more than %d frames (or an iall of more than %d)", (long long)i,
                          PVX_SEG_MAX_SIDE, 2 * PVX_SEG_MAX_SIDE + 1);
            return PVX_ERR_UNSUPPORTED;
        }
    }
    if ((rc = pvx_require_device()) != PVX_OK) return rc;
    if (DEV) {
        if ((rc = pvx_seg_refine_run(spec, nfine, nband, ranges, tseg, nseg, hop, half, tsr, sr, thr, has_thr, valb, vala, cross, out, s,
                                     &t_segment_kernels)) != PVX_OK) return rc;
        return nseg;
    }
    DevMem ds, db, da, dc, dout;
    const size_t sb = (size_t)nfine * nband * 8, cells = (size_t)nseg * nband;
    if ((rc = ds.alloc(sb)) != PVX_OK || (valb && (rc = db.alloc(cells * 8)) != PVX_OK) || (vala && (rc = da.alloc(cells * 8)) != PVX_OK) ||
        (cross && (rc = dc.alloc(cells * 4)) != PVX_OK) || (out && (rc = dout.alloc((size_t)nseg * 8)) != PVX_OK)) return rc;
    if (sb && (rc = pvx_host_to_device(ds.get(), spec, sb)) != PVX_OK) return rc;
    if ((rc = pvx_seg_refine_run(ds.as<double>(), nfine, nband, ranges, tseg, nseg, hop, half, tsr, sr, thr, has_thr, valb ? db.as<double>() : nullptr,
                                 vala ? da.as<double>() : nullptr, cross ? dc.as<int>() : nullptr, out ? dout.as<double>() : nullptr, s,
                                 &t_segment_kernels)) != PVX_OK) return rc;
    if ((valb && (rc = pvx_device_to_host(valb, db.get(), cells * 8)) != PVX_OK) || (vala && (rc = pvx_device_to_host(vala, da.get(), cells * 8)) != PVX_OK) ||
        (cross && (rc = pvx_device_to_host(cross, dc.get(), cells * 4)) != PVX_OK) || (out && (rc = pvx_device_to_host(out, dout.get(), (size_t)nseg * 8)) != PVX_OK)) return rc;
    return nseg;
}

extern "C" int64_t pvx_seg_refine(const double* spec, int64_t nfine, int nband, const int32_t* ranges, const double* tseg, int64_t nseg, int hop,
                                  double half, double tsr, double sr, double thr, int has_thr, double* valb, double* vala, int32_t* cross,
                                  double* out) {
    return seg_refine_body<false>(spec, nfine, nband, ranges, tseg, nseg, hop, half, tsr, sr, thr, has_thr, valb, vala, cross, out, nullptr);
}

extern "C" int64_t pvx_seg_refine_dev(const double* d_spec, int64_t nfine, int nband, const int32_t* ranges, const double* tseg, int64_t nseg,
                                      int hop, double half, double tsr, double sr, double thr, int has_thr, double* d_valb, double* d_vala,
                                      int32_t* d_cross, double* d_out, void* stream) {
    return seg_refine_body<true>(d_spec, nfine, nband, ranges, tseg, nseg, hop, half, tsr, sr, thr, has_thr, d_valb, d_vala, d_cross, d_out,
                                 (hipStream_t)stream);
}

template <bool DEV>
static int64_t seg_transitions_body(const double* v, int64_t nser, int n, int64_t row_stride, int64_t elem_stride, double escale, const double* tx,
                                    int64_t tx_stride, const double* trt, int mode, double pct, double thr, double* ttr, double* vbef, double* vaft,
                                    int32_t* status, hipStream_t s) {
    int rc;
    t_segment_kernels = "";
    if (n > PVX_SEG_MAX_SERIES) { pvx_set_error("pvx_seg_transitions: series of %d points (the kernel takes up to %d)", n, PVX_SEG_MAX_SERIES); return PVX_ERR_UNSUPPORTED; }
    if (nser < 0 || n < 1 || row_stride < 0 || elem_stride < 1 || !(escale >= 0.0) || (tx_stride != 0 && tx_stride != n) || mode < PVX_SEG_MINMAX ||
        mode > PVX_SEG_PCT || !(pct >= 0.0 && pct <= 100.0)) {
        pvx_set_error("bad pvx_seg_transitions argument (nser >= 0, n >= 1, strides, escale >= 0, tx_stride 0 or n, a known mode, 0 <= pct <= 100)");
        return PVX_ERR_INVALID;
    }
    if (nser == 0) return 0;
    if (!v || !tx || !trt || !ttr || !vbef || !vaft || !status) { pvx_set_error("null pvx_seg_transitions array"); return PVX_ERR_INVALID; }
    for (int64_t r = 0; r < (tx_stride ? nser : 1); r++)
        for (int k = 0; k + 1 < n; k++)
            if (!(tx[r * n + k] <= tx[r * n + k + 1])) { pvx_set_error("pvx_seg_transitions: tx must ascend (row %lld, point %d)", (long long)r, k); return PVX_ERR_INVALID; }
    if ((rc = pvx_require_device()) != PVX_OK) return rc;
    if (DEV) {
        if ((rc = pvx_seg_transitions_run(v, nser, n, row_stride, elem_stride, escale, tx, tx_stride, trt, mode, pct, thr, ttr, vbef, vaft, status, s,
                                          &t_segment_kernels)) != PVX_OK) return rc;
        return nser;
    }
    const size_t span = (size_t)(nser - 1) * row_stride + (size_t)(n - 1) * elem_stride + 1, ob = (size_t)nser * 8;
    DevMem dv, d1, d2, d3, d4;
    if ((rc = dv.alloc(span * 8)) != PVX_OK || (rc = d1.alloc(ob)) != PVX_OK || (rc = d2.alloc(ob)) != PVX_OK || (rc = d3.alloc(ob)) != PVX_OK ||
        (rc = d4.alloc((size_t)nser * 4)) != PVX_OK) return rc;
    if ((rc = pvx_host_to_device(dv.get(), v, span * 8)) != PVX_OK) return rc;
    if ((rc = pvx_seg_transitions_run(dv.as<double>(), nser, n, row_stride, elem_stride, escale, tx, tx_stride, trt, mode, pct, thr, d1.as<double>(),
                                      d2.as<double>(), d3.as<double>(), d4.as<int>(), s, &t_segment_kernels)) != PVX_OK) return rc;
    if ((rc = pvx_device_to_host(ttr, d1.get(), ob)) != PVX_OK || (rc = pvx_device_to_host(vbef, d2.get(), ob)) != PVX_OK ||
        (rc = pvx_device_to_host(vaft, d3.get(), ob)) != PVX_OK || (rc = pvx_device_to_host(status, d4.get(), (size_t)nser * 4)) != PVX_OK) return rc;
    return nser;
}

extern "C" int64_t pvx_seg_transitions(const double* v, int64_t nser, int n, int64_t row_stride, int64_t elem_stride, double escale, const double* tx,
                                       int64_t tx_stride, const double* trt, int mode, double pct, double thr, double* ttr, double* vbef,
                                       double* vaft, int32_t* status) {
    return seg_transitions_body<false>(v, nser, n, row_stride, elem_stride, escale, tx, tx_stride, trt, mode, pct, thr, ttr, vbef, vaft, status, nullptr);
}

extern "C" int64_t pvx_seg_transitions_dev(const double* d_v, int64_t nser, int n, int64_t row_stride, int64_t elem_stride, double escale,
                                           const double* tx, int64_t tx_stride, const double* trt, int mode, double pct, double thr, double* d_ttr,
                                           double* d_vbef, double* d_vaft, int32_t* d_status, void* stream) {
    return seg_transitions_body<true>(d_v, nser, n, row_stride, elem_stride, escale, tx, tx_stride, trt, mode, pct, thr, d_ttr, d_vbef, d_vaft,
                                      d_status, (hipStream_t)stream);
}

// ---- pitch jumps on rows of tracks (k_jumps.hip) --------------------------------------------
static thread_local const char* t_jumps_kernels = "";
extern "C" const char* pvx_jumps_last_kernels(void) { return t_jumps_kernels; }
const char** pvx_jumps_kernels_slot() { return &t_jumps_kernels; }

// rows, nmax and (host form) the lengths of a call: PVX_OK, or the status to return
static int jump_rows(const char* what, int64_t rows, int nmax, const int32_t* host_len) {
    if (rows < 0 || rows > 0x7fffffffLL || nmax < 0 || rows * (int64_t)nmax > 0x7fffffffLL) {   // (rows first: the product cannot overflow)
        pvx_set_error("bad %s argument (0 <= rows < 2^31, nmax >= 0, rows * nmax < 2^31)", what);
        return PVX_ERR_INVALID;
    }
    if (host_len)
        for (int64_t r = 0; r < rows; r++)
            if (host_len[r] < 0 || host_len[r] > nmax) { pvx_set_error("%s: row %lld holds %d frames of nmax = %d", what, (long long)r, host_len[r], nmax); return PVX_ERR_INVALID; }
    return PVX_OK;
}

// rows without a frame: the per-row counts (and status) are 0 and nothing is launched; returns rows
template <bool DEV>
static int64_t jump_zero_counts(int32_t* count, int32_t* status, int64_t rows, hipStream_t s) {
    const size_t bytes = (size_t)rows * 4;
    if (DEV) {
        int rc;
        if ((rc = pvx_require_device()) != PVX_OK) return rc;
        PVX_HIP_CHECK(hipMemsetAsync(count, 0, bytes, s));
        if (status) PVX_HIP_CHECK(hipMemsetAsync(status, 0, bytes, s));
        PVX_HIP_CHECK(hipStreamSynchronize(s));
    } else {
        memset(count, 0, bytes);
        if (status) memset(status, 0, bytes);
    }
    return rows;
}

template <bool DEV>
static int64_t jump_select_body(const double* mag, const double* f0, const double* t, const int32_t* len, int64_t rows, int nmax, int K, double thr,
                                double* m, int32_t* isel, double* tsel, double* fsel, int32_t* nsel, int32_t* status, hipStream_t s) {
    int rc;
    t_jumps_kernels = "";
    if (K > PVX_JUMP_MAX_K) { pvx_set_error("pvx_jump_select: %d peaks per frame (the kernel takes up to %d)", K, PVX_JUMP_MAX_K); return PVX_ERR_UNSUPPORTED; }
    if (K < 1) { pvx_set_error("bad pvx_jump_select argument (K >= 1)"); return PVX_ERR_INVALID; }
    if ((rc = jump_rows("pvx_jump_select", rows, nmax, DEV ? nullptr : len)) != PVX_OK) return rc;
    if (rows == 0) return 0;
    if (!nsel || !status || (nmax > 0 && (!mag || !f0 || !t || !m || !isel || !tsel || !fsel))) { pvx_set_error("null pvx_jump_select array"); return PVX_ERR_INVALID; }
    if (nmax == 0) return jump_zero_counts<DEV>(nsel, status, rows, s);   // no frame: nothing selected, no launch (as pvx_winstat)
    if ((rc = pvx_require_device()) != PVX_OK) return rc;
    if (DEV) {
        if ((rc = pvx_jump_select_run(mag, f0, t, len, rows, nmax, K, thr, m, isel, tsel, fsel, nsel, status, s, &t_jumps_kernels)) != PVX_OK) return rc;
        return rows;
    }
    const size_t cells = (size_t)rows * nmax;
    Staged dmag, df0, dt, dlen, dm, di, dts, dfs, dn, dst;
    if ((rc = dmag.put(mag, cells * K * 8)) != PVX_OK || (rc = df0.put(f0, cells * 8)) != PVX_OK || (rc = dt.put(t, cells * 8)) != PVX_OK ||
        (rc = dlen.put(len, (size_t)rows * 4)) != PVX_OK || (rc = dm.room(cells * 8)) != PVX_OK || (rc = di.room(cells * 4)) != PVX_OK ||
        (rc = dts.room(cells * 8)) != PVX_OK || (rc = dfs.room(cells * 8)) != PVX_OK || (rc = dn.room((size_t)rows * 4)) != PVX_OK ||
        (rc = dst.room((size_t)rows * 4)) != PVX_OK) return rc;
    if ((rc = pvx_jump_select_run(dmag.as<double>(), df0.as<double>(), dt.as<double>(), dlen.as<int>(), rows, nmax, K, thr, dm.as<double>(), di.as<int>(),
                                  dts.as<double>(), dfs.as<double>(), dn.as<int>(), dst.as<int>(), s, &t_jumps_kernels)) != PVX_OK) return rc;
    if ((rc = dm.get(m, cells * 8)) != PVX_OK || (rc = di.get(isel, cells * 4)) != PVX_OK || (rc = dts.get(tsel, cells * 8)) != PVX_OK ||
        (rc = dfs.get(fsel, cells * 8)) != PVX_OK || (rc = dn.get(nsel, (size_t)rows * 4)) != PVX_OK || (rc = dst.get(status, (size_t)rows * 4)) != PVX_OK) return rc;
    return rows;
}

extern "C" int64_t pvx_jump_select(const double* mag, const double* f0, const double* t, const int32_t* len, int64_t rows, int nmax, int K,
                                   double mag_threshold, double* m, int32_t* isel, double* tsel, double* fsel, int32_t* nsel, int32_t* status) {
    return jump_select_body<false>(mag, f0, t, len, rows, nmax, K, mag_threshold, m, isel, tsel, fsel, nsel, status, nullptr);
}

extern "C" int64_t pvx_jump_select_dev(const double* d_mag, const double* d_f0, const double* d_t, const int32_t* d_len, int64_t rows, int nmax, int K,
                                       double mag_threshold, double* d_m, int32_t* d_isel, double* d_tsel, double* d_fsel, int32_t* d_nsel,
                                       int32_t* d_status, void* stream) {
    return jump_select_body<true>(d_mag, d_f0, d_t, d_len, rows, nmax, K, mag_threshold, d_m, d_isel, d_tsel, d_fsel, d_nsel, d_status,
                                  (hipStream_t)stream);
}

template <bool DEV>
static int64_t winstat_body(const double* t, const double* x, const int32_t* len, int64_t rows, int nmax, int kind, int wl, int wr, int hop, int flags,
                            double* out, hipStream_t s) {
    int rc;
    t_jumps_kernels = "";
    if (kind < PVX_WIN_ZMEAN || kind > PVX_WIN_LINREG2 || hop < 1 || (flags & ~(PVX_WIN_USE_L | PVX_WIN_USE_R))) {
        pvx_set_error("bad pvx_winstat argument (a known kind, hop >= 1, flags of PVX_WIN_USE_L | PVX_WIN_USE_R)");
        return PVX_ERR_INVALID;
    }
    const bool right_ok = (wr >= 3 && wr <= PVX_JUMP_MAX_SIDE) || (wr == 0 && kind != PVX_WIN_LINREG2);
    if (wl < 3 || wl > PVX_JUMP_MAX_SIDE || !right_ok) {
        pvx_set_error("pvx_winstat: window sides %d and %d (the kernel takes 3 .. %d points a side; wright 0 for the kinds other than LINREG2)", wl, wr,
                      PVX_JUMP_MAX_SIDE);
        return PVX_ERR_UNSUPPORTED;
    }
    if ((rc = jump_rows("pvx_winstat", rows, nmax, DEV ? nullptr : len)) != PVX_OK) return rc;
    if (rows == 0 || nmax == 0) return rows;
    if (!t || !x || !out) { pvx_set_error("null pvx_winstat array"); return PVX_ERR_INVALID; }
    if ((rc = pvx_require_device()) != PVX_OK) return rc;
    if (DEV) {
        if ((rc = pvx_winstat_run(t, x, len, rows, nmax, kind, wl, wr, hop, flags, out, s, &t_jumps_kernels)) != PVX_OK) return rc;
        return rows;
    }
    const size_t cells = (size_t)rows * nmax;
    Staged dt, dx, dlen, dout;
    if ((rc = dt.put(t, cells * 8)) != PVX_OK || (rc = dx.put(x, cells * 8)) != PVX_OK || (rc = dlen.put(len, (size_t)rows * 4)) != PVX_OK ||
        (rc = dout.room(cells * 8)) != PVX_OK) return rc;
    if ((rc = pvx_winstat_run(dt.as<double>(), dx.as<double>(), dlen.as<int>(), rows, nmax, kind, wl, wr, hop, flags, dout.as<double>(), s,
                              &t_jumps_kernels)) != PVX_OK) return rc;
    if ((rc = dout.get(out, cells * 8)) != PVX_OK) return rc;
    return rows;
}

extern "C" int64_t pvx_winstat(const double* t, const double* x, const int32_t* len, int64_t rows, int nmax, int kind, int wleft, int wright, int hop,
                               int flags, double* out) {
    return winstat_body<false>(t, x, len, rows, nmax, kind, wleft, wright, hop, flags, out, nullptr);
}

extern "C" int64_t pvx_winstat_dev(const double* d_t, const double* d_x, const int32_t* d_len, int64_t rows, int nmax, int kind, int wleft, int wright,
                                   int hop, int flags, double* d_out, void* stream) {
    return winstat_body<true>(d_t, d_x, d_len, rows, nmax, kind, wleft, wright, hop, flags, d_out, (hipStream_t)stream);
}

template <bool DEV>
static int64_t jump_pick_body(const double* zs, const double* t, const double* x, const int32_t* len, int64_t rows, int nmax, double thr, int nsl,
                              int maxjump, int32_t* idx, int32_t* dir, int32_t* njump, double* intcpts, double* sumres, int32_t* status,
                              int64_t* overflow_row, hipStream_t s) {
    int rc;
    t_jumps_kernels = "";
    if (overflow_row) *overflow_row = -1;
    if (nsl < 1 || maxjump < 0 || rows * (int64_t)maxjump > 0x3fffffffLL) {
        pvx_set_error("bad pvx_jump_pick argument (nsl >= 1, maxjump >= 0, rows * maxjump < 2^30)");
        return PVX_ERR_INVALID;
    }
    if ((rc = jump_rows("pvx_jump_pick", rows, nmax, DEV ? nullptr : len)) != PVX_OK) return rc;
    if (rows == 0) return 0;
    if (!njump || (nmax > 0 && (!t || !x)) || (maxjump > 0 && (!idx || !intcpts || !sumres || !status)) || (zs && maxjump > 0 && !dir)) {
        pvx_set_error("null pvx_jump_pick array");
        return PVX_ERR_INVALID;
    }
    if (nmax == 0) return zs ? jump_zero_counts<DEV>(njump, nullptr, rows, s) : rows;   // no frame: no jump, no launch (lists of the caller's: nothing to fit)
    if ((rc = pvx_require_device()) != PVX_OK) return rc;
    const size_t cells = (size_t)rows * nmax, slots = (size_t)rows * maxjump;
    std::vector<int32_t> counts;
    const int32_t* got = njump;
    if (DEV) {
        if ((rc = pvx_jump_pick_run(zs, t, x, len, rows, nmax, thr, nsl, maxjump, idx, dir, njump, intcpts, sumres, status, s, &t_jumps_kernels)) != PVX_OK) return rc;
        counts.resize((size_t)rows);
        if ((rc = pvx_device_to_host(counts.data(), njump, (size_t)rows * 4)) != PVX_OK) return rc;
        got = counts.data();
    } else {
        Staged dz, dt, dx, dlen, di, dd, dn, dic, dsr, dst;
        if ((rc = dz.put(zs, cells * 8)) != PVX_OK || (rc = dt.put(t, cells * 8)) != PVX_OK || (rc = dx.put(x, cells * 8)) != PVX_OK ||
            (rc = dlen.put(len, (size_t)rows * 4)) != PVX_OK || (rc = zs ? di.room(slots * 4) : di.put(idx, slots * 4)) != PVX_OK ||
            (rc = dd.room(slots * 4)) != PVX_OK || (rc = zs ? dn.room((size_t)rows * 4) : dn.put(njump, (size_t)rows * 4)) != PVX_OK || (rc = dic.room(slots * 16)) != PVX_OK || (rc = dsr.room(slots * 16)) != PVX_OK ||
            (rc = dst.room(slots * 4)) != PVX_OK) return rc;
        if ((rc = pvx_jump_pick_run(dz.as<double>(), dt.as<double>(), dx.as<double>(), dlen.as<int>(), rows, nmax, thr, nsl, maxjump, di.as<int>(), dd.as<int>(),
                                    dn.as<int>(), dic.as<double>(), dsr.as<double>(), dst.as<int>(), s, &t_jumps_kernels)) != PVX_OK) return rc;
        // (slots beyond a row's count hold nothing: the caller reads njump[r] of them)
        if ((zs && ((rc = dn.get(njump, (size_t)rows * 4)) != PVX_OK || (rc = di.get(idx, slots * 4)) != PVX_OK || (rc = dd.get(dir, slots * 4)) != PVX_OK)) ||
            (rc = dic.get(intcpts, slots * 16)) != PVX_OK || (rc = dsr.get(sumres, slots * 16)) != PVX_OK || (rc = dst.get(status, slots * 4)) != PVX_OK) return rc;
    }
    for (int64_t r = 0; r < rows; r++)
        if (got[r] > maxjump) {
            if (overflow_row) *overflow_row = r;
            pvx_set_error("pvx_jump_pick: row %lld has %d jumps, the lists hold maxjump = %d", (long long)r, got[r], maxjump);
            return PVX_ERR_SIZE;
        }
    return rows;
}

extern "C" int64_t pvx_jump_pick(const double* zs, const double* t, const double* x, const int32_t* len, int64_t rows, int nmax, double t_threshold,
                                 int nsl, int maxjump, int32_t* idx, int32_t* dir, int32_t* njump, double* intcpts, double* sumres, int32_t* status,
                                 int64_t* overflow_row) {
    return jump_pick_body<false>(zs, t, x, len, rows, nmax, t_threshold, nsl, maxjump, idx, dir, njump, intcpts, sumres, status, overflow_row, nullptr);
}

extern "C" int64_t pvx_jump_pick_dev(const double* d_zs, const double* d_t, const double* d_x, const int32_t* d_len, int64_t rows, int nmax,
                                     double t_threshold, int nsl, int maxjump, int32_t* d_idx, int32_t* d_dir, int32_t* d_njump, double* d_intcpts,
                                     double* d_sumres, int32_t* d_status, int64_t* overflow_row, void* stream) {
    return jump_pick_body<true>(d_zs, d_t, d_x, d_len, rows, nmax, t_threshold, nsl, maxjump, d_idx, d_dir, d_njump, d_intcpts, d_sumres, d_status,
                                overflow_row, (hipStream_t)stream);
}

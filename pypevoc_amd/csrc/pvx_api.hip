// pvx_api.hip -- host side of the C ABI declared in include/pvx.h: device selection, analysis
// plans (constants of PV.__init__, pypevoc/PVAnalysis.py:72-131; rocFFT plan; device workspace),
// chunked launch sequence of run_pv (PV.py:213-264) and the host-buffer convenience wrappers.
//
// There is deliberately no CPU path in this library: every entry point needs a HIP device.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <memory>
#include <tuple>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include <time.h>

#include "pvx_internal.h"
#include "pvx_mem.h"

// float64 -> float32 while staging (RNE, what v_cvt_f32_f64 does on the device): AVX2 where the host has it
#if defined(__x86_64__)
#include <immintrin.h>
__attribute__((target("avx2"))) static void narrow_avx2(const double* src, float* dst, size_t n) {
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
        const __m128 a = _mm256_cvtpd_ps(_mm256_loadu_pd(src + i)), b = _mm256_cvtpd_ps(_mm256_loadu_pd(src + i + 4));
        _mm256_storeu_ps(dst + i, _mm256_set_m128(b, a));
    }
    for (; i < n; i++) dst[i] = (float)src[i];
}
#endif
static void narrow_f64_f32(const double* src, float* dst, size_t n) {
#if defined(__x86_64__)
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (avx2) { narrow_avx2(src, dst, n); return; }
#endif
    for (size_t i = 0; i < n; i++) dst[i] = (float)src[i];
}

// PVX_TRACE=1: host-side time stamps of the small-call paths on stderr (where a sub-millisecond round trip goes)
namespace {
struct HostTrace {
    bool on;
    const char* what;
    double t0, last;
    static double now() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3; }
    explicit HostTrace(const char* w) : on(getenv("PVX_TRACE") != nullptr), what(w), t0(0), last(0) { if (on) { t0 = last = now(); } }
    void mark(const char* label) { if (on) { const double t = now(); fprintf(stderr, "[pvx %s] %-28s +%7.1f us (%7.1f)\n", what, label, t - last, t - t0); last = t; } }
};
}  // namespace

// ---- errors ---------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

void pvx_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* pvx_last_error(void) { return g_err; }
extern "C" int pvx_version(void) { return PVX_VERSION; }

// ---- device ---------------------------------------------------------------------------------
static std::mutex g_mu;
static int g_device = -1;
static thread_local int t_device = -1;   // a worker thread of pvx_batch_run is bound to its own device (the process default stays g_device)
static bool g_fft_setup = false;
static char g_devname[256] = "";

extern "C" int pvx_init(int device) {
    std::lock_guard<std::mutex> lk(g_mu);
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        pvx_set_error("no HIP device available (%s); libpvx_hip has no CPU fallback",
                      e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
        return PVX_ERR_NO_DEVICE;
    }
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess) device = 0;
    }
    if (device >= n) { pvx_set_error("device %d out of range (%d devices)", device, n); return PVX_ERR_INVALID; }
    PVX_HIP_CHECK(hipSetDevice(device));
    hipDeviceProp_t prop;
    PVX_HIP_CHECK(hipGetDeviceProperties(&prop, device));
    snprintf(g_devname, sizeof(g_devname), "%s (%s)", prop.name, prop.gcnArchName);
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        pvx_set_error("device %d is %s; libpvx_hip carries gfx950 (MI355X) code objects only", device, prop.gcnArchName);
        return PVX_ERR_NO_DEVICE;
    }
    if (!g_fft_setup) {
        PVX_FFT_CHECK(rocfft_setup());
        g_fft_setup = true;
    }
    g_device = device;
    return PVX_OK;
}

extern "C" const char* pvx_device_name(void) { return g_devname; }
extern "C" int pvx_device(void) { return g_device; }

int pvx_require_device() {
    const int d = t_device >= 0 ? t_device : g_device;
    if (d >= 0) {
        // the calling thread may be new: bind it
        if (hipSetDevice(d) != hipSuccess) { pvx_set_error("hipSetDevice(%d) failed", d); return PVX_ERR_NO_DEVICE; }
        return PVX_OK;
    }
    return pvx_init(-1);
}

struct pvx_plan;
static int plan_device(const pvx_plan* p);
// entry points that take a plan: the thread is bound as above, and the plan must have been created under the device the
// call runs on -- its buffers, streams and events live there (a worker of pvx_batch_run creates its plan under its own
// device; anything else handing a plan of device a to a thread bound to device b is refused, not run)
int pvx_require_plan_device(const pvx_plan* p) {
    const int rc = pvx_require_device();
    if (rc != PVX_OK || !p) return rc;
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) { pvx_set_error("hipGetDevice failed"); return PVX_ERR_HIP; }
    if (cur != plan_device(p)) {
        pvx_set_error("the plan was created on device %d and is used under device %d (pvx_init / the batch worker's device): create the plan under the device that runs it",
                      plan_device(p), cur);
        return PVX_ERR_INVALID;
    }
    return PVX_OK;
}

extern "C" int64_t pvx_nframes(int64_t nsamp, int nfft, int hop) {
    // PV.py:223-249: pos = 0, hop, 2 hop, ... while pos < nsamp - nfft (strict)
    const int64_t maxpos = nsamp - nfft;
    if (maxpos <= 0 || hop <= 0 || nfft <= 0) return 0;
    return (maxpos + hop - 1) / hop;
}

// ---- plan -----------------------------------------------------------------------------------
// The analysis routes: which kernels one call of analyze_rows() runs (route_for() picks it), and pvx_plan_last_kernels' name
// of each.  The fused kernels come first.
enum class Route {
    none,
    fused, fused_mw, fused_ring, fused_rev, fused_team,   // fft modes 1 - 5: one float32 launch (k_fused*.hip)
    pv_rev, pv_team,      // float64, one launch over all rows, the spectrum rows on chip (k_pv_rev.hip, k_pv_team.hip)
    stft_pv,              // k_stft_pv.hip: window + FFT + peaks per chunk, the spectrum rows in the workspace
    stft_peaks, stft_cand_peaks,   // k_stft -> k_phase_peaks; cand: the transform hands each row's candidate peaks on
    frames_rocfft,        // k_frames -> rocFFT -> k_phase_peaks
};
static const char* const kRouteName[] = {"", "k_fused", "k_fused_mw", "k_fused_ring", "k_fused_rev", "k_fused_team", "k_pv_rev", "k_pv_team",
                                         "k_stft_pv", "k_stft+k_phase_peaks", "k_stft+k_phase_peaks", "k_frames+rocfft+k_phase_peaks"};
static_assert(sizeof(kRouteName) / sizeof(kRouteName[0]) == (size_t)Route::frames_rocfft + 1, "one name per route");
static bool is_fused(Route r) { return r >= Route::fused && r <= Route::fused_team; }

struct pvx_plan {
    int device = -1;          // the HIP device current when the plan was created: every buffer / stream / event below lives there
    double sr = 0, pkthresh = 0, wfact = 0, fstep = 0, dt = 0;
    int nfft = 0, hop = 0, npks = 0, N2 = 0, precision = 32, fft_mode = 0;
    int64_t max_rows = 0;     // rows per launch (without the halo row)
    bool rows_from_env = false;   // ... as PVX_MAX_ROWS set them
    Route general = Route::frames_rocfft;  // fft mode 0's route for the plan's shape and creation-time switches (route_for narrows
                                           // it per call); all but frames_rocfft have k_stft write d_spec (has_stft)
    Route last_route = Route::none;        // kernels of the last calls (pvx_plan_last_kernels)
    int last_rev_kc = 0;                   // k_fused_rev: the npks its instantiation had as a constant (0: the generic kernel)
    const char* last_synth = nullptr;
    std::string last_kernels;
    int64_t ldi = 0, ldo = 0; // workspace row pitches (elements / complex elements)
    std::vector<double> win;  // caller's window
    bool win_symmetric = false;  // win[n] == win[nfft-1-n] for every n
    int cand_cap = 0;            // entries per row of d_cand_y / d_cand_bin
    int64_t ws_bytes = 0;
    bool rocfft_ready = false;   // frames/spectrum workspace + rocFFT plan are created on first use
    int wire_fmt = 1;            // the gather's wire format (k_wire.hip): 1 = f as float64, 2 = the float32 it is computed from (pvx_plan_set_wire_format)
    int64_t rocfft_rows = 0;     // rows of the rocFFT workspace (2 when only pvx_stft_frames uses it)
    bool rocfft_small = false;   // ... and its output then goes to d_rspec, not to the analysis' d_spec
    int64_t harm_cap = 0;        // entries of d_hf0 / d_hprev
    // progress callback of the host entry points
    pvx_progress_fn progress_fn = nullptr;
    void* progress_user = nullptr;
    bool progress_live = false;   // inside a host entry point: chunk completions are reported
    int64_t fused_blocks = 0;    // PVX_FUSED_BLOCKS override
    int frames_per_wave = 2;     // k_phase_peaks: frames a wave handles one after the other (latency floor of a chunked launch; PVX_FPW)
    // resident results (pvx_analyze_resident): the reference's arrays stay in HBM for the tracker, the
    // resynthesis and the frame descriptors; only what the caller fetches crosses PCIe
    int64_t res_F = 0, res_nsig = 0;
    bool res_valid = false;
    size_t trk_cap = 0;                    // entries of d_pid / d_pst / d_pln
    int64_t res_P = -1, res_maxend = -1;
    unsigned sws_gen = 0;                  // calls on d_sws since it was allocated
    // optional stage timing (bench): events[4*i..4*i+3] bracket the three stages of chunk i
    bool timing = false;
    size_t ev_used = 0;
    std::vector<std::pair<int, size_t>> ev_spans;   // (stage, index of the start event; end = next event)

    // ---- what the plan owns (pvx_mem.h).  Members are destroyed last to first: the events, the rocFFT plan, the buffers, and
    // the streams at the very end.
    Stream s_host;                         // non-blocking stream of the host entry points
    Stream s_copy;                         // second stream: DMA of finished waveform slices under the next slice's kernel
    DevMem d_win;             // window / wfact in the working precision
    DevMem d_wfbin;           // double [N2]
    DevMem d_frames;          // [max_rows+1][ldi]
    DevMem d_spec;            // [max_rows+1][ldo] complex
    DevMem d_cand_y;          // the split transform's candidate peaks per workspace row (pvx_stft.h): |X|^2 [max_rows+1][cand_cap],
    DevMem d_cand_bin;        // unsigned short bins, and double [max_rows+1][4] max / min / sum / count
    DevMem d_cand_stats;
    DevMem d_rspec;           // rocFFT output when the main spectrum workspace belongs to k_stft
    DevMem d_twiddle64;       // complex<T>[nfft] W_nfft^j for k_stft (T = the plan's precision)
    DevMem d_twiddle;         // float2[2048] W_2048^j for the fused kernel
    DevMem d_specrow;         // 1024 complex float: spectrum of one requested row (fused mode)
    DevMem d_stash;           // k_fused_rev: first spectra of its waves, for the waves below them (FusedParams::stash)
    // PVHarmonic: per-frame f0 / previous-row tables and the carried spectrum of the last valid frame
    DevMem d_hf0;
    DevMem d_hx;              // pvx_harmonic_analyze: the host signal's device copy (kept: allocating and freeing hundreds of MB
                              // per call cost more than the analysis)
    DevMem d_hprev;
    DevMem d_carry;
    DevMem d_lastspec;        // k_pv_rev / k_pv_team: double [N2][2] the spectrum of the one row a call asks for (chunk carry, last_spec)
    DevMem d_pvstage;         // k_pv_rev at nfft 2048: the kept peaks' values between the frames (PvRevParams::stage)
    DevMem d_wiretmp;         // pvx_analyze_dev_wire on plans whose kernels do not write the wire format themselves: the result block that is then packed
    // host entry points: plan-owned, grow-only buffers (no hipMalloc / hipFree per call)
    DevMem d_in[2];           // input chunks (double-buffered: H2D of chunk i+1 under the kernels of chunk i)
    DevMem d_out[2];          // result blocks of a chunk when the results stream back to the host
    PinMem h_pin;             // pinned staging of small calls (input, then the result block)
    PinMem h_ring;            // pinned ring of the threaded staging of large host transfers (kStageThreads x 2 slots)
    DevMem d_prev;            // double [N2][2] spectrum carried from one input chunk to the next (PV.py:209)
    DevMem d_res;             // the resident result block
    DevMem d_pid, d_pst, d_pln;   // resident partial table (int32)
    DevMem d_tws;             // tracker workspace
    DevMem d_w;               // resynthesised waveform
    DevMem d_sws;             // resynthesis workspace (k_synth.hip)
    DevMem d_x32;             // a device-resident float64 signal narrowed for the fused float32 kernels
    DevMem d_desc;            // descriptor outputs (f0 / harmonic power)
    RealFft fft;              // with its work buffer
    Event ev_done[2];
    Event ev_ring[16];
    std::vector<Event> ev_pool;
};
static int plan_device(const pvx_plan* p) { return p->device; }
struct ProgressScope {   // progress_live until the scope ends, however it ends
    pvx_plan* const p;
    explicit ProgressScope(pvx_plan* q) : p(q) { p->progress_live = true; }
    ~ProgressScope() { p->progress_live = false; }
    ProgressScope(const ProgressScope&) = delete;
};
extern "C" int pvx_plan_device(const pvx_plan* plan) { return plan ? plan->device : PVX_ERR_INVALID; }
extern "C" const char* pvx_plan_last_kernels(const pvx_plan* plan) {
    if (!plan) return "";
    pvx_plan* p = const_cast<pvx_plan*>(plan);
    p->last_kernels.clear();
    if (p->last_route != Route::none) { p->last_kernels += "analysis="; p->last_kernels += kRouteName[(int)p->last_route]; }
    if (p->last_route == Route::fused_rev && p->last_rev_kc > 0) p->last_kernels += "<kc" + std::to_string(p->last_rev_kc) + ">";   // (npks a constant of the kernel)
    if (p->last_synth) { if (!p->last_kernels.empty()) p->last_kernels += ";"; p->last_kernels += "synth="; p->last_kernels += p->last_synth; }
    return p->last_kernels.c_str();
}

static size_t real_size(int precision) { return precision == 32 ? 4 : 8; }

#include "build_sha.inc"
extern "C" const char* pvx_build_fingerprint(void) { return PVX_BUILD_SHA; }

extern "C" int pvx_plan_destroy(pvx_plan* plan) {
    delete plan;
    return PVX_OK;
}

extern "C" int64_t pvx_plan_workspace_bytes(const pvx_plan* plan) { return plan ? plan->ws_bytes : 0; }

int pvx_resident_blocks(const void* fn, int threads, size_t lds) {
    static std::mutex mu;
    static std::map<std::tuple<int, const void*, int, size_t>, int> seen;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
    const auto key = std::make_tuple(dev, fn, threads, lds);
    std::lock_guard<std::mutex> lk(mu);
    auto it = seen.find(key);
    if (it != seen.end()) return it->second;
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, threads, lds) != hipSuccess) { (void)hipGetLastError(); nb = 0; }
    seen[key] = nb;
    return nb;
}

extern "C" int pvx_plan_set_fft_mode(pvx_plan* plan, int mode) {
    if (!plan) { pvx_set_error("null plan"); return PVX_ERR_INVALID; }
    if (mode < 0 || mode > 5) { pvx_set_error("unknown fft mode %d", mode); return PVX_ERR_INVALID; }
    if (mode == 5 && !pvx_fused_team_supported(plan->nfft, plan->precision, plan->npks)) {
        pvx_set_error("the team kernel handles nfft in {4096, 8192} at precision=32 with npks <= 128 (this plan: nfft=%d precision=%d npks=%d)", plan->nfft, plan->precision, plan->npks);
        return PVX_ERR_UNSUPPORTED;
    }
    if (mode == 4 && !pvx_fused_rev_supported(plan->nfft, plan->precision, plan->npks)) {
        pvx_set_error("the descending-order fused kernel handles nfft in {512, 1024, 2048} at precision=32 while npks leaves it enough LDS (this plan: nfft=%d precision=%d npks=%d)", plan->nfft, plan->precision, plan->npks);
        return PVX_ERR_UNSUPPORTED;
    }
    if (mode == 3 && !pvx_fused_ring_supported(plan->nfft, plan->precision, plan->npks)) {
        pvx_set_error("fft mode 3 (the ring kernel, a witness of the bit-identity tests: tests/libpvx_witness.so, not libpvx_hip.so) handles nfft in {512, 1024, 2048} at precision=32 while npks leaves it enough LDS (this plan: nfft=%d precision=%d npks=%d)", plan->nfft, plan->precision, plan->npks);
        return PVX_ERR_UNSUPPORTED;
    }
    if (mode == 2 && !pvx_fused_mw_supported(plan->nfft, plan->precision, plan->npks)) {
        pvx_set_error("fft mode 2 (several waves per frame, a witness since the general path took its cases: tests/libpvx_witness.so, not libpvx_hip.so) handles nfft in {2048, 4096, 8192} at precision=32 (this plan: nfft=%d precision=%d)", plan->nfft, plan->precision);
        return PVX_ERR_UNSUPPORTED;
    }
    if (mode == 1 && !pvx_fused_supported(plan->nfft, plan->precision, plan->npks)) {
        pvx_set_error("fft mode 1 (one wave per frame over two buffers, a witness of the bit-identity tests: tests/libpvx_witness.so, not libpvx_hip.so) handles nfft in {512, 1024, 2048} at precision=32 (this plan: nfft=%d precision=%d)", plan->nfft, plan->precision);
        return PVX_ERR_UNSUPPORTED;
    }
    plan->fft_mode = mode;
    return PVX_OK;
}

extern "C" int pvx_plan_get_fft_mode(const pvx_plan* plan) { return plan ? plan->fft_mode : PVX_ERR_INVALID; }

extern "C" int pvx_plan_create(pvx_plan** out, double sr, int nfft, int hop, int npks, double pkthresh,
                               const double* win, int precision, int64_t max_rows) {
    if (!out) { pvx_set_error("null plan pointer"); return PVX_ERR_INVALID; }
    *out = nullptr;
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    if (nfft < 4 || hop <= 0 || npks <= 0 || !(sr > 0) || (precision != 32 && precision != 64)) {
        pvx_set_error("invalid analysis parameters (sr=%g nfft=%d hop=%d npks=%d precision=%d)", sr, nfft, hop, npks, precision);
        return PVX_ERR_INVALID;
    }
    const int64_t rows_hint = max_rows;
    std::unique_ptr<pvx_plan> owner(new pvx_plan());      // an early return destroys the plan and what it holds so far
    pvx_plan* p = owner.get();
    if (hipGetDevice(&p->device) != hipSuccess) { pvx_set_error("hipGetDevice failed"); return PVX_ERR_HIP; }
    p->sr = sr; p->nfft = nfft; p->hop = hop; p->npks = npks; p->pkthresh = pkthresh;
    p->precision = precision;
    p->N2 = nfft / 2;                                   // PV.py:88
    p->win.resize(nfft);
    if (win) {
        memcpy(p->win.data(), win, sizeof(double) * nfft);
    } else {                                            // np.hanning(nfft)
        for (int i = 0; i < nfft; i++) {
            const double n = (double)(1 - nfft + 2 * i);
            p->win[i] = 0.5 + 0.5 * cos(3.141592653589793238462643383279502884 * n / (double)(nfft - 1));
        }
    }
    double wsum2 = 0.0;                                 // PV.py:99 (Python sum: left to right)
    for (int i = 0; i < nfft; i++) wsum2 = wsum2 + p->win[i] * p->win[i];
    p->win_symmetric = true;
    for (int i = 0; i < nfft / 2; i++) p->win_symmetric = p->win_symmetric && (p->win[i] == p->win[nfft - 1 - i]);
    p->wfact = sqrt(wsum2 * nfft) / 2.0;                // PV.py:102
    p->fstep = sr / (double)nfft;                       // PV.py:105
    p->dt = (double)hop / sr;                           // PV.py:108
    if (!(p->wfact > 0)) { pvx_set_error("window has no energy"); return PVX_ERR_INVALID; }

    const size_t rs = real_size(precision);
    // Launch size: the frame + spectrum workspace of one launch (~96 MiB by default) stays inside
    // the 256 MiB Infinity Cache, so rocFFT and the peak kernel read what the previous kernel just
    // wrote from on-die memory.  `max_rows` from the caller is a "rows needed" hint and only ever
    // shrinks the workspace; PVX_MAX_ROWS (environment) overrides the cap for tuning.
    int64_t cap_rows = (int64_t)(96.0 * 1024 * 1024 / ((double)nfft * rs * 2.0));
    if (cap_rows < 256) cap_rows = 256;
    if (cap_rows > 65536) cap_rows = 65536;
    if (const char* e = getenv("PVX_MAX_ROWS")) {
        const long long v = atoll(e);
        if (v >= 2) { cap_rows = (int64_t)v; p->rows_from_env = true; }
    }
    if (const char* e = getenv("PVX_FPW")) {
        const int v = atoi(e);
        if (v >= 1) p->frames_per_wave = v;
    }
    if (max_rows <= 0 || max_rows > cap_rows) max_rows = cap_rows;
    if (max_rows < 2) max_rows = 2;
    p->max_rows = max_rows;
    p->ldi = (nfft + 3) & ~3;
    p->ldo = ((nfft / 2 + 1) + 1) & ~1;                 // rocFFT writes nfft/2+1 bins; keep rows 16-byte aligned

    // device constants
    {
        std::vector<double> wf(p->N2 > 0 ? p->N2 : 1);
        const double pi2 = 2.0 * 3.141592653589793238462643383279502884;
        for (int k = 0; k < p->N2; k++) {
            const double fbin = (double)k * p->fstep;                   // PV.py:114
            const double dthetabin = pi2 * fbin * p->dt;                // PV.py:116
            wf[k] = nearbyint(dthetabin / pi2) * pi2;                   // PV.py:118 (np.round: half to even)
        }
        if (p->d_wfbin.alloc(sizeof(double) * wf.size()) != PVX_OK) { pvx_set_error("hipMalloc(wfbin) failed"); return PVX_ERR_ALLOC; }
        if (hipMemcpy(p->d_wfbin.get(), wf.data(), sizeof(double) * wf.size(), hipMemcpyHostToDevice) != hipSuccess) { pvx_set_error("hipMemcpy(wfbin) failed"); return PVX_ERR_HIP; }
        // window with 1/wfact folded in (fft(x*win)/wfact, PV.py:156-157)
        if (p->d_win.alloc(rs * nfft) != PVX_OK) { pvx_set_error("hipMalloc(win) failed"); return PVX_ERR_ALLOC; }
        hipError_t e;
        if (precision == 32) {
            std::vector<float> w(nfft);
            for (int i = 0; i < nfft; i++) w[i] = (float)(p->win[i] / p->wfact);
            e = hipMemcpy(p->d_win.get(), w.data(), rs * nfft, hipMemcpyHostToDevice);
        } else {
            std::vector<double> w(nfft);
            for (int i = 0; i < nfft; i++) w[i] = p->win[i] / p->wfact;
            e = hipMemcpy(p->d_win.get(), w.data(), rs * nfft, hipMemcpyHostToDevice);
        }
        if (e != hipSuccess) { pvx_set_error("hipMemcpy(win) failed"); return PVX_ERR_HIP; }
    }

    // float64 fused STFT kernel (k_stft.hip): its own twiddle table; the spectrum workspace is the only intermediate
    // array left, so a launch may cover far more rows than the Infinity-Cache-sized chunks of the three-kernel path
    if (pvx_stft_supported(nfft, precision) && !getenv("PVX_NO_STFT")) {
        std::vector<double> tw(2 * (size_t)nfft);
        const double pi = 3.141592653589793238462643383279502884;
        if (nfft % 8 == 0) {
            // W^j = cos - i sin from libm on the first octant only; the rest by the table's exact symmetries
            // W^(N/4 - j) = (-Im, -Re) W^j and W^(j + N/4) = -i W^j, so that a kernel may keep an eighth of the table and
            // derive the other entries (k_stft_pv.hip) and still use the very values the full-table kernels read
            const int q = nfft / 4, o = nfft / 8;
            for (int j = 0; j <= o; j++) { tw[2 * j] = cos(2.0 * pi * j / (double)nfft); tw[2 * j + 1] = -sin(2.0 * pi * j / (double)nfft); }
            tw[2 * o] = 0.70710678118654752440; tw[2 * o + 1] = -0.70710678118654752440;      // W^(N/8) is its own mirror image
            for (int j = o + 1; j <= q; j++) { tw[2 * j] = -tw[2 * (q - j) + 1]; tw[2 * j + 1] = -tw[2 * (q - j)]; }
            for (int j = q + 1; j < nfft; j++) { tw[2 * j] = tw[2 * (j - q) + 1]; tw[2 * j + 1] = -tw[2 * (j - q)]; }
        } else
        for (int j = 0; j < nfft; j++) { tw[2 * j] = cos(2.0 * pi * j / (double)nfft); tw[2 * j + 1] = -sin(2.0 * pi * j / (double)nfft); }
        std::vector<float> twf(tw.begin(), tw.end());
        const void* src = precision == 64 ? (const void*)tw.data() : (const void*)twf.data();
        if (p->d_twiddle64.alloc(tw.size() * rs) != PVX_OK) { pvx_set_error("hipMalloc(stft twiddle) failed"); return PVX_ERR_ALLOC; }
        if (hipMemcpy(p->d_twiddle64.get(), src, tw.size() * rs, hipMemcpyHostToDevice) != hipSuccess) { pvx_set_error("hipMemcpy(stft twiddle) failed"); return PVX_ERR_HIP; }
        // nfft 512 .. 2048: the peaks found in the transform's launch; at float64 with npks <= 64 the spectrum rows kept on chip
        p->general = Route::stft_peaks;
        if (pvx_stft_pv_supported(nfft, precision, npks) && !getenv("PVX_NO_STFT_PV"))
            p->general = pvx_pv_rev_supported(nfft, precision, npks) && !getenv("PVX_NO_PV_REV") ? Route::pv_rev : Route::stft_pv;
        // (k_pv_team is a witness kernel -- tests/libpvx_witness.so, asked for with PVX_PV_TEAM=1: correct, one launch, and slower than
        // the two kernels it would replace, profiles/r06_ab_steps.txt; in the product library pvx_pv_team_supported() says no)
        if (getenv("PVX_PV_TEAM") && pvx_pv_team_supported(nfft, precision, npks, hop)) p->general = Route::pv_team;
        if (!getenv("PVX_MAX_ROWS")) {
            int64_t big = (int64_t)(((size_t)1 << 30) / ((size_t)p->ldo * 2 * rs));
            if (big > 262144) big = 262144;
            const int64_t want = (rows_hint > 0 && rows_hint < big) ? rows_hint : big;
            p->max_rows = want < 2 ? 2 : want;
        }
    }

    // fused kernel tables
    const bool can1 = pvx_fused_supported(nfft, precision, npks) != 0, can2 = pvx_fused_mw_supported(nfft, precision, npks) != 0;
    const bool can3 = pvx_fused_ring_supported(nfft, precision, npks) != 0, can4 = pvx_fused_rev_supported(nfft, precision, npks) != 0;
    const bool can5 = pvx_fused_team_supported(nfft, precision, npks) != 0;
    if (can1 || can2 || can3 || can4 || can5) {
        const size_t ntt = can5 ? (size_t)pvx_fused_team_table_len(nfft) : 0;       // k_fused_team's lane-ordered twiddles follow the table
        std::vector<float> tw(2 * ((size_t)nfft + ntt));
        const double pi = 3.141592653589793238462643383279502884;
        for (int j = 0; j < nfft; j++) { tw[2 * j] = (float)cos(2.0 * pi * j / (double)nfft); tw[2 * j + 1] = (float)(-sin(2.0 * pi * j / (double)nfft)); }
        if (ntt) pvx_fused_team_table(nfft, tw.data(), tw.data() + 2 * (size_t)nfft);
        if (p->d_twiddle.alloc(tw.size() * 4) != PVX_OK || p->d_specrow.alloc((size_t)nfft * 4) != PVX_OK) { pvx_set_error("hipMalloc(fused tables) failed"); return PVX_ERR_ALLOC; }
        if (hipMemcpy(p->d_twiddle.get(), tw.data(), tw.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { pvx_set_error("hipMemcpy(twiddle) failed"); return PVX_ERR_HIP; }
        // default: one wave per frame where it exists (nfft <= 2048: independent waves walking their rows downwards
        // over one buffer each, k_fused_rev.hip, while npks leaves them enough LDS), several waves per frame above
        // (nfft 4096 / 8192: teams of such waves, k_fused_team.hip, while npks <= 128; the general path beyond -- and wherever
        // npks asks for more staging than these kernels' LDS holds.  Mode 2, k_fused_mw.hip, is a witness: only when asked for)
        p->fft_mode = can4 ? 4 : can3 ? 3 : can1 ? 1 : can5 ? 5 : 0;
        if (const char* e = getenv("PVX_FFT_MODE")) {
            const int m = atoi(e);
            if (m == 0 || (m == 1 && can1) || (m == 2 && can2) || (m == 3 && can3) || (m == 4 && can4) || (m == 5 && can5)) p->fft_mode = m;
        }
        if (const char* e = getenv("PVX_FUSED_BLOCKS")) { const long long v = atoll(e); if (v > 0) p->fused_blocks = v; }
    }
    *out = owner.release();
    return PVX_OK;
}

// spectrum workspace of the k_stft path: [max_rows+1][ldo] complex, created on first use
static int ensure_spec_ws(pvx_plan* p) {
    if (p->d_spec) return PVX_OK;
    const size_t sbytes = (size_t)(p->max_rows + 1) * p->ldo * 2 * real_size(p->precision);
    if (p->d_spec.alloc(sbytes) != PVX_OK) { pvx_set_error("hipMalloc of %.1f MiB spectrum workspace failed", sbytes / 1048576.0); return PVX_ERR_ALLOC; }
    p->ws_bytes += (int64_t)sbytes;
    return PVX_OK;
}
static bool has_stft(const pvx_plan* p) { return p->general != Route::frames_rocfft; }

// The route of one call of analyze_rows() over `total_rows` rows of samples of type x_dtype: the plan's fft mode, else its
// general route as far as the call allows.  The one-launch kernels index rows in 32 bits: a larger call of a team plan takes
// the general path (for that call only), the float64 ones take k_stft_pv / k_stft.
static Route route_for(const pvx_plan* p, int x_dtype, int64_t total_rows) {
    const bool rows32 = total_rows < 0x7fffff00LL;
    switch (p->fft_mode) {
        case 1: return Route::fused;
        case 2: return Route::fused_mw;
        case 3: return Route::fused_ring;
        case 4: return Route::fused_rev;
        case 5: if (rows32) return Route::fused_team; break;
    }
    const Route g = p->general;
    if (g == Route::pv_rev && rows32 && pvx_pv_rev_takes(p->nfft, x_dtype, p->hop)) return Route::pv_rev;
    if (g == Route::pv_team && rows32) return Route::pv_team;
    if (g == Route::pv_rev || g == Route::stft_pv) return pvx_stft_pv_takes(p->nfft, p->precision, x_dtype, p->hop) ? Route::stft_pv : Route::stft_peaks;
    if (g == Route::frames_rocfft) return g;
    // nfft 8192 (k_stft_split -> k_phase_peaks): the transform leaves every row's candidate peaks, the peak kernel does not
    // stream the 64 KB rows again (float64, config 2's signal: 0.79 -> 0.63 ms; PVX_NO_CAND=1: the two kernels as before).  At
    // nfft 4096 (teams of two waves at 256 registers: the scan's reads cannot all be in flight) the scan costs the transform
    // kernel what it saves the peak kernel: off unless PVX_CAND_4096=1.
    const bool cand = getenv("PVX_NO_CAND") == nullptr && (p->nfft == 8192 || (p->nfft == 4096 && getenv("PVX_CAND_4096") != nullptr));
    return cand ? Route::stft_cand_peaks : Route::stft_peaks;
}

static int ensure_cand_ws(pvx_plan* p) {
    if (p->d_cand_bin) return PVX_OK;
    const int cap = p->N2 / 2 + 8;
    const size_t rows = (size_t)p->max_rows + 1, rs = real_size(p->precision);
    if (p->d_cand_y.alloc(rows * cap * rs) != PVX_OK || p->d_cand_bin.alloc(rows * cap * 2) != PVX_OK ||
        p->d_cand_stats.alloc(rows * 4 * sizeof(double)) != PVX_OK) {
        p->d_cand_y.reset(); p->d_cand_bin.reset(); p->d_cand_stats.reset();
        pvx_set_error("hipMalloc of the candidate workspace failed");
        return PVX_ERR_ALLOC;
    }
    p->cand_cap = cap;
    p->ws_bytes += (int64_t)(rows * cap * (rs + 2) + rows * 32);
    return PVX_OK;
}

// frames + spectrum workspace and the rocFFT plan (fft mode 0, calc_fft_frame): created on first use.
// With k_stft in charge of the analysis the rocFFT side only serves pvx_stft_frames: two rows, its own output.
static void release_rocfft(pvx_plan* p) {
    p->fft.reset();
    p->d_frames.reset();
    p->d_rspec.reset();
    if (!p->rocfft_small && !has_stft(p)) p->d_spec.reset();
    p->rocfft_ready = false; p->rocfft_small = false;
}

// full = the analysis itself goes through rocFFT (fft mode 0 without k_stft, PVHarmonic at float32): workspace of
// max_rows + 1 rows; otherwise only pvx_stft_frames uses it, one frame at a time: 3 rows, output of its own
static int ensure_rocfft(pvx_plan* p, bool full) {
    if (p->rocfft_ready && (!full || !p->rocfft_small)) return PVX_OK;
    if (p->rocfft_ready) release_rocfft(p);
    const int nfft = p->nfft, precision = p->precision;
    const size_t rs = real_size(precision);
    const bool small = !full || has_stft(p);
    const int64_t max_rows = small ? 2 : p->max_rows;
    const int64_t ws_rows = max_rows + 1;
    p->rocfft_rows = max_rows;
    const size_t fbytes = (size_t)ws_rows * p->ldi * rs, sbytes = (size_t)ws_rows * p->ldo * 2 * rs;
    DevMem& spec = small ? p->d_rspec : p->d_spec;
    p->rocfft_small = small;
    if (p->d_frames.alloc(fbytes) != PVX_OK || spec.alloc(sbytes) != PVX_OK) {
        pvx_set_error("hipMalloc of %.1f MiB analysis workspace failed", (fbytes + sbytes) / 1048576.0);
        p->d_frames.reset();
        return PVX_ERR_ALLOC;
    }
    // rocFFT: batched 1-D real -> hermitian, one transform per workspace row (PV.py:157)
    rocfft_status st;
    switch (p->fft.create((size_t)nfft, (size_t)ws_rows, precision == 32 ? rocfft_precision_single : rocfft_precision_double,
                          rocfft_placement_notinplace, (size_t)p->ldi, (size_t)p->ldo, &st)) {
        case RealFft::done: break;
        case RealFft::info: pvx_set_error("rocfft work buffer query failed: %d", (int)st); return PVX_ERR_HIP;
        default: pvx_set_error("rocfft_plan_create(nfft=%d, batch=%lld) failed: %d", nfft, (long long)ws_rows, (int)st); return PVX_ERR_HIP;
    }
    if (const size_t wb = p->fft.work_bytes()) {
        if (p->fft.work.alloc(wb) != PVX_OK) { pvx_set_error("hipMalloc(rocfft work, %zu) failed", wb); return PVX_ERR_ALLOC; }
        st = p->fft.set_work(p->fft.work.get(), wb);
        if (st != rocfft_status_success) { pvx_set_error("rocfft set_work_buffer failed: %d", (int)st); return PVX_ERR_HIP; }
    }
    p->ws_bytes += (int64_t)(fbytes + sbytes + p->fft.work_bytes());
    p->rocfft_ready = true;
    return PVX_OK;
}

extern "C" int pvx_plan_set_progress(pvx_plan* plan, pvx_progress_fn fn, void* user) {
    if (!plan) { pvx_set_error("null plan"); return PVX_ERR_INVALID; }
    plan->progress_fn = fn;
    plan->progress_user = user;
    return PVX_OK;
}

// after a launch chunk: rows [0, rows_done) of total_rows are in flight; report once they are done
static int plan_progress(pvx_plan* p, hipStream_t s, int64_t rows_done, int64_t total_rows, int64_t nsig) {
    if (!p->progress_live || !p->progress_fn) return PVX_OK;
    PVX_HIP_CHECK(hipStreamSynchronize(s));
    // rows include one zero row per signal; report frames
    const int64_t per = total_rows / nsig;                            // F + 1
    const int64_t full = rows_done / per, rem = rows_done - full * per;
    const int64_t frames = full * (per - 1) + (rem > 0 ? rem - 1 : 0);
    if (frames < nsig * (per - 1)) p->progress_fn(frames, nsig * (per - 1), p->progress_user);   // the last report comes from the entry point
    return PVX_OK;
}

extern "C" int pvx_plan_set_timing(pvx_plan* plan, int enable) {
    if (!plan) { pvx_set_error("null plan"); return PVX_ERR_INVALID; }
    plan->timing = enable != 0;
    plan->ev_used = 0;
    plan->ev_spans.clear();
    return PVX_OK;
}

// stage >= 0: the event starts a span of that stage (which ends at the next recorded event);
// stage < 0: the event only ends the previous span
static int plan_event(pvx_plan* p, hipStream_t s, int stage) {
    if (!p->timing) return PVX_OK;
    if (p->ev_used == p->ev_pool.size()) {
        Event e;
        PVX_HIP_CHECK(e.ensure(hipEventDefault));
        p->ev_pool.push_back(std::move(e));
    }
    if (stage >= 0) p->ev_spans.push_back(std::make_pair(stage, p->ev_used));
    PVX_HIP_CHECK(hipEventRecord(p->ev_pool[p->ev_used++], s));
    return PVX_OK;
}

extern "C" int pvx_plan_get_timing(pvx_plan* plan, double* ms, int64_t* launches) {
    if (!plan || !ms || !launches) { pvx_set_error("null argument"); return PVX_ERR_INVALID; }
    for (int i = 0; i < 4; i++) { ms[i] = 0.0; launches[i] = 0; }
    if (plan->ev_used) PVX_HIP_CHECK(hipEventSynchronize(plan->ev_pool[plan->ev_used - 1]));
    for (const auto& sp : plan->ev_spans) {
        if (sp.second + 1 >= plan->ev_used || sp.first > 3) continue;
        float t = 0.f;
        PVX_HIP_CHECK(hipEventElapsedTime(&t, plan->ev_pool[sp.second], plan->ev_pool[sp.second + 1]));
        ms[sp.first] += (double)t;
        launches[sp.first] += 1;
    }
    plan->ev_used = 0;
    plan->ev_spans.clear();
    return PVX_OK;
}

// ---- run_pv ---------------------------------------------------------------------------------
// the spectrum row a call asks for (chunk carry, last_spec; -1: none), and a page-locked block the fused kernels write it to
// instead of d_specrow
struct SpecRequest { int64_t row = -1; float* host = nullptr; };

// where `route` left the spectrum row its call asked for (the call's last row `row`): [N2] complex, float32 or float64
struct SpecRow { const void* d; bool f32; };
static SpecRow spec_row_at(const pvx_plan* p, Route route, int64_t row) {
    if (is_fused(route)) return {p->d_specrow.as<float>(), true};
    if (route == Route::pv_rev || route == Route::pv_team) return {p->d_lastspec.as<double>(), false};
    const int64_t wsrow = row % p->max_rows + 1;             // in the last chunk's workspace
    return {p->d_spec.as<const char>() + (size_t)wsrow * p->ldo * 2 * real_size(p->precision), p->precision == 32};
}

// window + FFT of a chunk's workspace rows into d_spec: k_stft, or k_frames + rocFFT (stage events 0 and 1)
static int launch_transform(pvx_plan* p, const FrameParams& fp, int x_dtype, hipStream_t s) {
    int rc;
    if ((rc = plan_event(p, s, 0)) != PVX_OK) return rc;
    if (has_stft(p)) return pvx_launch_stft(fp, p->d_spec.get(), p->ldo, p->d_twiddle64.get(), x_dtype, p->precision, s);
    if ((rc = pvx_launch_frames(fp, x_dtype, p->precision, s)) != PVX_OK || (rc = plan_event(p, s, 1)) != PVX_OK) return rc;
    PVX_FFT_CHECK(p->fft.execute(p->d_frames.get(), p->d_spec.get(), s));
    return PVX_OK;
}

// The analysis of a call by `route` (route_for), which the plan records.  wire_out: d_f / d_mag / d_ph / d_binno / d_totalmag
// are the sections of a wire block (pvx_analyze_dev_wire): only k_fused_rev writes it itself.
static int analyze_rows(pvx_plan* p, Route route, const void* d_x, int x_dtype, int64_t nsamp, int64_t nsig, int64_t sig_stride,
                        int64_t F, double* d_f, double* d_mag, double* d_ph, double* d_realph, double* d_binno,
                        double* d_t, double* d_totalmag, const double* d_prev0, hipStream_t s,
                        SpecRequest spec = {}, bool wire_out = false) {
    const int64_t total_rows = nsig * (F + 1);
    int rc;
    if (wire_out && route != Route::fused_rev) return PVX_ERR_UNSUPPORTED;
    p->last_route = route;
    if (is_fused(route)) {
        // one launch: window + FFT + peaks, no intermediate arrays (k_fused_rev.hip / k_fused_team.hip; the witnesses' modes 1 - 3)
        if (x_dtype == PVX_F64) {
            // float64 samples already in HBM (the host entry points narrow while they stage): the fused kernels' first step
            // is (float) x[n] -- done here in one pass, so that they exist for float32 and int16 samples only (a float64
            // sample pair per lane and row cost them registers they do not have)
            const size_t nel = (size_t)((nsig - 1) * sig_stride + nsamp);
            if ((rc = p->d_x32.grow(nel * 4, Sizing::headroom)) != PVX_OK) return rc;
            if ((rc = pvx_launch_narrow((const double*)d_x, p->d_x32.as<float>(), (int64_t)nel, s)) != PVX_OK) return rc;
            d_x = p->d_x32.as<float>(); x_dtype = PVX_F32;
        }
        FusedParams fp;
        fp.x = d_x; fp.sig_stride = sig_stride; fp.F = F; fp.total_rows = total_rows;
        fp.hop = p->hop; fp.K = p->npks; fp.rad = 5;                                     // PV.py:177
        fp.thr = p->pkthresh; fp.sr = p->sr; fp.fstep = p->fstep; fp.dt = p->dt;
        fp.wfbin = p->d_wfbin.as<double>(); fp.prev0 = d_prev0;
        fp.f = d_f; fp.mag = d_mag; fp.ph = d_ph; fp.realph = d_realph; fp.binno = d_binno;
        fp.t = d_t; fp.totalmag = d_totalmag; fp.win = p->d_win.get(); fp.twiddle = p->d_twiddle.get();
        fp.spec_out = spec.row >= 0 ? (spec.host ? spec.host : p->d_specrow.as<float>()) : nullptr; fp.spec_row = spec.row;
        fp.blocks_override = p->fused_blocks;
        fp.stash = nullptr; fp.stash_bytes = 0;
        fp.wire = wire_out ? p->wire_fmt : 0;
        if (route == Route::fused_rev) {
            // k_fused_rev: the block where its waves hand a spectrum to the wave below them (sized once, for a full grid)
            if (!p->d_stash) {
                FusedParams q = fp;
                q.total_rows = (int64_t)1 << 30;
                const size_t need = pvx_fused_rev_stash_bytes(q, p->nfft);
                if (need > 0 && p->d_stash.alloc(need) != PVX_OK) (void)hipGetLastError();   // not an error: without it the waves compute that row themselves
            }
            fp.stash = p->d_stash.get(); fp.stash_bytes = p->d_stash.cap();
        }
        if ((rc = plan_event(p, s, 3)) != PVX_OK) return rc;
        switch (route) {
            case Route::fused: rc = pvx_launch_fused(fp, p->nfft, x_dtype, s); break;
            case Route::fused_mw: rc = pvx_launch_fused_mw(fp, p->nfft, x_dtype, s); break;
            case Route::fused_ring: rc = pvx_launch_fused_ring(fp, p->nfft, x_dtype, s); break;
            case Route::fused_team: rc = pvx_launch_fused_team(fp, p->nfft, x_dtype, s); break;
            default: rc = pvx_launch_fused_rev(fp, p->nfft, x_dtype, s, &p->last_rev_kc); break;
        }
        return rc != PVX_OK ? rc : plan_event(p, s, -1);
    }
    if (route == Route::pv_rev || route == Route::pv_team) {
        // float64, npks <= 64: ONE launch over all rows, no spectrum workspace -- nfft 512 .. 2048: a wave per frame (k_pv_rev.hip);
        // nfft 4096 / 8192 at the sliding-window hops: a team of waves per frame (k_pv_team.hip)
        const bool team = route == Route::pv_team;
        PvRevParams rp;
        rp.x = d_x; rp.sig_stride = sig_stride; rp.F = F; rp.total_rows = total_rows;
        rp.hop = p->hop; rp.K = p->npks; rp.rad = 5;                                     // PV.py:177
        rp.thr = p->pkthresh; rp.sr = p->sr; rp.fstep = p->fstep; rp.dt = p->dt;
        rp.wfbin = p->d_wfbin.as<double>(); rp.prev0 = d_prev0;
        rp.f = d_f; rp.mag = d_mag; rp.ph = d_ph; rp.realph = d_realph; rp.binno = d_binno;
        rp.t = d_t; rp.totalmag = d_totalmag; rp.win = p->d_win.get(); rp.twiddle = p->d_twiddle64.get();
        rp.spec_out = nullptr; rp.spec_row = spec.row;
        if (spec.row >= 0) {
            if (!p->d_lastspec && (rc = p->d_lastspec.alloc(sizeof(double) * 2 * (size_t)(p->N2 > 0 ? p->N2 : 1))) != PVX_OK) return rc;
            rp.spec_out = p->d_lastspec.as<double>();
        }
        rp.blocks_override = 0;
        if (const char* e = getenv("PVX_PV_REV_BLOCKS")) { const long long v = atoll(e); if (v >= 1) rp.blocks_override = v; }   // tests: other grids
        rp.win_symmetric = p->win_symmetric ? 1 : 0;
        rp.stage = nullptr; rp.stage_bytes = 0;
        const size_t need = team ? pvx_pv_team_stage_bytes(p->nfft) : pvx_pv_rev_stage_bytes(p->nfft);
        if (need > 0) {
            if ((rc = p->d_pvstage.grow(need, Sizing::headroom)) != PVX_OK) return rc;
            rp.stage = p->d_pvstage.get(); rp.stage_bytes = p->d_pvstage.cap();
        }
        // one launch -- unless the caller set PVX_MAX_ROWS: then pieces of that many rows, each reported (tests, progress displays)
        const int64_t piece = p->rows_from_env ? p->max_rows : total_rows;
        for (int64_t R0 = 0; R0 < total_rows; R0 += piece) {
            rp.row_begin = R0; rp.row_end = (total_rows - R0 < piece) ? total_rows : R0 + piece;
            if ((rc = plan_event(p, s, 3)) != PVX_OK) return rc;
            if ((rc = team ? pvx_launch_pv_team(rp, p->nfft, x_dtype, s) : pvx_launch_pv_rev(rp, p->nfft, x_dtype, s)) != PVX_OK) return rc;
            if ((rc = plan_event(p, s, -1)) != PVX_OK) return rc;
            if ((rc = plan_progress(p, s, rp.row_end, total_rows, nsig)) != PVX_OK) return rc;
        }
        return PVX_OK;
    }
    // chunks of max_rows rows through the spectrum workspace
    if ((rc = has_stft(p) ? ensure_spec_ws(p) : ensure_rocfft(p, true)) != PVX_OK) return rc;
    const bool cand = route == Route::stft_cand_peaks;
    if (cand && (rc = ensure_cand_ws(p)) != PVX_OK) return rc;
    for (int64_t R0 = 0; R0 < total_rows; R0 += p->max_rows) {
        const int64_t nrows = (total_rows - R0 < p->max_rows) ? (total_rows - R0) : p->max_rows;
        FrameParams fp;
        fp.x = d_x; fp.nsamp = nsamp; fp.sig_stride = sig_stride; fp.F = F; fp.R0 = R0;
        fp.ws_rows = nrows + 1; fp.total_rows = total_rows; fp.nfft = p->nfft; fp.hop = p->hop;
        fp.win = p->d_win.get(); fp.frames = p->d_frames.get(); fp.ldi = p->ldi; fp.win_symmetric = p->win_symmetric ? 1 : 0;
        PeaksParams pp;
        pp.spec = p->d_spec.get(); pp.ldo = p->ldo; pp.F = F; pp.R0 = R0; pp.nrows = nrows;
        pp.nfft = p->nfft; pp.hop = p->hop; pp.N2 = p->N2; pp.K = p->npks; pp.rad = 5;   // PV.py:177
        pp.thr = p->pkthresh; pp.sr = p->sr; pp.fstep = p->fstep; pp.dt = p->dt;
        pp.wfbin = p->d_wfbin.as<double>(); pp.prev0 = d_prev0;
        pp.f = d_f; pp.mag = d_mag; pp.ph = d_ph; pp.realph = d_realph; pp.binno = d_binno;
        pp.t = d_t; pp.totalmag = d_totalmag; pp.frames_per_wave = p->frames_per_wave;
        if (cand) {
            fp.cand_y = p->d_cand_y.get(); fp.cand_bin = p->d_cand_bin.as<unsigned short>(); fp.cand_stats = p->d_cand_stats.as<double>(); fp.cand_cap = p->cand_cap; fp.cand_thr = p->pkthresh;
            pp.cand_y = p->d_cand_y.get(); pp.cand_bin = p->d_cand_bin.as<unsigned short>(); pp.cand_stats = p->d_cand_stats.as<double>(); pp.cand_cap = p->cand_cap;
        }
        if (route == Route::stft_pv) {
            // window + FFT + untangle + peaks of every row in one kernel (k_stft_pv.hip); the spectrum rows still land in
            // the workspace
            if ((rc = plan_event(p, s, 3)) != PVX_OK) return rc;
            if ((rc = pvx_launch_stft_pv(fp, pp, p->d_spec.get(), p->ldo, p->d_twiddle64.get(), x_dtype, p->precision, s)) != PVX_OK) return rc;
        } else {
            if ((rc = launch_transform(p, fp, x_dtype, s)) != PVX_OK) return rc;
            if ((rc = plan_event(p, s, 2)) != PVX_OK) return rc;
            if ((rc = pvx_launch_phase_peaks(pp, p->precision, s)) != PVX_OK) return rc;
        }
        if ((rc = plan_event(p, s, -1)) != PVX_OK) return rc;
        if ((rc = plan_progress(p, s, R0 + nrows, total_rows, nsig)) != PVX_OK) return rc;
    }
    return PVX_OK;
}

static int check_analyze_args(pvx_plan* p, const void* x, int x_dtype, int64_t nsamp, int64_t nsig, int64_t sig_stride,
                              const void* prev0) {
    if (!p) { pvx_set_error("null plan"); return PVX_ERR_INVALID; }
    if (!x && nsamp > 0) { pvx_set_error("null signal"); return PVX_ERR_INVALID; }
    if (x_dtype != PVX_F32 && x_dtype != PVX_F64 && x_dtype != PVX_I16) { pvx_set_error("bad x_dtype %d", x_dtype); return PVX_ERR_INVALID; }
    if (nsamp < 0 || nsig < 1) { pvx_set_error("bad nsamp/nsig"); return PVX_ERR_INVALID; }
    if (nsig > 1 && sig_stride < nsamp) { pvx_set_error("sig_stride %lld < nsamp %lld", (long long)sig_stride, (long long)nsamp); return PVX_ERR_INVALID; }
    if (prev0 && nsig != 1) { pvx_set_error("prev0 is only valid with nsig == 1"); return PVX_ERR_INVALID; }
    return PVX_OK;
}

extern "C" int64_t pvx_analyze_dev(pvx_plan* p, const void* d_x, int x_dtype, int64_t nsamp, int64_t nsig,
                                   int64_t sig_stride, double* d_f, double* d_mag, double* d_ph, double* d_realph,
                                   double* d_binno, double* d_t, double* d_totalmag, const double* d_prev0,
                                   void* stream) {
    int rc = pvx_require_plan_device(p);
    if (rc != PVX_OK) return rc;
    rc = check_analyze_args(p, d_x, x_dtype, nsamp, nsig, sig_stride, d_prev0);
    if (rc != PVX_OK) return rc;
    const int64_t F = pvx_nframes(nsamp, p->nfft, p->hop);
    if (F == 0) return 0;
    if (!d_f || !d_mag || !d_ph || !d_realph || !d_binno) { pvx_set_error("null output array"); return PVX_ERR_INVALID; }
    rc = analyze_rows(p, route_for(p, x_dtype, nsig * (F + 1)), d_x, x_dtype, nsamp, nsig, sig_stride, F, d_f, d_mag, d_ph,
                      d_realph, d_binno, d_t, d_totalmag, d_prev0, (hipStream_t)stream);
    return rc == PVX_OK ? F : rc;
}

static size_t dtype_size(int x_dtype) { return x_dtype == PVX_F32 ? 4 : (x_dtype == PVX_F64 ? 8 : 2); }

static int host_stream(pvx_plan* p) {
    PVX_HIP_CHECK(p->s_host.ensure(hipStreamNonBlocking));
    for (int i = 0; i < 2; i++) PVX_HIP_CHECK(p->ev_done[i].ensure(hipEventDisableTiming));
    return PVX_OK;
}

// Large host <-> device transfers of PAGEABLE caller memory.  A plain hipMemcpy stages through the runtime's own pinned
// buffers on one thread (~20 GB/s host-side; measured on BASELINE config 2's 106 MB signal: 4.9 ms -> 2.7 ms with four threads on 2 MB pieces, 2.3 ms on 4 MB pieces; eight threads on 1 MB pieces: 3.4 ms; `tools/ab/stage_ab.sh`); here kStageThreads threads copy 4 MB pieces between the caller's array and a
// pinned ring (two slots per thread) while the DMA engine moves the other slots: the host copies run in parallel with each
// other and with the DMA, the link (PCIe Gen5 x16, ~55 GB/s) becomes the limit.  The DMAs are queued on `s`: work issued on
// `s` afterwards is ordered behind them; the calls return when every host-side copy is done (H2D) / every byte has
// arrived in the caller's array (D2H).
static const int kStageMaxThreads = 8;
static const int kStageThreads = [] { const char* e = getenv("PVX_STAGE_THREADS"); const int v = e ? atoi(e) : 0; return (v >= 1 && v <= kStageMaxThreads) ? v : 4; }();
static const size_t kStagePiece = [] { const char* e = getenv("PVX_STAGE_PIECE_MB"); const int v = e ? atoi(e) : 0; return (size_t)((v >= 1 && v <= 16) ? v : 4) << 20; }();
static const size_t kStageMin = (size_t)16 << 20;           // below this a plain copy is as good

struct StageRing { PinMem& h_ring; Event* ev_ring; };         // a plan's ring, or the process-wide one of the plan-less entry points
static int stage_ring(StageRing r) {
    if (!r.h_ring && r.h_ring.alloc(kStagePiece * 2 * kStageThreads) != PVX_OK) { pvx_set_error("hipHostMalloc(staging ring) failed"); return PVX_ERR_ALLOC; }
    for (int i = 0; i < 16; i++) PVX_HIP_CHECK(r.ev_ring[i].ensure(hipEventDisableTiming));
    return PVX_OK;
}
static int stage_ring(pvx_plan* p) { return stage_ring(StageRing{p->h_ring, p->ev_ring}); }

// narrow: `host` holds float64 samples and the device gets them as float32 (`bytes` counts the float32 bytes): every
// precision-32 kernel's first step is (float) x[n], so the staging threads do it while they copy -- the same rounding, half
// the bytes over the link.
static int staged_copy(StageRing ring, void* dev, void* host, size_t bytes, bool to_device, hipStream_t s, bool narrow = false) {
    int rc = stage_ring(ring);
    if (rc != PVX_OK) return rc;
    char* const h_ring = ring.h_ring.as<char>();
    Event* const ev_ring = ring.ev_ring;
    int devid = 0;
    (void)hipGetDevice(&devid);
    const size_t npieces = (bytes + kStagePiece - 1) / kStagePiece;
    int err[kStageMaxThreads] = {0};
    auto worker = [&](int t, int nthreads) {
        if (hipSetDevice(devid) != hipSuccess) { err[t] = 1; return; }
        size_t k = 0;
        for (size_t i = (size_t)t; i < npieces; i += nthreads, k++) {
            const int slot = 2 * t + (int)(k & 1);
            char* pin = h_ring + (size_t)slot * kStagePiece;
            const size_t o = i * kStagePiece, c = bytes - o < kStagePiece ? bytes - o : kStagePiece;
            if (to_device) {
                // the slot's previous DMA has read it -- of this call or of an earlier one on the same ring (nothing orders
                // the host against those but this event; on an event never recorded the wait returns at once)
                if (hipEventSynchronize(ev_ring[slot]) != hipSuccess) { err[t] = 1; return; }
                if (narrow) narrow_f64_f32((const double*)host + o / 4, (float*)pin, c / 4);
                else memcpy(pin, (const char*)host + o, c);
                if (hipMemcpyAsync((char*)dev + o, pin, c, hipMemcpyHostToDevice, s) != hipSuccess || hipEventRecord(ev_ring[slot], s) != hipSuccess) { err[t] = 1; return; }
            } else {
                // two DMAs of this thread in flight: piece k+1 lands while piece k is copied out
                if (k == 0) {
                    if (hipMemcpyAsync(pin, (const char*)dev + o, c, hipMemcpyDeviceToHost, s) != hipSuccess || hipEventRecord(ev_ring[slot], s) != hipSuccess) { err[t] = 1; return; }
                }
                const size_t in = i + nthreads;
                if (in < npieces) {
                    const int ns = 2 * t + (int)((k + 1) & 1);
                    const size_t no = in * kStagePiece, nc = bytes - no < kStagePiece ? bytes - no : kStagePiece;
                    if (hipMemcpyAsync(h_ring + (size_t)ns * kStagePiece, (const char*)dev + no, nc, hipMemcpyDeviceToHost, s) != hipSuccess ||
                        hipEventRecord(ev_ring[ns], s) != hipSuccess) { err[t] = 1; return; }
                }
                if (hipEventSynchronize(ev_ring[slot]) != hipSuccess) { err[t] = 1; return; }
                memcpy((char*)host + o, pin, c);
            }
        }
    };
    // (a thread that cannot be created must not take the process down through the C ABI: the copy then runs on this thread)
    const bool one_thread = getenv("PVX_NO_STAGE_THREADS") != nullptr;
    int nthreads = one_thread ? 1 : kStageThreads;
    std::thread th[kStageMaxThreads];
    int started = 1;
    try {
        for (int t = 1; t < nthreads; t++) { th[t] = std::thread(worker, t, nthreads); started = t + 1; }
    } catch (...) {
        for (int t = 1; t < started; t++) th[t].join();
        if (started > 1) { (void)hipStreamSynchronize(s); pvx_set_error("staged host transfer: could not start its threads"); return PVX_ERR_HIP; }
        nthreads = 1;
    }
    worker(0, nthreads);
    for (int t = 1; t < (started > 1 ? nthreads : 1); t++) th[t].join();
    for (int t = 0; t < nthreads; t++)
        if (err[t]) { (void)hipStreamSynchronize(s); pvx_set_error("staged host transfer failed (%s)", hipGetErrorString(hipGetLastError())); return PVX_ERR_HIP; }
    return PVX_OK;
}

static int staged_copy(pvx_plan* p, void* dev, void* host, size_t bytes, bool to_device, hipStream_t s, bool narrow = false) {
    return staged_copy(StageRing{p->h_ring, p->ev_ring}, dev, host, bytes, to_device, s, narrow);
}
// Transfers between the CALLER's arrays and device memory.  A hipMemcpy of a pageable array of 1 MB or more makes the
// runtime register (pin in place) that memory; when the caller frees the array -- result arrays: every call -- the next
// transfer of the process waits tens of milliseconds for the unmapping (measured: PVHarmonic.run_pv 8 -> 32 ms per
// call).  So nothing of the caller's above kDirectMax is ever handed to hipMemcpy: page-locked arrays go straight, large
// pageable ones through the threaded ring, the ones in between bounce through the process-wide ring's memory.
static const size_t kDirectMax = (size_t)512 << 10;
static const int kMaxDevices = 16;
struct DevRing { PinMem ring; Event ev[16]; std::mutex mu; };   // one per device: its events belong to that device
static DevRing* const g_rings = new DevRing[kMaxDevices];        // (for the process: never deleted, pvx_mem.h)
static bool host_is_pinned(const void* host) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, host) != hipSuccess) { (void)hipGetLastError(); return false; }
    return attr.type == hipMemoryTypeHost;
}
static int user_copy(void* dev, void* host, size_t bytes, bool to_device) {
    if (bytes == 0) return PVX_OK;
    const hipMemcpyKind kind = to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    if (bytes <= kDirectMax || host_is_pinned(host)) {
        PVX_HIP_CHECK(to_device ? hipMemcpy(dev, host, bytes, kind) : hipMemcpy(host, dev, bytes, kind));
        return PVX_OK;
    }
    int devid = 0;
    (void)hipGetDevice(&devid);
    DevRing& dr = g_rings[devid >= 0 && devid < kMaxDevices ? devid : 0];
    std::lock_guard<std::mutex> lk(dr.mu);
    const StageRing ring{dr.ring, dr.ev};
    if (bytes >= kStageMin && getenv("PVX_NO_STAGE_THREADS") == nullptr) {
        const int rc = staged_copy(ring, dev, host, bytes, to_device, nullptr);
        if (rc != PVX_OK) return rc;
        PVX_HIP_CHECK(hipStreamSynchronize(nullptr));
        return PVX_OK;
    }
    int rc = stage_ring(ring);
    if (rc != PVX_OK) return rc;
    const size_t cap = kStagePiece * 2 * kStageThreads;
    void* const g_ring = dr.ring.get();
    for (size_t o = 0; o < bytes; o += cap) {
        const size_t c = bytes - o < cap ? bytes - o : cap;
        if (to_device) {
            memcpy(g_ring, (const char*)host + o, c);
            PVX_HIP_CHECK(hipMemcpy((char*)dev + o, g_ring, c, kind));
        } else {
            PVX_HIP_CHECK(hipMemcpy(g_ring, (const char*)dev + o, c, kind));
            memcpy((char*)host + o, g_ring, c);
        }
    }
    return PVX_OK;
}
static int host_to_device(void* dev, const void* host, size_t bytes) { return user_copy(dev, (void*)host, bytes, true); }
static int device_to_host(void* host, const void* dev, size_t bytes) { return user_copy((void*)dev, host, bytes, false); }

struct HostOut { double *f, *mag, *ph, *realph, *binno, *t, *totalmag; };

// pointers into a packed result block of `rows` frames: f | mag | ph | realph | binno | t | totalmag
static HostOut block_ptrs(double* base, int64_t rows, int K) {
    const size_t n = (size_t)rows * K;
    HostOut o;
    o.f = base; o.mag = base + n; o.ph = base + 2 * n; o.realph = base + 3 * n; o.binno = base + 4 * n;
    o.t = base + 5 * n; o.totalmag = base + 5 * n + rows;
    return o;
}

static const size_t kSmallCall = (size_t)4 << 20;     // calls up to this size go through pinned staging, one sync
// ... and analyses up to the size where the threaded ring takes over (kStageMin): the plan's own pinned block, the DMA of
// piece i under the host copy of piece i+1, one result copy, one synchronisation -- and no lock shared with other plans
// (pvx_batch_run's workers; the process-wide bounce ring in between cost a 30-s signal 0.45 ms alone and serialised them)
static const size_t kSmallAnalyze = kStageMin;

// spectrum of the last row of the call that just ran on `s` by `route` -> p->d_prev (float64 [N2][2])
static int carry_spectrum(pvx_plan* p, Route route, int64_t rows_in_call, hipStream_t s) {
    const SpecRow r = spec_row_at(p, route, rows_in_call - 1);
    return pvx_launch_spec_to_prev(p->d_prev.as<double>(), r.d, 2 * p->N2, r.f32, s);
}

// The host entry point of run_pv (PV.py:213-264).
//   keep = false: results stream back into the caller's arrays (`ho`);
//   keep = true : results stay in the plan's resident block (pvx_analyze_resident), nothing comes back.
// The input is taken in chunks of frames (one signal) or of whole signals (a batch) that fit
// PVX_MAX_DEVICE_BYTES, double-buffered: while the kernels of chunk i run on the plan's stream the host
// copies chunk i+1 in and chunk i-1's results out.  Between chunks of one signal the spectrum of the last
// frame is carried on the device as the next chunk's `oldfft` (PV.py:209), so the result is the same,
// bit for bit, as one launch over the whole signal -- and a signal larger than HBM runs.
static int64_t analyze_host(pvx_plan* p, const void* x, int x_dtype, int64_t nsamp, int64_t nsig, int64_t sig_stride,
                            const HostOut* ho, const double* prev0, double* last_spec, bool keep) {
    HostTrace tr("analyze");
    int rc = pvx_require_plan_device(p);
    if (rc != PVX_OK) return rc;
    rc = check_analyze_args(p, x, x_dtype, nsamp, nsig, sig_stride, prev0);
    if (rc != PVX_OK) return rc;
    const int64_t F = pvx_nframes(nsamp, p->nfft, p->hop);
    if (keep) { p->res_valid = false; p->res_P = -1; }         // only a resident run replaces the resident block
    if (F == 0) return 0;
    if (!keep && (!ho->f || !ho->mag || !ho->ph || !ho->realph || !ho->binno)) { pvx_set_error("null output array"); return PVX_ERR_INVALID; }
    if (nsig == 1) sig_stride = nsamp;
    if ((rc = host_stream(p)) != PVX_OK) return rc;
    hipStream_t s = p->s_host;
    const int K = p->npks;
    const size_t es = dtype_size(x_dtype);
    const size_t per_frame_out = (size_t)(5 * K + 2) * sizeof(double);
    size_t limit = (size_t)2 << 30;                                   // per buffer (input chunk + its result block)
    if (const char* e = getenv("PVX_MAX_DEVICE_BYTES")) { const long long v = atoll(e); if (v > 0) limit = (size_t)v; }
    if (keep) {
        if ((rc = p->d_res.grow((size_t)nsig * F * per_frame_out, Sizing::headroom)) != PVX_OK) return rc;
    }
    if (!p->d_prev && (rc = p->d_prev.alloc(sizeof(double) * 2 * (size_t)(p->N2 > 0 ? p->N2 : 1))) != PVX_OK) return rc;
    if (prev0) PVX_HIP_CHECK(hipMemcpyAsync(p->d_prev.as<double>(), prev0, sizeof(double) * 2 * p->N2, hipMemcpyHostToDevice, s));

    // ---- chunking: units are frames of the one signal, or whole signals of a batch
    const bool by_frames = nsig == 1;
    const int64_t units = by_frames ? F : nsig;
    int64_t per_chunk;
    if (by_frames) {
        const size_t fixed = (size_t)p->nfft * es;
        const size_t per = (size_t)p->hop * es + (keep ? 0 : per_frame_out);
        per_chunk = limit > fixed + per ? (int64_t)((limit - fixed) / per) : 1;
    } else {
        const size_t per = (size_t)sig_stride * es + (keep ? 0 : (size_t)F * per_frame_out);
        per_chunk = (int64_t)(limit / per);
        if (per_chunk < 1) {
            // one signal of the batch does not fit: run the signals one by one through the frame chunking
            if (last_spec || prev0) { pvx_set_error("prev0 / last_spec need nsig == 1"); return PVX_ERR_INVALID; }
            for (int64_t b = 0; b < nsig; b++) {
                HostOut hb;
                const size_t o1 = (size_t)b * F, ok = o1 * K;
                if (!keep) { hb.f = ho->f + ok; hb.mag = ho->mag + ok; hb.ph = ho->ph + ok; hb.realph = ho->realph + ok; hb.binno = ho->binno + ok;
                             hb.t = ho->t ? ho->t + o1 : nullptr; hb.totalmag = ho->totalmag ? ho->totalmag + o1 : nullptr; }
                if (keep) { pvx_set_error("a signal of this batch exceeds PVX_MAX_DEVICE_BYTES: resident results need nsig == 1 for it"); return PVX_ERR_UNSUPPORTED; }
                const int64_t r = analyze_host(p, (const char*)x + (size_t)b * sig_stride * es, x_dtype, nsamp, 1, nsamp, &hb, nullptr, nullptr, false);
                if (r < 0) return r;
            }
            return F;
        }
    }
    if (per_chunk < 1) per_chunk = 1;
    if (per_chunk > units) per_chunk = units;
    const int64_t nchunks = (units + per_chunk - 1) / per_chunk;
    const size_t total_in = (size_t)((nsig - 1) * sig_stride + nsamp) * es;
    const size_t total_out = (size_t)nsig * F * per_frame_out;
    const bool small = nchunks == 1 && total_in + (keep ? 0 : total_out) <= kSmallAnalyze;
    // a small call's pinned block: the staged input | the result block at out_off | the last spectrum at spec_off
    const size_t spec_pin = (size_t)(p->N2 > 0 ? p->N2 : 1) * 16 + 256;
    const size_t out_off = (total_in + 255) & ~(size_t)255, spec_off = (out_off + (keep ? 0 : total_out) + 255) & ~(size_t)255;
    // a float64 signal analysed at precision 32: every kernel's first step is (float)x[n], so the host side narrows while it
    // stages (same rounding, half the bytes over PCIe, the aligned float loads on the device) -- on the small-call path and
    // in the staging threads of the large one
    const bool narrow = p->precision == 32 && x_dtype == PVX_F64;
    const int dev_dtype = narrow ? PVX_F32 : x_dtype;
    const size_t des = narrow ? 4 : es;

    auto chunk_geom = [&](int64_t c, int64_t& u0, int64_t& u1, size_t& in_off, size_t& in_bytes, int64_t& c_nsamp, int64_t& c_nsig, int64_t& c_frames) {
        u0 = c * per_chunk; u1 = u0 + per_chunk < units ? u0 + per_chunk : units;
        if (by_frames) {
            in_off = (size_t)u0 * p->hop * es;
            // frames u0 .. u1-1 need samples [u0 hop, (u1-1) hop + nfft]: nframes() is strict (PV.py:224-225), one more sample
            c_nsamp = (u1 - 1 - u0) * (int64_t)p->hop + p->nfft + 1;
            if ((int64_t)u0 * p->hop + c_nsamp > nsamp) c_nsamp = nsamp - u0 * (int64_t)p->hop;
            in_bytes = (size_t)c_nsamp * es;
            c_nsig = 1; c_frames = u1 - u0;
        } else {
            in_off = (size_t)u0 * sig_stride * es;
            c_nsig = u1 - u0; c_nsamp = nsamp; c_frames = (u1 - u0) * F;
            in_bytes = (size_t)((c_nsig - 1) * sig_stride + nsamp) * es;
        }
    };
    // results of chunk c (in d_out[c & 1]) -> the caller's arrays
    auto fetch = [&](int64_t c) -> int {
        int64_t u0, u1, c_nsamp, c_nsig, c_frames; size_t in_off, in_bytes;
        chunk_geom(c, u0, u1, in_off, in_bytes, c_nsamp, c_nsig, c_frames);
        PVX_HIP_CHECK(hipEventSynchronize(p->ev_done[c & 1]));
        const HostOut d = block_ptrs(p->d_out[c & 1].as<double>(), c_frames, K);
        const size_t r0 = by_frames ? (size_t)u0 : (size_t)u0 * F;
        const size_t nk = (size_t)c_frames * K * sizeof(double), n1 = (size_t)c_frames * sizeof(double);
        int rcc;
        if ((rcc = device_to_host(ho->f + r0 * K, d.f, nk)) != PVX_OK || (rcc = device_to_host(ho->mag + r0 * K, d.mag, nk)) != PVX_OK ||
            (rcc = device_to_host(ho->ph + r0 * K, d.ph, nk)) != PVX_OK || (rcc = device_to_host(ho->realph + r0 * K, d.realph, nk)) != PVX_OK ||
            (rcc = device_to_host(ho->binno + r0 * K, d.binno, nk)) != PVX_OK) return rcc;
        if (ho->totalmag && (rcc = device_to_host(ho->totalmag + r0, d.totalmag, n1)) != PVX_OK) return rcc;
        return PVX_OK;
    };

    const ProgressScope live(p);               // (nothing after the loop asks for progress_live)
    int64_t last_rows = 0;
    Route route = Route::none;                 // the last chunk's route and spectrum request
    SpecRequest spec;
    tr.mark("setup");
    for (int64_t c = 0; c < nchunks; c++) {
        const int b = (int)(c & 1);
        int64_t u0, u1, c_nsamp, c_nsig, c_frames; size_t in_off, in_bytes;
        chunk_geom(c, u0, u1, in_off, in_bytes, c_nsamp, c_nsig, c_frames);
        if (c >= 2) {
            // chunk c-2 used these buffers: its kernels are done (and its results fetched, below)
            if ((rc = (int)hipEventSynchronize(p->ev_done[b])) != 0) { pvx_set_error("hipEventSynchronize failed"); return PVX_ERR_HIP; }
        }
        if ((rc = p->d_in[b].grow(in_bytes, Sizing::headroom)) != PVX_OK) return rc;
        double* ob = nullptr;
        if (!keep) {
            if ((rc = p->d_out[b].grow((size_t)c_frames * per_frame_out, Sizing::headroom)) != PVX_OK) return rc;
            ob = p->d_out[b].as<double>();
        }
        if (small) {
            if ((rc = p->h_pin.grow(out_off + (keep ? 0 : total_out) + spec_pin, Sizing::exact)) != PVX_OK) return rc;
            // staged in pieces: the DMA of piece i runs under the host copy of piece i+1
            const size_t nel = in_bytes / es, piece = (size_t)64 << 10;
            for (size_t e0 = 0; e0 < nel; e0 += piece) {
                const size_t cnt = nel - e0 < piece ? nel - e0 : piece;
                if (narrow) {
                    narrow_f64_f32((const double*)x + e0, p->h_pin.as<float>() + e0, cnt);
                    tr.mark("  piece narrowed");
                } else {
                    memcpy(p->h_pin.as<char>() + e0 * es, (const char*)x + e0 * es, cnt * es);
                }
                PVX_HIP_CHECK(hipMemcpyAsync(p->d_in[b].as<char>() + e0 * des, p->h_pin.as<char>() + e0 * des, cnt * des, hipMemcpyHostToDevice, s));
            }
        } else {
            // pageable: concurrent with the kernels of chunk c-1 on the plan's stream; large chunks through the threaded ring
            const bool threaded = getenv("PVX_NO_STAGE_THREADS") == nullptr;
            if (narrow || (threaded && in_bytes >= kStageMin)) {
                if ((rc = staged_copy(p, p->d_in[b].get(), (void*)((const char*)x + in_off), narrow ? in_bytes / 2 : in_bytes, true, s, narrow)) != PVX_OK) return rc;
            } else {
                if ((rc = host_to_device(p->d_in[b].get(), (const char*)x + in_off, in_bytes)) != PVX_OK) return rc;
            }
        }
        tr.mark("staged + H2D issued");
        HostOut d;
        if (keep) {
            const HostOut all = block_ptrs(p->d_res.as<double>(), nsig * F, K);
            const size_t r0 = by_frames ? (size_t)u0 : (size_t)u0 * F;
            d.f = all.f + r0 * K; d.mag = all.mag + r0 * K; d.ph = all.ph + r0 * K; d.realph = all.realph + r0 * K;
            d.binno = all.binno + r0 * K; d.t = nchunks == 1 ? all.t : nullptr; d.totalmag = all.totalmag + r0;
        } else {
            d = block_ptrs(ob, c_frames, K);
            d.t = nullptr;
        }
        const double* dprev = (c > 0 && by_frames) || prev0 ? p->d_prev.as<double>() : nullptr;
        last_rows = c_nsig * (c_frames / c_nsig + 1);
        route = route_for(p, dev_dtype, last_rows);
        spec = SpecRequest{(c + 1 < nchunks && by_frames) || (last_spec && c + 1 == nchunks) ? last_rows - 1 : -1};
        // small call, fused kernels: the last spectrum is written by the kernel itself into the pinned block (one
        // 16 KB burst over PCIe instead of a separate copy operation behind the kernel)
        if (small && last_spec && is_fused(route) && spec_off + (size_t)p->N2 * 8 <= p->h_pin.cap()) spec.host = (float*)(p->h_pin.as<unsigned char>() + spec_off);
        rc = analyze_rows(p, route, p->d_in[b].get(), dev_dtype, c_nsamp, c_nsig, by_frames ? c_nsamp : sig_stride, c_frames / c_nsig,
                          d.f, d.mag, d.ph, d.realph, d.binno, d.t, d.totalmag, dprev, s, spec);
        tr.mark("kernels issued");
        if (rc == PVX_OK && c + 1 < nchunks && by_frames) rc = carry_spectrum(p, route, last_rows, s);
        if (rc != PVX_OK) return rc;
        PVX_HIP_CHECK(hipEventRecord(p->ev_done[b], s));
        if (!keep && !small && c >= 1) {
            if ((rc = fetch(c - 1)) != PVX_OK) return rc;      // under the kernels of chunk c
        }
        if (p->progress_fn && nchunks > 1 && c + 1 < nchunks) {
            const int64_t done = by_frames ? u1 : u1 * F;
            p->progress_fn(done, nsig * F, p->progress_user);
        }
    }
    // ---- tail: last chunk's results, frame times, the last spectrum
    if (keep) {
        const HostOut all = block_ptrs(p->d_res.as<double>(), nsig * F, K);
        if (nchunks > 1 && (rc = pvx_launch_fill_t(all.t, F, nsig, p->hop, p->nfft, p->sr, s)) != PVX_OK) return rc;   // else the kernels wrote it
        p->res_F = F; p->res_nsig = nsig; p->res_valid = true;
    } else if (small) {
        // one D2H of the whole block into pinned memory, one synchronisation, then plain memcpys
        double* hb = (double*)(p->h_pin.as<char>() + out_off);
        PVX_HIP_CHECK(hipMemcpyAsync(hb, p->d_out[0].as<double>(), total_out, hipMemcpyDeviceToHost, s));
        PVX_HIP_CHECK(hipStreamSynchronize(s));
        const HostOut h = block_ptrs(hb, nsig * F, K);
        const size_t nk = (size_t)nsig * F * K * sizeof(double), n1 = (size_t)nsig * F * sizeof(double);
        memcpy(ho->f, h.f, nk); memcpy(ho->mag, h.mag, nk); memcpy(ho->ph, h.ph, nk); memcpy(ho->realph, h.realph, nk);
        memcpy(ho->binno, h.binno, nk);
        if (ho->totalmag) memcpy(ho->totalmag, h.totalmag, n1);
    } else {
        if ((rc = fetch(nchunks - 1)) != PVX_OK) return rc;
    }
    if (!keep && ho->t) {
        for (int64_t b = 0; b < nsig; b++)
            for (int64_t fr = 0; fr < F; fr++) ho->t[b * F + fr] = ((double)(fr * (int64_t)p->hop) + p->nfft / 2.0) / p->sr;   // PV.py:247
    }
    // the spectrum of the last frame (PV.oldfft after the loop, PV.py:209), where the last chunk's route left it: in the pinned
    // block already when the fused kernel wrote it there; a small call's copy goes there too, under the one synchronisation below
    const SpecRow last = last_spec ? spec_row_at(p, route, last_rows - 1) : SpecRow{nullptr, false};
    const size_t last_bytes = (size_t)p->N2 * 2 * (last.f32 ? 4 : 8);
    unsigned char* h_last = (unsigned char*)spec.host;
    if (last_spec && small && !h_last && spec_off + last_bytes <= p->h_pin.cap()) {
        h_last = p->h_pin.as<unsigned char>() + spec_off;
        PVX_HIP_CHECK(hipMemcpyAsync(h_last, last.d, last_bytes, hipMemcpyDeviceToHost, s));
    }
    tr.mark("tail issued");
    PVX_HIP_CHECK(hipStreamSynchronize(s));
    tr.mark("synchronised");
    if (last_spec) {
        std::vector<unsigned char> tmp;
        if (!h_last) {
            tmp.resize(last_bytes);
            h_last = tmp.data();
            PVX_HIP_CHECK(hipMemcpy(h_last, last.d, last_bytes, hipMemcpyDeviceToHost));
        }
        for (int i = 0; i < 2 * p->N2; i++)
            last_spec[i] = last.f32 ? (double)((const float*)h_last)[i] : ((const double*)h_last)[i];
    }
    if (p->progress_fn) p->progress_fn(nsig * F, nsig * F, p->progress_user);
    return F;
}

extern "C" int64_t pvx_analyze(pvx_plan* p, const void* x, int x_dtype, int64_t nsamp, int64_t nsig, int64_t sig_stride,
                               double* f, double* mag, double* ph, double* realph, double* binno, double* t,
                               double* totalmag, const double* prev0, double* last_spec) {
    HostOut ho = {f, mag, ph, realph, binno, t, totalmag};
    return analyze_host(p, x, x_dtype, nsamp, nsig, sig_stride, &ho, prev0, last_spec, false);
}

// ---- many independent signals over the GPUs of this process (SURVEY.md 8(b) pvx_analyze_batch, 8(e)) ------------------
// The path shards by signal and has no exchange step: every device analyses whole signals and its results go straight to
// the caller's arrays, so the devices never talk to each other (no RCCL here: that is for callers that live in separate
// processes, pypevoc_amd/batch.py).  One queue, longest signal first; `workers` host threads per device, each with its own
// plan and stream, so one signal's transfers run under another's kernels; a worker takes the next signal when it is free,
// which balances ragged batches and unequal devices without a schedule.
static_assert(sizeof(pvx_batch_item) == 88, "pvx_batch_item is part of the C ABI");
struct pvx_batch {
    double sr = 0, pkthresh = 0;
    int nfft = 0, hop = 0, npks = 0, precision = 32, workers = 4;
    std::vector<double> win;
    std::vector<int> devices;
    std::vector<pvx_plan*> plans;          // [device slot][worker], created by the worker on its first signal
};

extern "C" int pvx_batch_create(pvx_batch** out, double sr, int nfft, int hop, int npks, double pkthresh, const double* win,
                                int precision, const int* devices, int ndev, int workers_per_device) {
    if (!out) { pvx_set_error("null batch pointer"); return PVX_ERR_INVALID; }
    *out = nullptr;
    if (nfft < 4 || hop <= 0 || npks <= 0 || !(sr > 0) || (precision != 32 && precision != 64) || ndev < 0 || (ndev > 0 && !devices) ||
        workers_per_device < 0 || workers_per_device > 8) {
        pvx_set_error("invalid batch parameters (sr=%g nfft=%d hop=%d npks=%d precision=%d ndev=%d workers=%d)", sr, nfft, hop, npks, precision, ndev, workers_per_device);
        return PVX_ERR_INVALID;
    }
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    int ndevices = 0;
    PVX_HIP_CHECK(hipGetDeviceCount(&ndevices));
    pvx_batch* b = new pvx_batch();
    b->sr = sr; b->nfft = nfft; b->hop = hop; b->npks = npks; b->pkthresh = pkthresh; b->precision = precision;
    b->workers = workers_per_device > 0 ? workers_per_device : 4;
    if (win) b->win.assign(win, win + nfft);
    if (ndev == 0) b->devices.push_back(t_device >= 0 ? t_device : g_device);
    for (int i = 0; i < ndev; i++) {
        const int d = devices[i];
        if (d < 0 || d >= ndevices || d >= kMaxDevices) { pvx_set_error("device %d out of range (%d devices)", d, ndevices); delete b; return PVX_ERR_INVALID; }
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            pvx_set_error("device %d is not a gfx950 (MI355X) device; libpvx_hip carries gfx950 code objects only", d);
            delete b;
            return PVX_ERR_NO_DEVICE;
        }
        b->devices.push_back(d);
    }
    b->plans.assign(b->devices.size() * (size_t)b->workers, nullptr);
    *out = b;
    return PVX_OK;
}

extern "C" int pvx_batch_destroy(pvx_batch* b) {
    if (!b) return PVX_OK;
    int cur = 0;
    const bool have = hipGetDevice(&cur) == hipSuccess;
    for (size_t i = 0; i < b->plans.size(); i++)
        if (b->plans[i]) { (void)hipSetDevice(b->devices[i / b->workers]); delete b->plans[i]; }
    if (have) (void)hipSetDevice(cur);
    delete b;
    return PVX_OK;
}

extern "C" int64_t pvx_batch_run(pvx_batch* b, int x_dtype, pvx_batch_item* items, int64_t nitems) {
    if (!b || nitems < 0 || (nitems > 0 && !items)) { pvx_set_error("invalid batch arguments"); return PVX_ERR_INVALID; }
    if (x_dtype != PVX_F32 && x_dtype != PVX_F64 && x_dtype != PVX_I16) { pvx_set_error("unknown sample type %d", x_dtype); return PVX_ERR_INVALID; }
    if (nitems == 0) return 0;
    // (no C++ exception may leave an extern "C" function: a bad_alloc of the two vectors, or of a worker's plan, is
    // PVX_ERR_ALLOC; threads already started are always joined)
    std::vector<int64_t> order;
    std::vector<std::thread> th;
    const int nw = (int)b->plans.size();
    try {
        order.resize((size_t)nitems);
        th.reserve((size_t)nw);
    } catch (...) { pvx_set_error("pvx_batch_run: out of host memory for %lld items", (long long)nitems); return PVX_ERR_ALLOC; }
    for (int64_t i = 0; i < nitems; i++) { order[(size_t)i] = i; items[i].nframes = 0; items[i].device = -1; }
    try {
        std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t c) { return items[a].nsamp > items[c].nsamp; });
    } catch (...) { pvx_set_error("pvx_batch_run: out of host memory for %lld items", (long long)nitems); return PVX_ERR_ALLOC; }
    std::atomic<int64_t> next(0);
    std::atomic<int> first_rc(PVX_OK);
    std::mutex err_mu;
    char err_text[512] = "";
    auto worker = [&](int w) {
        const int dev = b->devices[(size_t)(w / b->workers)];
        t_device = dev;
        auto fail = [&](int64_t item, int rc) {
            if (item >= 0) items[item].nframes = rc;
            int expect = PVX_OK;
            if (first_rc.compare_exchange_strong(expect, rc)) {
                std::lock_guard<std::mutex> lk(err_mu);
                snprintf(err_text, sizeof(err_text), "signal %lld on device %d: %s", (long long)item, dev, g_err);
            }
        };
        for (;;) {
            const int64_t q = next.fetch_add(1);
            if (q >= nitems) break;
            const int64_t i = order[(size_t)q];
            pvx_batch_item& it = items[i];
            try {
            it.device = dev;
            if (!b->plans[(size_t)w]) {
                const int rc = pvx_plan_create(&b->plans[(size_t)w], b->sr, b->nfft, b->hop, b->npks, b->pkthresh, b->win.empty() ? nullptr : b->win.data(), b->precision, 0);
                if (rc != PVX_OK) { fail(i, rc); continue; }
            }
            const int64_t F = pvx_analyze(b->plans[(size_t)w], it.x, x_dtype, it.nsamp, 1, it.nsamp, it.f, it.mag, it.ph, it.realph, it.binno, it.t, it.totalmag, nullptr, nullptr);
            if (F < 0) { fail(i, (int)F); continue; }
            it.nframes = F;
            } catch (...) { pvx_set_error("out of host memory"); fail(i, PVX_ERR_ALLOC); }
        }
        t_device = -1;
    };
    const int nthreads = (int64_t)nw < nitems ? nw : (int)nitems;
    // workers are dealt to the devices in turn (worker w -> slot w % ndev's next worker), so a batch smaller than the pool
    // still spreads over the devices
    const int nd = (int)b->devices.size();
    auto slot_of = [&](int k) { return (k % nd) * b->workers + k / nd; };
    const int saved = t_device;
    try {
        for (int k = 1; k < nthreads; k++) th.emplace_back(worker, slot_of(k));      // (th has its capacity: only thread creation can fail)
    } catch (...) { /* the threads that started and this one share the queue */ }
    worker(slot_of(0));
    t_device = saved;
    for (auto& t : th) t.join();
    (void)pvx_require_device();            // this thread served a device: back to the caller's
    if (first_rc.load() != PVX_OK) { pvx_set_error("%s", err_text); return first_rc.load(); }
    int64_t total = 0;
    for (int64_t i = 0; i < nitems; i++) total += items[i].nframes;
    return total;
}

extern "C" int64_t pvx_analyze_batch(double sr, int nfft, int hop, int npks, double pkthresh, const double* win, int precision,
                                     int x_dtype, pvx_batch_item* items, int64_t nitems, const int* devices, int ndev) {
    pvx_batch* b = nullptr;
    const int rc = pvx_batch_create(&b, sr, nfft, hop, npks, pkthresh, win, precision, devices, ndev, 0);
    if (rc != PVX_OK) return rc;
    const int64_t r = pvx_batch_run(b, x_dtype, items, nitems);
    pvx_batch_destroy(b);
    return r;
}

// ---- page-locked host arrays for results (the DMA engine writes them directly) ------------------------
extern "C" void* pvx_host_alloc(size_t bytes) {
    if (pvx_require_device() != PVX_OK) return nullptr;
    void* q = nullptr;
    if (hipHostMalloc(&q, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); pvx_set_error("hipHostMalloc(%zu) failed", bytes); return nullptr; }
    return q;
}
extern "C" void pvx_host_free(void* q) {
    if (q) (void)hipHostFree(q);
}

// ---- resident results ---------------------------------------------------------------------------
extern "C" int64_t pvx_analyze_resident(pvx_plan* p, const void* x, int x_dtype, int64_t nsamp, int64_t nsig,
                                        int64_t sig_stride, const double* prev0, double* last_spec) {
    return analyze_host(p, x, x_dtype, nsamp, nsig, sig_stride, nullptr, prev0, last_spec, true);
}

static int need_resident(pvx_plan* p) {
    if (!p) { pvx_set_error("null plan"); return PVX_ERR_INVALID; }
    if (!p->res_valid) { pvx_set_error("the plan holds no resident results (pvx_analyze_resident first)"); return PVX_ERR_INVALID; }
    return pvx_require_plan_device(p);
}

extern "C" int pvx_resident_fetch(pvx_plan* p, int which, double* host) {
    int rc = need_resident(p);
    if (rc != PVX_OK) return rc;
    if (!host || which < 0 || which > 6) { pvx_set_error("bad fetch argument"); return PVX_ERR_INVALID; }
    const int64_t rows = p->res_nsig * p->res_F;
    const HostOut all = block_ptrs(p->d_res.as<double>(), rows, p->npks);
    const double* src[7] = {all.f, all.mag, all.ph, all.realph, all.binno, all.t, all.totalmag};
    const size_t bytes = (size_t)rows * (which < 5 ? p->npks : 1) * sizeof(double);
    PVX_HIP_CHECK(hipStreamSynchronize(p->s_host));
    return device_to_host(host, src[which], bytes);
}

extern "C" const double* pvx_resident_ptr(pvx_plan* p, int which) {
    if (!p || !p->res_valid || which < 0 || which > 6) return nullptr;
    const HostOut all = block_ptrs(p->d_res.as<double>(), p->res_nsig * p->res_F, p->npks);
    const double* src[7] = {all.f, all.mag, all.ph, all.realph, all.binno, all.t, all.totalmag};
    return src[which];
}

extern "C" int pvx_stft_frames(pvx_plan* p, const void* x, int x_dtype, int64_t nsamp, const int64_t* pos, int64_t nfr,
                               double* spec) {
    int rc = pvx_require_plan_device(p);
    if (rc != PVX_OK) return rc;
    if (!p || !x || !pos || !spec || nfr < 0) { pvx_set_error("bad argument"); return PVX_ERR_INVALID; }
    if (x_dtype != PVX_F32 && x_dtype != PVX_F64 && x_dtype != PVX_I16) { pvx_set_error("bad x_dtype %d", x_dtype); return PVX_ERR_INVALID; }
    if ((rc = ensure_rocfft(p, false)) != PVX_OK) return rc;
    const size_t es = dtype_size(x_dtype), rs = real_size(p->precision);
    for (int64_t i = 0; i < nfr; i++)
        if (pos[i] < 0 || pos[i] + p->nfft > nsamp) { pvx_set_error("frame %lld at %lld leaves the signal", (long long)i, (long long)pos[i]); return PVX_ERR_INVALID; }
    // Each requested frame is framed as its own 1-frame "signal" (stride = its position), so the
    // regular framing kernel can be used: signal b = samples [pos[b], pos[b]+nfft+1).
    DevMem dx;
    if ((rc = dx.alloc((size_t)(p->nfft + 1) * es)) != PVX_OK) return rc;
    const int nb = p->nfft / 2 + 1;
    std::vector<unsigned char> row((size_t)nb * 2 * rs);
    for (int64_t i = 0; i < nfr; i++) {
        // copy nfft samples (+1 so that nframes(nfft+1) == 1)
        PVX_HIP_CHECK(hipMemset(dx.get(), 0, (size_t)(p->nfft + 1) * es));
        PVX_HIP_CHECK(hipMemcpy(dx.get(), (const char*)x + (size_t)pos[i] * es, (size_t)p->nfft * es, hipMemcpyHostToDevice));
        FrameParams fp;
        fp.x = dx.get(); fp.nsamp = p->nfft + 1; fp.sig_stride = p->nfft + 1; fp.F = 1; fp.R0 = 0; fp.ws_rows = 3;
        fp.total_rows = 2; fp.nfft = p->nfft; fp.hop = p->hop; fp.win = p->d_win.get(); fp.frames = p->d_frames.get(); fp.ldi = p->ldi;
        if (p->rocfft_rows < 2) { pvx_set_error("plan workspace too small"); return PVX_ERR_SIZE; }
        rc = pvx_launch_frames(fp, x_dtype, p->precision, nullptr);
        if (rc != PVX_OK) return rc;
        void* rspec = p->rocfft_small ? p->d_rspec.get() : p->d_spec.get();
        PVX_FFT_CHECK(p->fft.execute(p->d_frames.get(), rspec, nullptr));
        PVX_HIP_CHECK(hipStreamSynchronize(nullptr));
        // global row 1 (frame 0) sits in workspace row 2
        PVX_HIP_CHECK(hipMemcpy(row.data(), (char*)rspec + (size_t)2 * p->ldo * 2 * rs, row.size(), hipMemcpyDeviceToHost));
        double* o = spec + (size_t)i * nb * 2;
        for (int k = 0; k < 2 * nb; k++)
            o[k] = p->precision == 32 ? (double)((float*)row.data())[k] : ((double*)row.data())[k];
    }
    return PVX_OK;
}

// ---- PeakFinder -----------------------------------------------------------------------------
extern "C" int pvx_peakfinder(const double* y, int64_t nrows, int n, int npeaks, int thr_kind, double thr_val, int rad,
                              int32_t* pos, int8_t* keep, int32_t* count, int cap) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    if (!y || !pos || !keep || !count || nrows < 0 || n < 1 || cap < 1 || thr_kind < 0 || thr_kind > 2) {
        pvx_set_error("bad PeakFinder argument");
        return PVX_ERR_INVALID;
    }
    if (nrows == 0) return PVX_OK;
    DevMem dy, dpos, dkeep, dcount;
    const size_t yb = (size_t)nrows * n * sizeof(double);
    if ((rc = dy.alloc(yb)) != PVX_OK || (rc = dpos.alloc((size_t)nrows * cap * 4)) != PVX_OK ||
        (rc = dkeep.alloc((size_t)nrows * cap)) != PVX_OK || (rc = dcount.alloc((size_t)nrows * 4)) != PVX_OK)
        return rc;
    if ((rc = host_to_device(dy.get(), y, yb)) != PVX_OK) return rc;
    PVX_HIP_CHECK(hipMemset(dpos.get(), 0xff, (size_t)nrows * cap * 4));
    PVX_HIP_CHECK(hipMemset(dkeep.get(), 0, (size_t)nrows * cap));
    PeakRowsParams pp;
    pp.y = dy.as<const double>(); pp.nrows = nrows; pp.n = n; pp.npeaks = npeaks; pp.thr_kind = thr_kind;
    pp.thr_val = thr_val; pp.rad = rad; pp.cap = cap;
    pp.pos = dpos.as<int32_t>(); pp.keep = dkeep.as<int8_t>(); pp.count = dcount.as<int32_t>();
    rc = pvx_launch_peak_rows(pp, nullptr);
    if (rc != PVX_OK) return rc;
    PVX_HIP_CHECK(hipStreamSynchronize(nullptr));
    if ((rc = device_to_host(pos, dpos.get(), (size_t)nrows * cap * 4)) != PVX_OK || (rc = device_to_host(keep, dkeep.get(), (size_t)nrows * cap)) != PVX_OK ||
        (rc = device_to_host(count, dcount.get(), (size_t)nrows * 4)) != PVX_OK) return rc;
    return PVX_OK;
}

// ---- tracker: PV.toSinSum (PV.py:299-322) ---------------------------------------------------
static size_t track_ws_bytes(int64_t F, int K) {
    const size_t n = (size_t)F * K;
    // link, root: int32 [F*K]; newcount int32 [F]; newbase int64 [F+1]; npartials, ambiguous, maxend int64; succ [F*K]
    size_t off = n * 4 * 2 + (size_t)F * 4;
    off = (off + 7) & ~(size_t)7;
    off += ((size_t)F + 1) * 8 + 32 + n;
    off = (off + 7) & ~(size_t)7;
    const size_t nch = (size_t)(F + 127) / 128;                  // k_track_links_g8 / _lane: chunkbase int64 [nch + 1], chunktot / chunklast int32 [nch] (chunks of 128 or 256 frames)
    return off + (nch + 1) * 8 + nch * 8;
}

// the tracker on device arrays with a caller-provided workspace of track_ws_bytes(F, K); returns P
static int64_t track_on(const double* d_f, const double* d_mag, int64_t F, int K, double maxpitchjmp,
                        int32_t* d_partial_id, int32_t* d_part_start, int32_t* d_part_len, int64_t cap, char* w,
                        hipStream_t s, int64_t* maxend, int64_t* pinned3 = nullptr) {
    const size_t n = (size_t)F * K;
    const size_t off_link = 0, off_root = off_link + n * 4, off_cnt = off_root + n * 4;
    const size_t off_base = (off_cnt + (size_t)F * 4 + 7) & ~(size_t)7;
    const size_t off_np = off_base + ((size_t)F + 1) * 8, off_succ = off_np + 32;
    TrackParams tp;
    tp.f = d_f; tp.mag = d_mag; tp.F = F; tp.K = K; tp.maxjmp = maxpitchjmp;
    tp.partial_id = d_partial_id; tp.part_start = d_part_start; tp.part_len = d_part_len; tp.cap = cap;
    tp.link = (int32_t*)(w + off_link); tp.root = (int32_t*)(w + off_root);
    tp.succ = (unsigned char*)(w + off_succ); tp.newcount = (int32_t*)(w + off_cnt); tp.newbase = (int64_t*)(w + off_base);
    {
        const size_t nch = (size_t)(F + 127) / 128, off_cb = (off_succ + n + 7) & ~(size_t)7;
        tp.chunkbase = (int64_t*)(w + off_cb); tp.chunktot = (int32_t*)(w + off_cb + (nch + 1) * 8); tp.chunklast = tp.chunktot + nch;
    }
    // { partials, exact double tie met, last frame with a point }: three single stores by the kernels.  In page-locked
    // host memory when the caller has some (the resident chain): the host reads them after the one synchronisation,
    // no copy operation behind the kernels.
    // (the fourth word: k_track_links_lane's report of a frame too wide for it -- the call's number, see TrackParams::wide)
    int64_t pa_[4] = {0, 0, -1, 0};
    volatile int64_t* pa = pinned3 ? pinned3 : pa_;
    tp.npartials = pinned3 ? pinned3 : (int64_t*)(w + off_np);
    tp.ambiguous = tp.npartials + 1;
    tp.maxend = tp.npartials + 2;
    static std::atomic<unsigned> calls{0};
    tp.wide = (unsigned*)(tp.npartials + 3);
    tp.wide_dev = (unsigned*)(w + off_np + 24) + 1;              // (the workspace's own copy of the words is device memory either way)
    do { tp.gen = ++calls; } while (tp.gen == 0);
    if (K > 8) {                                                   // (rows of at most 8 slots never use the words)
        if (pinned3) pinned3[3] = 0;
        PVX_HIP_CHECK(hipMemsetAsync(w + off_np + 24, 0, 8, s));
    }
    int rc = pvx_launch_track(tp, s);
    if (rc != PVX_OK) return rc;
    if (!pinned3) PVX_HIP_CHECK(hipMemcpyAsync(pa_, tp.npartials, 32, hipMemcpyDeviceToHost, s));
    PVX_HIP_CHECK(hipStreamSynchronize(s));
    if ((unsigned)pa[3] == tp.gen) {
        // a frame with a valid peak beyond slot 7: the table of the wave-per-frame kernels instead
        tp.wide = nullptr;
        if ((rc = pvx_launch_track(tp, s)) != PVX_OK) return rc;
        if (!pinned3) PVX_HIP_CHECK(hipMemcpyAsync(pa_, tp.npartials, 24, hipMemcpyDeviceToHost, s));
        PVX_HIP_CHECK(hipStreamSynchronize(s));
    }
    if (pa[1] != 0 && getenv("PVX_TRACK_FORBID_SEQUENTIAL")) {      // tests: which tables the frame-parallel kernels hand over
        pvx_set_error("the frame-parallel tracker kernels left this table to k_track_sequential");
        return PVX_ERR_UNSUPPORTED;
    }
    if (pa[1] != 0 || getenv("PVX_TRACK_SEQUENTIAL")) {
        // an exact double tie (k_track.hip): the reference's order of the previous partials decides; redo the
        // table with the sequential kernel, which has the partial indices at hand
        if ((rc = pvx_launch_track_sequential(tp, s)) != PVX_OK) return rc;
        if (!pinned3) PVX_HIP_CHECK(hipMemcpyAsync(pa_, tp.npartials, 24, hipMemcpyDeviceToHost, s));
        PVX_HIP_CHECK(hipStreamSynchronize(s));
    }
    if (maxend) *maxend = pa[2];
    if (pa[0] > cap) { pvx_set_error("%lld partials exceed the table capacity %lld", (long long)pa[0], (long long)cap); return PVX_ERR_SIZE; }
    return pa[0];
}

extern "C" int64_t pvx_track_dev(const double* d_f, const double* d_mag, int64_t F, int K, double maxpitchjmp,
                                 int32_t* d_partial_id, int32_t* d_part_start, int32_t* d_part_len, int64_t cap,
                                 void* stream) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    if (F < 0 || K <= 0 || cap < 0) { pvx_set_error("bad tracker argument"); return PVX_ERR_INVALID; }
    if (F == 0) return 0;
    if (!d_f || !d_mag || !d_partial_id || !d_part_start || !d_part_len) { pvx_set_error("null tracker array"); return PVX_ERR_INVALID; }
    // the workspace of the plan-less tracker is kept (allocating and freeing it cost as much as the kernels); the call is
    // synchronous, one at a time through it
    // (one workspace per DEVICE: a thread bound to another device must not hand its kernels a buffer of this one; the result
    // words are page-locked memory every device can write: hipHostMallocPortable)
    static std::mutex mu;
    static std::map<int, DevMem*> wsd;      // (for the process: never deleted, pvx_mem.h)
    static int64_t* pin3 = nullptr;         // { partials, exact double tie, last frame with a point } in page-locked memory:
    std::lock_guard<std::mutex> lk(mu);     // the kernel's three stores are what the host waits for, no copy behind them
    if (!pin3 && hipHostMalloc((void**)&pin3, 64, hipHostMallocPortable) != hipSuccess) { pin3 = nullptr; (void)hipGetLastError(); }
    int dev = 0;
    PVX_HIP_CHECK(hipGetDevice(&dev));
    DevMem* w = nullptr;
    try { DevMem*& e = wsd[dev]; if (!e) e = new DevMem(); w = e; } catch (...) { pvx_set_error("out of memory for the tracker's per-device workspace record"); return PVX_ERR_ALLOC; }   // (no C++ exception leaves the C ABI)
    if ((rc = w->grow(track_ws_bytes(F, K), Sizing::headroom)) != PVX_OK) return rc;
    return track_on(d_f, d_mag, F, K, maxpitchjmp, d_partial_id, d_part_start, d_part_len, cap, w->as<char>(), (hipStream_t)stream, nullptr, pin3);
}

extern "C" int pvx_synth_dev_flags(const double* d_f, const double* d_mag, const double* d_realph, const int32_t* d_partial_id,
                             int64_t F, int K, const int32_t* d_part_start, const int32_t* d_part_len, int64_t P,
                             double sr, int nfft, int hop_analysis, int hop_synth, double edge, int minframes,
                             double* d_w, int64_t wlen, void* stream, int flags);
extern "C" int64_t pvx_synth_len(int64_t max_end_frame, int nfft, int hop_analysis, int hop_synth, double edge);
static int synth_slice(const double* d_f, const double* d_mag, const double* d_realph, const int32_t* d_partial_id, int64_t F, int K,
                       const int32_t* d_part_start, const int32_t* d_part_len, int64_t P, double sr, int nfft, int hop_analysis, int hop_synth,
                       double edge, int minframes, double* d_w, int64_t wlen, hipStream_t stream, int64_t seg0, int64_t seg_count, bool first,
                       void* ws, size_t ws_bytes, unsigned* ws_gen, int f32_samples);
// plans at precision 32 resynthesise with the float32 sample loop (k_synth_bodies<R, float>: the stated waveform tolerance there is
// 1e-4 max|w|); PVX_SYNTH_F64=1: the float64 loop whatever the plan's precision (tests, A/B)
static int plan_synth_f32(const pvx_plan* p);

// ---- the chain on resident results: toSinSum -> synth, descriptors -------------------------------
extern "C" int64_t pvx_track_resident(pvx_plan* p, double maxpitchjmp, int64_t* max_end_frame) {
    int rc = need_resident(p);
    if (rc != PVX_OK) return rc;
    if (p->res_nsig != 1) { pvx_set_error("the tracker works on one signal (resident results hold %lld)", (long long)p->res_nsig); return PVX_ERR_INVALID; }
    const int64_t F = p->res_F;
    const int K = p->npks;
    const size_t n = (size_t)F * K;
    if (n > p->trk_cap) {
        p->d_pid.reset(); p->d_pst.reset(); p->d_pln.reset(); p->trk_cap = 0;
        if (p->d_pid.alloc(n * 4) != PVX_OK || p->d_pst.alloc(n * 4) != PVX_OK || p->d_pln.alloc(n * 4) != PVX_OK) {
            pvx_set_error("hipMalloc of the partial table failed"); return PVX_ERR_ALLOC;
        }
        p->trk_cap = n;
    }
    if ((rc = p->d_tws.grow(track_ws_bytes(F, K), Sizing::headroom)) != PVX_OK) return rc;
    const HostOut all = block_ptrs(p->d_res.as<double>(), F, K);
    int64_t maxend = -1;
    if ((rc = p->h_pin.grow(64, Sizing::exact)) != PVX_OK) return rc;
    HostTrace tr("track");
    const int64_t P = track_on(all.f, all.mag, F, K, maxpitchjmp, p->d_pid.as<int32_t>(), p->d_pst.as<int32_t>(), p->d_pln.as<int32_t>(), (int64_t)n, p->d_tws.as<char>(), p->s_host, &maxend,
                               p->h_pin.as<int64_t>());
    tr.mark("launched + synchronised");
    if (P < 0) return P;
    p->res_P = P; p->res_maxend = maxend;
    if (max_end_frame) *max_end_frame = maxend;
    return P;
}

extern "C" int pvx_resident_fetch_table(pvx_plan* p, int32_t* partial_id, int32_t* part_start, int32_t* part_len) {
    int rc = need_resident(p);
    if (rc != PVX_OK) return rc;
    if (p->res_P < 0) { pvx_set_error("no resident partial table (pvx_track_resident first)"); return PVX_ERR_INVALID; }
    PVX_HIP_CHECK(hipStreamSynchronize(p->s_host));
    if (partial_id && (rc = device_to_host(partial_id, p->d_pid.as<int32_t>(), (size_t)p->res_F * p->npks * 4)) != PVX_OK) return rc;
    if (part_start && p->res_P && (rc = device_to_host(part_start, p->d_pst.as<int32_t>(), (size_t)p->res_P * 4)) != PVX_OK) return rc;
    if (part_len && p->res_P && (rc = device_to_host(part_len, p->d_pln.as<int32_t>(), (size_t)p->res_P * 4)) != PVX_OK) return rc;
    return PVX_OK;
}

extern "C" int pvx_synth_resident(pvx_plan* p, double sr, int hop_synth, double edge, int minframes, double* w, int64_t wlen) {
    int rc = need_resident(p);
    if (rc != PVX_OK) return rc;
    if (p->res_P < 0) { pvx_set_error("no resident partial table (pvx_track_resident first)"); return PVX_ERR_INVALID; }
    if (!w || hop_synth <= 0 || !(sr > 0)) { pvx_set_error("bad resynthesis argument"); return PVX_ERR_INVALID; }
    if (p->res_P == 0) { pvx_set_error("max() arg is an empty sequence"); return PVX_ERR_INVALID; }          // PV.py:1059
    const int64_t need = pvx_synth_len(p->res_maxend, p->nfft, p->hop, hop_synth, edge);
    if (need < 0 || need != wlen) { pvx_set_error("output length %lld, expected %lld", (long long)wlen, (long long)need); return PVX_ERR_SIZE; }
    HostTrace tr("synth");
    {
        const void* before = p->d_sws.get();
        const size_t cap_before = p->d_sws.cap();
        if ((rc = p->d_sws.grow(pvx_synth_ws_bytes(p->res_F, p->npks, p->res_P, p->nfft, p->hop, hop_synth, edge), Sizing::headroom)) != PVX_OK) return rc;
        if (p->d_sws.get() != before || p->d_sws.cap() != cap_before) p->sws_gen = 0;           // a new buffer: its flags are cleared on first use
    }
    const HostOut all = block_ptrs(p->d_res.as<double>(), p->res_F, p->npks);
    const int32_t *pid = p->d_pid.as<int32_t>(), *pst = p->d_pst.as<int32_t>(), *pln = p->d_pln.as<int32_t>();
    const size_t bytes = (size_t)wlen * 8;
    hipPointerAttribute_t attr;
    const bool pinned = hipPointerGetAttributes(&attr, w) == hipSuccess && attr.type == hipMemoryTypeHost;
    if (!pinned) (void)hipGetLastError();                        // an ordinary pointer is reported as an error
    // (off by default since the attacks / releases reach the waveform in a launch of their own and k_synth_bodies reads them
    // back: over PCIe that costs more than the DMA it saves -- config 3: 0.21 ms against 0.17 ms)
    static const bool zero_copy = getenv("PVX_SYNTH_ZEROCOPY") != nullptr;
    if (pinned && zero_copy && bytes <= kSmallCall) {
        // the caller's array is page-locked (pvx_host_alloc) and small: the kernel stores its segments straight into
        // it (posted writes over PCIe, spread over the kernel's run time as workgroups finish) -- no copy operation
        // behind the kernel at all
        rc = synth_slice(all.f, all.mag, all.realph, pid, p->res_F, p->npks, pst, pln, p->res_P, sr, p->nfft,
                         p->hop, hop_synth, edge, minframes, w, wlen, p->s_host, 0, 0, true, p->d_sws.get(), p->d_sws.cap(), &p->sws_gen, plan_synth_f32(p));
        if (rc != PVX_OK) return rc;
        tr.mark("kernel issued");
        PVX_HIP_CHECK(hipStreamSynchronize(p->s_host));
        tr.mark("here");
        return PVX_OK;
    }
    if ((rc = p->d_w.grow((size_t)wlen * 8, Sizing::headroom)) != PVX_OK) return rc;
    if (pinned && bytes >= kStageMin && getenv("PVX_NO_SYNTH_SLICES") == nullptr) {
        // a large waveform into page-locked memory: the segments are computed in slices and the DMA of a finished slice
        // (second stream) runs under the next slice's kernel -- the link, not kernel + link, is what the call costs
        if ((rc = stage_ring(p)) != PVX_OK) return rc;                   // (its events)
        PVX_HIP_CHECK(p->s_copy.ensure(hipStreamNonBlocking));
        const int NS = 8;                                                // slices (ev_ring holds 16 events)
        const int64_t nseg = (wlen + hop_synth - 1) / hop_synth, per = (nseg + NS - 1) / NS;
        for (int i = 0; i < NS; i++) {
            const int64_t s0 = (int64_t)i * per;
            if (s0 >= nseg) break;
            const int64_t cnt = nseg - s0 < per ? nseg - s0 : per;
            rc = synth_slice(all.f, all.mag, all.realph, pid, p->res_F, p->npks, pst, pln, p->res_P, sr, p->nfft, p->hop, hop_synth,
                             edge, minframes, p->d_w.as<double>(), wlen, p->s_host, s0, cnt, i == 0, p->d_sws.get(), p->d_sws.cap(), &p->sws_gen, plan_synth_f32(p));
            if (rc != PVX_OK) return rc;
            PVX_HIP_CHECK(hipEventRecord(p->ev_ring[i], p->s_host));
            PVX_HIP_CHECK(hipStreamWaitEvent(p->s_copy, p->ev_ring[i], 0));
            const int64_t o = s0 * hop_synth, c = (wlen - o < cnt * hop_synth) ? wlen - o : cnt * hop_synth;
            PVX_HIP_CHECK(hipMemcpyAsync(w + o, p->d_w.as<double>() + o, (size_t)c * 8, hipMemcpyDeviceToHost, p->s_copy));
        }
        tr.mark("slices + copies issued");
        PVX_HIP_CHECK(hipStreamSynchronize(p->s_copy));
        PVX_HIP_CHECK(hipStreamSynchronize(p->s_host));
        tr.mark("here");
        return PVX_OK;
    }
    rc = synth_slice(all.f, all.mag, all.realph, pid, p->res_F, p->npks, pst, pln, p->res_P, sr, p->nfft,
                     p->hop, hop_synth, edge, minframes, p->d_w.as<double>(), wlen, p->s_host, 0, 0, true, p->d_sws.get(), p->d_sws.cap(), &p->sws_gen, plan_synth_f32(p));
    if (rc != PVX_OK) return rc;
    if (pinned) {
        // the caller's array is page-locked: the DMA lands in it, nothing to stage or copy
        PVX_HIP_CHECK(hipMemcpyAsync(w, p->d_w.as<double>(), bytes, hipMemcpyDeviceToHost, p->s_host));
        tr.mark("kernel + copy issued");
        PVX_HIP_CHECK(hipStreamSynchronize(p->s_host));
        tr.mark("here");
        return PVX_OK;
    }
    if (bytes <= kSmallCall) {
        // through pinned memory in pieces: the host copy of piece i runs under the DMA of piece i+1 (two events in turn)
        if ((rc = p->h_pin.grow(bytes, Sizing::exact)) != PVX_OK) return rc;
        const size_t piece = bytes > ((size_t)256 << 10) ? ((bytes + 3) / 4 + 255) & ~(size_t)255 : bytes;
        const int np_ = (int)((bytes + piece - 1) / piece);
        auto issue = [&](int i) -> int {
            const size_t o = (size_t)i * piece, c = bytes - o < piece ? bytes - o : piece;
            PVX_HIP_CHECK(hipMemcpyAsync(p->h_pin.as<char>() + o, p->d_w.as<const char>() + o, c, hipMemcpyDeviceToHost, p->s_host));
            PVX_HIP_CHECK(hipEventRecord(p->ev_done[i & 1], p->s_host));
            return PVX_OK;
        };
        if ((rc = issue(0)) != PVX_OK) return rc;
        if (np_ > 1 && (rc = issue(1)) != PVX_OK) return rc;
        tr.mark("kernel + copies issued");
        for (int i = 0; i < np_; i++) {
            const size_t o = (size_t)i * piece, c = bytes - o < piece ? bytes - o : piece;
            PVX_HIP_CHECK(hipEventSynchronize(p->ev_done[i & 1]));
            if (i + 2 < np_ && (rc = issue(i + 2)) != PVX_OK) return rc;       // its event is free again
            memcpy((char*)w + o, p->h_pin.as<const char>() + o, c);
        }
        tr.mark("copied out");
    } else {
        const bool threaded = getenv("PVX_NO_STAGE_THREADS") == nullptr;
        if (threaded && bytes >= kStageMin) {
            // (the DMAs are queued behind the kernel on the same stream)
            if ((rc = staged_copy(p, p->d_w.as<double>(), w, bytes, false, p->s_host)) != PVX_OK) return rc;
            tr.mark("copied out (threaded ring)");
        } else {
            PVX_HIP_CHECK(hipStreamSynchronize(p->s_host));
            if ((rc = device_to_host(w, p->d_w.as<double>(), bytes)) != PVX_OK) return rc;
        }
    }
    return PVX_OK;
}

// PV.calc_f0 (PV.py:371-391) on the resident arrays: fm float64 [F], idx int32 [F] come back, nothing else moves
extern "C" int pvx_f0_resident(pvx_plan* p, double fmin, double fmax, double thr, double* fm, int32_t* idx) {
    int rc = need_resident(p);
    if (rc != PVX_OK) return rc;
    if (!fm || !idx) { pvx_set_error("null output array"); return PVX_ERR_INVALID; }
    const int64_t rows = p->res_nsig * p->res_F;
    if ((rc = p->d_desc.grow((size_t)rows * 12, Sizing::headroom)) != PVX_OK) return rc;
    const HostOut all = block_ptrs(p->d_res.as<double>(), rows, p->npks);
    double* d_fm = p->d_desc.as<double>();
    int32_t* d_im = (int32_t*)(d_fm + rows);
    if ((rc = pvx_launch_f0(all.f, all.mag, rows, p->npks, fmin, fmax, thr, d_fm, d_im, p->s_host)) != PVX_OK) return rc;
    PVX_HIP_CHECK(hipStreamSynchronize(p->s_host));
    if ((rc = device_to_host(fm, d_fm, (size_t)rows * 8)) != PVX_OK || (rc = device_to_host(idx, d_im, (size_t)rows * 4)) != PVX_OK) return rc;
    return PVX_OK;
}

// PV.calc_harmonic_power (PV.py:266-297) on the resident arrays: hpower, nharmonics float64 [F, K].
// Returns PVX_ERR_SIZE where the reference raises IndexError (a valid peak slot >= number of frames, PV.py:278).
extern "C" int pvx_harmonic_power_resident(pvx_plan* p, double f_threshold, double* hpower, double* nharm) {
    int rc = need_resident(p);
    if (rc != PVX_OK) return rc;
    if (!hpower || !nharm) { pvx_set_error("null output array"); return PVX_ERR_INVALID; }
    if (p->res_nsig != 1) { pvx_set_error("calc_harmonic_power works on one signal"); return PVX_ERR_INVALID; }
    const int64_t F = p->res_F;
    const int K = p->npks;
    const size_t n = (size_t)F * K;
    if ((rc = p->d_desc.grow(n * 16 + (size_t)K * 8 + 16, Sizing::headroom)) != PVX_OK) return rc;
    const HostOut all = block_ptrs(p->d_res.as<double>(), F, K);
    double* d_hp = p->d_desc.as<double>();
    double* d_nh = d_hp + n;
    double* d_rp = d_nh + n;
    int32_t* d_top = (int32_t*)(d_rp + K);
    if ((rc = pvx_launch_hpower_rows(all.f, all.mag, F, K, d_rp, d_top, p->s_host)) != PVX_OK) return rc;
    int32_t top = -1;
    PVX_HIP_CHECK(hipMemcpyAsync(&top, d_top, 4, hipMemcpyDeviceToHost, p->s_host));
    PVX_HIP_CHECK(hipStreamSynchronize(p->s_host));
    if (top >= F) { pvx_set_error("index %d is out of bounds for axis 0 with size %lld", (int)top, (long long)F); return PVX_ERR_SIZE; }
    if ((rc = pvx_launch_hpower(all.f, F, K, f_threshold, d_rp, d_hp, d_nh, p->s_host)) != PVX_OK) return rc;
    PVX_HIP_CHECK(hipStreamSynchronize(p->s_host));
    if ((rc = device_to_host(hpower, d_hp, n * 8)) != PVX_OK || (rc = device_to_host(nharm, d_nh, n * 8)) != PVX_OK) return rc;
    return PVX_OK;
}

extern "C" int64_t pvx_track(const double* f, const double* mag, int64_t F, int K, double maxpitchjmp,
                             int32_t* partial_id, int32_t* part_start, int32_t* part_len, int64_t cap) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    if (F < 0 || K <= 0 || cap < 0) { pvx_set_error("bad tracker argument"); return PVX_ERR_INVALID; }
    if (F == 0) return 0;
    if (!f || !mag || !partial_id || !part_start || !part_len) { pvx_set_error("null tracker array"); return PVX_ERR_INVALID; }
    const size_t n = (size_t)F * K;
    const int64_t dcap = (int64_t)n;           // always sufficient on the device side
    DevMem df, dm, dpid, dst, dln;
    if ((rc = df.alloc(n * 8)) != PVX_OK || (rc = dm.alloc(n * 8)) != PVX_OK || (rc = dpid.alloc(n * 4)) != PVX_OK ||
        (rc = dst.alloc(n * 4)) != PVX_OK || (rc = dln.alloc(n * 4)) != PVX_OK)
        return rc;
    if ((rc = host_to_device(df.get(), f, n * 8)) != PVX_OK || (rc = host_to_device(dm.get(), mag, n * 8)) != PVX_OK) return rc;
    const int64_t P = pvx_track_dev(df.as<const double>(), dm.as<const double>(), F, K, maxpitchjmp, dpid.as<int32_t>(),
                                    dst.as<int32_t>(), dln.as<int32_t>(), dcap, nullptr);
    if (P < 0) return P;
    if (P > cap) { pvx_set_error("%lld partials exceed the caller's capacity %lld", (long long)P, (long long)cap); return PVX_ERR_SIZE; }
    if ((rc = device_to_host(partial_id, dpid.get(), n * 4)) != PVX_OK || (rc = device_to_host(part_start, dst.get(), (size_t)P * 4)) != PVX_OK ||
        (rc = device_to_host(part_len, dln.get(), (size_t)P * 4)) != PVX_OK) return rc;
    return P;
}

// ---- PVHarmonic.run_pv (PV.py:493-535): f0-guided analysis on the general path's spectra ------
static int harmonic_rows(pvx_plan* p, const void* d_x, int x_dtype, int64_t nsamp, int64_t F, const double* f0,
                         double fmin, double* d_f, double* d_mag, double* d_ph, double* d_res, double* d_t,
                         const double* d_prev0, hipStream_t s, bool* any_valid) {
    int rc;
    if ((rc = has_stft(p) ? ensure_spec_ws(p) : ensure_rocfft(p, true)) != PVX_OK) return rc;
    const size_t rs = real_size(p->precision);
    // previous-valid-frame table (PV.py:509, 491: oldfft only moves on analysed frames)
    std::vector<int32_t> prow((size_t)F);
    int64_t last = -1;
    for (int64_t fr = 0; fr < F; fr++) {
        const int64_t R0 = ((fr + 1) / p->max_rows) * p->max_rows;      // chunk holding row fr+1
        if (last < 0) prow[fr] = -1;
        else if (last + 1 >= R0 - 1) prow[fr] = (int32_t)(last + 1 - R0 + 1);
        else prow[fr] = -2;
        const double v = f0[fr];
        if (v > 0.0) {
            if (v / p->sr * (double)p->nfft < 0.5) {
                pvx_set_error("f0[%lld] = %g Hz is below half a bin (%g Hz): the harmonic series is not resolvable", (long long)fr, v, 0.5 * p->fstep);
                return PVX_ERR_INVALID;
            }
            last = fr;
        }
    }
    *any_valid = last >= 0;
    if (F > p->harm_cap) {
        p->d_hf0.reset(); p->d_hprev.reset(); p->harm_cap = 0;
        if (p->d_hf0.alloc((size_t)F * 8) != PVX_OK || p->d_hprev.alloc((size_t)F * 4) != PVX_OK) {
            pvx_set_error("hipMalloc of the f0 tables failed"); return PVX_ERR_ALLOC;
        }
        p->harm_cap = F;
    }
    if (!p->d_carry && p->d_carry.alloc((size_t)p->ldo * 2 * rs) != PVX_OK) { pvx_set_error("hipMalloc(carry) failed"); return PVX_ERR_ALLOC; }
    PVX_HIP_CHECK(hipMemcpyAsync(p->d_hf0.as<double>(), f0, (size_t)F * 8, hipMemcpyHostToDevice, s));
    PVX_HIP_CHECK(hipMemcpyAsync(p->d_hprev.as<int32_t>(), prow.data(), (size_t)F * 4, hipMemcpyHostToDevice, s));
    PVX_HIP_CHECK(hipStreamSynchronize(s));                              // prow is a local
    const int64_t total_rows = F + 1;
    for (int64_t R0 = 0; R0 < total_rows; R0 += p->max_rows) {
        const int64_t nrows = (total_rows - R0 < p->max_rows) ? (total_rows - R0) : p->max_rows;
        FrameParams fp;
        fp.x = d_x; fp.nsamp = nsamp; fp.sig_stride = nsamp; fp.F = F; fp.R0 = R0;
        fp.ws_rows = nrows + 1; fp.total_rows = total_rows; fp.nfft = p->nfft; fp.hop = p->hop;
        fp.win = p->d_win.get(); fp.frames = p->d_frames.get(); fp.ldi = p->ldi;
        if ((rc = launch_transform(p, fp, x_dtype, s)) != PVX_OK || (rc = plan_event(p, s, -1)) != PVX_OK) return rc;
        HarmParams hp;
        hp.spec = p->d_spec.get(); hp.ldo = p->ldo;
        hp.fr_begin = (R0 > 1 ? R0 : 1) - 1;
        const int64_t fr_last = R0 + nrows - 2;
        hp.nfr = fr_last - hp.fr_begin + 1;
        hp.ws_off = hp.fr_begin + 1 - R0 + 1;
        hp.nfft = p->nfft; hp.hop = p->hop; hp.N2 = p->N2; hp.K = p->npks;
        hp.sr = p->sr; hp.fstep = p->fstep; hp.dt = p->dt; hp.fmin = fmin;
        hp.wfbin = p->d_wfbin.as<double>(); hp.prev0 = d_prev0; hp.carry = p->d_carry.get();
        hp.f0 = p->d_hf0.as<double>(); hp.prevrow = p->d_hprev.as<int32_t>();
        hp.f = d_f; hp.mag = d_mag; hp.ph = d_ph; hp.residual = d_res; hp.t = d_t;
        if ((rc = pvx_launch_harmonic(hp, p->precision, s)) != PVX_OK) return rc;
        // carry the spectrum of the last valid frame of this chunk to the later ones
        int64_t lv = fr_last;
        while (lv >= hp.fr_begin && !(f0[lv] > 0.0)) lv--;
        if (lv >= hp.fr_begin)
            PVX_HIP_CHECK(hipMemcpyAsync(p->d_carry.get(), p->d_spec.as<const char>() + (size_t)(lv + 1 - R0 + 1) * p->ldo * 2 * rs,
                                         (size_t)p->ldo * 2 * rs, hipMemcpyDeviceToDevice, s));
        if ((rc = plan_progress(p, s, R0 + nrows, total_rows, 1)) != PVX_OK) return rc;
    }
    return PVX_OK;
}

static int check_harmonic_args(pvx_plan* p, const void* x, int x_dtype, int64_t nsamp, const double* f0, int64_t nf0, int64_t F) {
    int rc = check_analyze_args(p, x, x_dtype, nsamp, 1, nsamp, nullptr);
    if (rc != PVX_OK) return rc;
    if (F > 0 && (!f0 || nf0 < F)) {
        // the reference indexes f0[int(curpos/hop)] (PV.py:507) and raises IndexError
        pvx_set_error("index %lld is out of bounds for f0 with size %lld", (long long)(nf0 < 0 ? 0 : nf0), (long long)nf0);
        return PVX_ERR_SIZE;
    }
    return PVX_OK;
}

extern "C" int64_t pvx_harmonic_analyze_dev(pvx_plan* p, const void* d_x, int x_dtype, int64_t nsamp, const double* f0,
                                            int64_t nf0, double fmin, double* d_f, double* d_mag, double* d_ph,
                                            double* d_residual, double* d_t, const double* d_prev0, void* stream) {
    int rc = pvx_require_plan_device(p);
    if (rc != PVX_OK) return rc;
    if (!p) { pvx_set_error("null plan"); return PVX_ERR_INVALID; }
    const int64_t F = pvx_nframes(nsamp, p->nfft, p->hop);
    if ((rc = check_harmonic_args(p, d_x, x_dtype, nsamp, f0, nf0, F)) != PVX_OK) return rc;
    if (F == 0) return 0;
    if (!d_f || !d_mag || !d_ph || !d_residual) { pvx_set_error("null output array"); return PVX_ERR_INVALID; }
    bool any = false;
    rc = harmonic_rows(p, d_x, x_dtype, nsamp, F, f0, fmin, d_f, d_mag, d_ph, d_residual, d_t, d_prev0, (hipStream_t)stream, &any);
    return rc == PVX_OK ? F : rc;
}

extern "C" int64_t pvx_harmonic_analyze(pvx_plan* p, const void* x, int x_dtype, int64_t nsamp, const double* f0, int64_t nf0,
                                        double fmin, double* f, double* mag, double* ph, double* residual, double* t,
                                        const double* prev0, double* last_spec) {
    int rc = pvx_require_plan_device(p);
    if (rc != PVX_OK) return rc;
    if (!p) { pvx_set_error("null plan"); return PVX_ERR_INVALID; }
    const int64_t F = pvx_nframes(nsamp, p->nfft, p->hop);
    if ((rc = check_harmonic_args(p, x, x_dtype, nsamp, f0, nf0, F)) != PVX_OK) return rc;
    if (F == 0) return 0;
    if (!f || !mag || !ph || !residual) { pvx_set_error("null output array"); return PVX_ERR_INVALID; }
    const size_t xbytes = (size_t)nsamp * dtype_size(x_dtype);
    const size_t fk = (size_t)F * p->npks * sizeof(double), f1 = (size_t)F * sizeof(double);
    HostTrace tr("harmonic");
    DevMem dout, dprev;
    if ((rc = p->d_hx.grow(xbytes, Sizing::headroom)) != PVX_OK) return rc;
    void* const d_x = p->d_hx.get();
    if ((rc = dout.alloc(3 * fk + 2 * f1)) != PVX_OK) return rc;
    tr.mark("device buffers");
    if ((rc = host_to_device(d_x, x, xbytes)) != PVX_OK) return rc;
    tr.mark("signal on the device");
    if (prev0) {
        if ((rc = dprev.alloc(sizeof(double) * 2 * p->N2)) != PVX_OK) return rc;
        PVX_HIP_CHECK(hipMemcpy(dprev.get(), prev0, sizeof(double) * 2 * p->N2, hipMemcpyHostToDevice));
    }
    char* o = dout.as<char>();
    double *d_f = (double*)o, *d_mag = (double*)(o + fk), *d_ph = (double*)(o + 2 * fk), *d_res = (double*)(o + 3 * fk),
           *d_t = (double*)(o + 3 * fk + f1);
    bool any = false;
    {
        const ProgressScope live(p);
        rc = harmonic_rows(p, d_x, x_dtype, nsamp, F, f0, fmin, d_f, d_mag, d_ph, d_res, d_t, dprev.as<const double>(), nullptr, &any);
    }
    if (rc != PVX_OK) return rc;
    PVX_HIP_CHECK(hipStreamSynchronize(nullptr));
    tr.mark("kernels");
    if ((rc = device_to_host(f, d_f, fk)) != PVX_OK || (rc = device_to_host(mag, d_mag, fk)) != PVX_OK || (rc = device_to_host(ph, d_ph, fk)) != PVX_OK ||
        (rc = device_to_host(residual, d_res, f1)) != PVX_OK) return rc;
    if (t && (rc = device_to_host(t, d_t, f1)) != PVX_OK) return rc;
    tr.mark("results on the host");
    if (last_spec) {
        // oldfft after the loop = spectrum of the last analysed frame (PV.py:491), else unchanged
        if (any) {
            const size_t rs = real_size(p->precision);
            std::vector<unsigned char> tmp((size_t)p->N2 * 2 * rs);
            PVX_HIP_CHECK(hipMemcpy(tmp.data(), p->d_carry.get(), tmp.size(), hipMemcpyDeviceToHost));
            for (int i = 0; i < 2 * p->N2; i++)
                last_spec[i] = p->precision == 32 ? (double)((float*)tmp.data())[i] : ((double*)tmp.data())[i];
        } else {
            for (int i = 0; i < 2 * p->N2; i++) last_spec[i] = prev0 ? prev0[i] : 0.0;
        }
    }
    if (p->progress_fn) p->progress_fn(F, F, p->progress_user);
    return F;
}

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
    DevMem dx, dh, dout, dic;
    if ((rc = dx.alloc((size_t)n * 8)) != PVX_OK || (rc = dh.alloc((size_t)n * 16)) != PVX_OK ||
        (rc = dout.alloc((size_t)nfr * 16)) != PVX_OK || (rc = dic.alloc((size_t)nfr * 8)) != PVX_OK) return rc;
    if ((rc = host_to_device(dx.get(), x, (size_t)n * 8)) != PVX_OK || (rc = host_to_device(dh.get(), hetsig, (size_t)n * 16)) != PVX_OK) return rc;
    const int64_t r = pvx_heterodyne_dev(dx.as<const double>(), dh.as<const double>(), n, wind, wlen, hop, dout.as<double>(),
                                         dic.as<int64_t>(), nullptr);
    if (r < 0) return r;
    if ((rc = device_to_host(out, dout.get(), (size_t)nfr * 16)) != PVX_OK) return rc;
    if (icent && (rc = device_to_host(icent, dic.get(), (size_t)nfr * 8)) != PVX_OK) return rc;
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
    DevMem dx, dout;
    if ((rc = dx.alloc((size_t)n * 8)) != PVX_OK || (rc = dout.alloc((size_t)nfr * 8)) != PVX_OK) return rc;
    if ((rc = host_to_device(dx.get(), x, (size_t)n * 8)) != PVX_OK) return rc;
    const int64_t r = pvx_rms_frames_dev(dx.as<const double>(), n, wind, wlen, hop, dout.as<double>(), nullptr);
    if (r < 0) return r;
    if ((rc = device_to_host(out, dout.get(), (size_t)nfr * 8)) != PVX_OK) return rc;
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
    DevMem dx, dout;
    if ((rc = dx.alloc(xb)) != PVX_OK || (rc = dout.alloc(ob)) != PVX_OK) return rc;
    if ((rc = host_to_device(dx.get(), x, xb)) != PVX_OK) return rc;
    const int64_t r = pvx_funcwind_dev(dx.as<const double>(), x_complex, n, wind, wlen, hop, func, divisor, dout.as<double>(), nullptr);
    if (r < 0) return r;
    if ((rc = device_to_host(out, dout.get(), ob)) != PVX_OK) return rc;
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
    DevMem dx, df, da, dic;
    if ((rc = dx.alloc((size_t)n * 8)) != PVX_OK || (rc = df.alloc((size_t)n * 8)) != PVX_OK || (rc = da.alloc(ab)) != PVX_OK ||
        (rc = dic.alloc((size_t)nfr * 8)) != PVX_OK) return rc;
    if ((rc = host_to_device(dx.get(), x, (size_t)n * 8)) != PVX_OK || (rc = host_to_device(df.get(), fvec, (size_t)n * 8)) != PVX_OK) return rc;
    const int64_t r = pvx_hetharm_dev(dx.as<const double>(), n, df.as<const double>(), wind, wlen, hop, first, count, halve_dc, da.as<double>(),
                                      dic.as<int64_t>(), nullptr);
    if (r < 0) return r;
    if ((rc = device_to_host(ah, da.get(), ab)) != PVX_OK) return rc;
    if (icent && (rc = device_to_host(icent, dic.get(), (size_t)nfr * 8)) != PVX_OK) return rc;
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
    DevMem df, da, dy, dh;
    if ((rc = df.alloc((size_t)n * 8)) != PVX_OK || (rc = da.alloc(ab)) != PVX_OK || (rc = dy.alloc((size_t)n * 8)) != PVX_OK ||
        (hf && (rc = dh.alloc((size_t)n * 16)) != PVX_OK)) return rc;
    if ((rc = host_to_device(df.get(), fvec, (size_t)n * 8)) != PVX_OK || (rc = host_to_device(da.get(), ah, ab)) != PVX_OK) return rc;
    const int64_t r = pvx_hetharm_resynth_dev(df.as<const double>(), n, da.as<const double>(), nfr, nharm_total, wlen, hop, first, count, filter, sr,
                                              fmin, fmax, ampthr, dy.as<double>(), hf ? dh.as<double>() : nullptr, nullptr);
    if (r < 0) return r;
    if ((rc = device_to_host(y, dy.get(), (size_t)n * 8)) != PVX_OK) return rc;
    if (hf && (rc = device_to_host(hf, dh.get(), (size_t)n * 16)) != PVX_OK) return rc;
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
    DevMem dx, dp, ds, dn, dq;
    if ((rc = dx.alloc((size_t)nsamp * 8)) != PVX_OK || (rc = dp.alloc(cb)) != PVX_OK || (rc = ds.alloc(cb)) != PVX_OK ||
        (rc = dn.alloc(ib)) != PVX_OK || (rc = dq.alloc(ib)) != PVX_OK) return rc;
    if ((rc = host_to_device(dx.get(), x, (size_t)nsamp * 8)) != PVX_OK) return rc;
    const int64_t r = pvx_periodicity_dev(dx.as<const double>(), nsamp, wind, nwind, idx, nidx, method, cand_method, mindelay, maxdelay, threshold,
                                          vthresh, ncand, fftthresh, dp.as<double>(), ds.as<double>(), dn.as<int32_t>(), dq.as<int32_t>(), nullptr);
    if (r < 0) return r;
    if ((rc = device_to_host(cand_period, dp.get(), cb)) != PVX_OK || (rc = device_to_host(cand_strength, ds.get(), cb)) != PVX_OK ||
        (rc = device_to_host(ncands, dn.get(), ib)) != PVX_OK || (rc = device_to_host(preferred, dq.get(), ib)) != PVX_OK) return rc;
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
    DevMem dx, df, dc, dt, dg, dk;
    if ((rc = dx.alloc((size_t)nsamp * 8)) != PVX_OK || (rc = df.alloc(db)) != PVX_OK || (rc = dc.alloc(db)) != PVX_OK ||
        (tau && (rc = dt.alloc(db)) != PVX_OK) || (flag && (rc = dg.alloc(ib)) != PVX_OK) || (pick && (rc = dk.alloc(ib)) != PVX_OK)) return rc;
    if ((rc = host_to_device(dx.get(), x, (size_t)nsamp * 8)) != PVX_OK) return rc;
    const int64_t r = pvx_yin_dev(dx.as<const double>(), nsamp, starts, nfr, nwind, lo, hi, tol, sr, df.as<double>(), dc.as<double>(),
                                  tau ? dt.as<double>() : nullptr, flag ? dg.as<int32_t>() : nullptr, pick ? dk.as<int32_t>() : nullptr, nullptr);
    if (r < 0) return r;
    if ((rc = device_to_host(freq, df.get(), db)) != PVX_OK || (rc = device_to_host(conf, dc.get(), db)) != PVX_OK ||
        (tau && (rc = device_to_host(tau, dt.get(), db)) != PVX_OK) || (flag && (rc = device_to_host(flag, dg.get(), ib)) != PVX_OK) ||
        (pick && (rc = device_to_host(pick, dk.get(), ib)) != PVX_OK)) return rc;
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
    DevMem dx, dm, dc, ds;
    if ((rc = dx.alloc((size_t)nsamp * 8)) != PVX_OK || (rc = dm.alloc(mb)) != PVX_OK || (rc = dc.alloc(ib)) != PVX_OK ||
        (rc = ds.alloc(ib)) != PVX_OK) return rc;
    if ((rc = host_to_device(dx.get(), x, (size_t)nsamp * 8)) != PVX_OK) return rc;
    PVX_HIP_CHECK(hipMemsetAsync(dm.get(), 0, mb, nullptr));          // the padding behind a row's marks reads as 0
    const int64_t r = pvx_marks_corr_dev(dx.as<const double>(), nsamp, row_start, row_stop, t0, toff, nrows, tf, f, ntf, f_fallback, sr,
                                         window, min_per, max_marks, max_steps, dm.as<double>(), dc.as<int32_t>(), ds.as<int32_t>(), nullptr);
    if (r < 0) return r;
    if ((rc = device_to_host(marks, dm.get(), mb)) != PVX_OK || (rc = device_to_host(count, dc.get(), ib)) != PVX_OK ||
        (rc = device_to_host(status, ds.get(), ib)) != PVX_OK) return rc;
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
    DevMem dx, dm, dv, dc, ds;
    if ((rc = dx.alloc((size_t)nsamp * 8)) != PVX_OK || (rc = dm.alloc(mb)) != PVX_OK || (rc = dv.alloc(mb)) != PVX_OK ||
        (rc = dc.alloc(ib)) != PVX_OK || (rc = ds.alloc(ib)) != PVX_OK) return rc;
    if ((rc = host_to_device(dx.get(), x, (size_t)nsamp * 8)) != PVX_OK) return rc;
    PVX_HIP_CHECK(hipMemsetAsync(dm.get(), 0, mb, nullptr));
    PVX_HIP_CHECK(hipMemsetAsync(dv.get(), 0, mb, nullptr));
    const int64_t r = pvx_marks_peak_dev(dx.as<const double>(), nsamp, row_start, row_stop, toff, nrows, tf, f, ntf, nf, sr, fit_points,
                                         max_marks, max_steps, dm.as<double>(), dv.as<double>(), dc.as<int32_t>(), ds.as<int32_t>(), nullptr);
    if (r < 0) return r;
    if ((rc = device_to_host(marks, dm.get(), mb)) != PVX_OK || (rc = device_to_host(vals, dv.get(), mb)) != PVX_OK ||
        (rc = device_to_host(count, dc.get(), ib)) != PVX_OK || (rc = device_to_host(status, ds.get(), ib)) != PVX_OK) return rc;
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
    size_t limit = (size_t)2 << 30;                                   // per buffer
    if (const char* e = getenv("PVX_MAX_DEVICE_BYTES")) { const long long v = atoll(e); if (v > 0) limit = (size_t)v; }
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
        if ((rc = host_to_device(dx.get(), (const char*)x + (size_t)(f0 * hop) * es, (size_t)((cnt - 1) * hop + nwind) * es)) != PVX_OK) return rc;
        if ((rc = pvx_fbank_run(dx.get(), x_dtype, cnt, wind, nwind, hop, fb, nband, cep_mode, spec ? ds.as<double>() : nullptr,
                                cep ? dc.as<double>() : nullptr, nullptr, &t_fbank_kernels)) != PVX_OK) return rc;
        if (spec && (rc = device_to_host((char*)spec + (size_t)f0 * sb, ds.get(), (size_t)cnt * sb)) != PVX_OK) return rc;
        if (cep && (rc = device_to_host((char*)cep + (size_t)f0 * cb, dc.get(), (size_t)cnt * cb)) != PVX_OK) return rc;
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
    size_t limit = (size_t)2 << 30;                                   // per buffer
    if (const char* e = getenv("PVX_MAX_DEVICE_BYTES")) { const long long v = atoll(e); if (v > 0) limit = (size_t)v; }
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
        if ((rc = host_to_device(dx.get(), (const char*)x + (size_t)(f0 * hop) * es, (size_t)((cnt - 1 + extra) * hop + nwind) * es)) != PVX_OK) return rc;
        if ((rc = pvx_specdesc_run(dx.get(), x_dtype, cnt, wind, nwind, hop, measure, a, b, dout.as<double>(), f0 == 0,
                                   f0 + cnt == nfr ? nfr : 0, nullptr, &t_specdesc_kernels)) != PVX_OK) return rc;
        if (!psd && (rc = device_to_host((char*)out + (size_t)f0 * 8, dout.get(), (size_t)cnt * 8)) != PVX_OK) return rc;
    }
    if (psd && (rc = device_to_host(out, dout.get(), (size_t)(nwind / 2) * 8)) != PVX_OK) return rc;
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
    size_t limit = (size_t)2 << 30;                                   // per buffer
    if (const char* e = getenv("PVX_MAX_DEVICE_BYTES")) { const long long v = atoll(e); if (v > 0) limit = (size_t)v; }
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
        if ((rc = host_to_device(dx.get(), (const char*)x + off, bytes)) != PVX_OK) return rc;
        if (y && (rc = host_to_device(dy.get(), (const char*)y + off, bytes)) != PVX_OK) return rc;
        if ((rc = pvx_xspec_run(dx.get(), y ? dy.get() : nullptr, x_dtype, wind, nwind, step, delta, cnt, nseg, dxy.as<double>(), dxx.as<double>(),
                                dyy.as<double>(), nullptr, &t_xspec_kernels)) != PVX_OK) return rc;
        if ((rc = device_to_host((char*)sxx + (size_t)(b0 * nhalf) * 8, dxx.get(), (size_t)(cnt * nhalf) * 8)) != PVX_OK) return rc;
        if (y && ((rc = device_to_host((char*)syy + (size_t)(b0 * nhalf) * 8, dyy.get(), (size_t)(cnt * nhalf) * 8)) != PVX_OK ||
                  (rc = device_to_host((char*)sxy + (size_t)(b0 * nhalf) * 16, dxy.get(), (size_t)(cnt * nhalf) * 16)) != PVX_OK)) return rc;
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
    size_t limit = (size_t)2 << 30;
    if (const char* e = getenv("PVX_MAX_DEVICE_BYTES")) { const long long v = atoll(e); if (v > 0) limit = (size_t)v; }
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
        if ((rc = host_to_device(dx.get(), (const char*)x + (size_t)lo * es, (size_t)(hi - lo) * es)) != PVX_OK) return rc;
        if ((rc = pvx_fric_run(dx.get(), x_dtype, rel.data(), cnt, L, nwind, win, sr, freq, psd ? dpsd.as<double>() : nullptr,
                               tail ? ddesc.as<double>() : nullptr, dim.as<int32_t>(), dst.as<int32_t>(), drms.as<double>(), nullptr,
                               &t_fric_kernels)) != PVX_OK) return rc;
        if (psd && (rc = device_to_host((char*)psd + (size_t)(r0 * nhalf) * 8, dpsd.get(), (size_t)(cnt * nhalf) * 8)) != PVX_OK) return rc;
        if (tail && ((rc = device_to_host((char*)desc + (size_t)r0 * 56, ddesc.get(), (size_t)cnt * 56)) != PVX_OK ||
                     (rc = device_to_host((char*)imax + (size_t)r0 * 4, dim.get(), (size_t)cnt * 4)) != PVX_OK ||
                     (rc = device_to_host((char*)status + (size_t)r0 * 4, dst.get(), (size_t)cnt * 4)) != PVX_OK ||
                     (rc = device_to_host((char*)rms + (size_t)r0 * 8, drms.get(), (size_t)cnt * 8)) != PVX_OK)) return rc;
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
    size_t limit = (size_t)2 << 30;
    if (const char* e = getenv("PVX_MAX_DEVICE_BYTES")) { const long long v = atoll(e); if (v > 0) limit = (size_t)v; }
    const int64_t rc_rows = std::min<int64_t>(nrows, std::max<int64_t>(1, (int64_t)(limit / ((size_t)nb * 8))));
    DevMem dpsd, ddesc, dim, dst;
    if ((rc = dpsd.alloc((size_t)(rc_rows * nb) * 8)) != PVX_OK || (rc = ddesc.alloc((size_t)rc_rows * 56)) != PVX_OK ||
        (rc = dim.alloc((size_t)rc_rows * 4)) != PVX_OK || (rc = dst.alloc((size_t)rc_rows * 4)) != PVX_OK) return rc;
    const int nper = 2 * (nb - 1);
    for (int64_t r0 = 0; r0 < nrows; r0 += rc_rows) {
        const int64_t cnt = std::min(rc_rows, nrows - r0);
        if ((rc = host_to_device(dpsd.get(), (const char*)psd + (size_t)(r0 * nb) * 8, (size_t)(cnt * nb) * 8)) != PVX_OK) return rc;
        if ((rc = pvx_fric_run(nullptr, PVX_F64, nullptr, cnt, nper, nper, nullptr, 1.0, freq, dpsd.as<double>(), ddesc.as<double>(),
                               dim.as<int32_t>(), dst.as<int32_t>(), nullptr, nullptr, &t_fric_kernels)) != PVX_OK) return rc;
        if ((rc = device_to_host((char*)desc + (size_t)r0 * 56, ddesc.get(), (size_t)cnt * 56)) != PVX_OK ||
            (rc = device_to_host((char*)imax + (size_t)r0 * 4, dim.get(), (size_t)cnt * 4)) != PVX_OK ||
            (rc = device_to_host((char*)status + (size_t)r0 * 4, dst.get(), (size_t)cnt * 4)) != PVX_OK) return rc;
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
    size_t limit = (size_t)2 << 30;                                   // per buffer
    if (const char* e = getenv("PVX_MAX_DEVICE_BYTES")) { const long long x = atoll(e); if (x > 0) limit = (size_t)x; }
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
        if ((rc = host_to_device(da.get(), (const char*)a + off, (size_t)((cnt - 1) * delta + la) * es)) != PVX_OK ||
            (rc = host_to_device(dv.get(), (const char*)v + off, (size_t)((cnt - 1) * delta + lv) * es)) != PVX_OK) return rc;
        if ((rc = pvx_xcorr_run(da.get(), dv.get(), x_dtype, la, lv, delta, cnt, detrend, win_a, win_v, use_abs, dlag.as<int32_t>(), dpeak.as<double>(),
                                corr ? dcorr.as<double>() : nullptr, nullptr, &t_xcorr_kernels)) != PVX_OK) return rc;
        if ((rc = device_to_host((char*)lag + (size_t)b0 * 4, dlag.get(), (size_t)cnt * 4)) != PVX_OK ||
            (rc = device_to_host((char*)peak + (size_t)b0 * 8, dpeak.get(), (size_t)cnt * 8)) != PVX_OK) return rc;
        if (corr && (rc = device_to_host((char*)corr + (size_t)(b0 * nlag) * 8, dcorr.get(), (size_t)(cnt * nlag) * 8)) != PVX_OK) return rc;
    }
    return nblk;
}

// ---- linear prediction and glottal inverse filtering (k_iaif.hip) -------------------------------
static thread_local const char* t_iaif_kernels = "";
extern "C" const char* pvx_iaif_last_kernels(void) { return t_iaif_kernels; }

static size_t iaif_limit() {
    size_t limit = (size_t)256 << 20;                                 // per buffer
    if (const char* e = getenv("PVX_MAX_DEVICE_BYTES")) { const long long v = atoll(e); if (v > 0) limit = (size_t)v; }
    return limit;
}

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

// rows of `bytes` each from a device buffer to the caller's: on the stream (DEV), or to the host before the return
template <bool DEV> static int rows_out(void* dst, const void* src, size_t bytes, hipStream_t s) {
    if (!dst || bytes == 0) return PVX_OK;
    if (!DEV) return device_to_host(dst, src, bytes);
    PVX_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
    return PVX_OK;
}
template <bool DEV> static int zero_out(double* dst, int64_t count, hipStream_t s) {
    if (!dst || count <= 0) return PVX_OK;
    if (!DEV) { memset(dst, 0, (size_t)count * 8); return PVX_OK; }
    PVX_HIP_CHECK(hipMemsetAsync(dst, 0, (size_t)count * 8, s));
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
    const size_t es = dtype_size(x_dtype), limit = iaif_limit();
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
            if ((rc = host_to_device(dx.get(), cx, (size_t)((nf - 1) * hop + nwind) * es)) != PVX_OK) return rc;
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
    const size_t es = dtype_size(x_dtype), limit = iaif_limit(), rb = (size_t)(order + 1) * 8;
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
            if ((rc = host_to_device(dx.get(), cx, (size_t)((cnt - 1) * hop + nwind) * es)) != PVX_OK) return rc;
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
        if (!DEV && (rc = device_to_host((char*)coef + (size_t)f0 * rb, dc.get(), (size_t)cnt * rb)) != PVX_OK) return rc;
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
    const size_t es = dtype_size(x_dtype), limit = iaif_limit();
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
            if ((rc = host_to_device(dx.get(), (const char*)x + (size_t)lo * es, (size_t)(hi - lo) * es)) != PVX_OK) return rc;
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
            if ((nkept && (rc = device_to_host(nkept + r0, wk.get(), k * 4)) != PVX_OK) ||
                (freq && (rc = device_to_host(freq + r0 * P, wf.get(), k * P * 8)) != PVX_OK) ||
                (bw && (rc = device_to_host(bw + r0 * P, wb.get(), k * P * 8)) != PVX_OK) ||
                (re && (rc = device_to_host(re + r0 * P, wr.get(), k * P * 8)) != PVX_OK) ||
                (im && (rc = device_to_host(im + r0 * P, wi.get(), k * P * 8)) != PVX_OK) ||
                (lpc && (rc = device_to_host(lpc + r0 * (P + 1), wl.get(), k * (P + 1) * 8)) != PVX_OK)) return rc;
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
        rc_rows = std::min(n, std::max<int64_t>(1, (int64_t)(iaif_limit() / rb)));
        if ((rc = dc.alloc((size_t)rc_rows * rb)) != PVX_OK || (rc = wr.alloc((size_t)rc_rows * P * 8)) != PVX_OK ||
            (rc = wi.alloc((size_t)rc_rows * P * 8)) != PVX_OK || (rc = wk.alloc((size_t)rc_rows * 4)) != PVX_OK ||
            (rc = wst.alloc((size_t)rc_rows * 4)) != PVX_OK) return rc;
    }
    for (int64_t r0 = 0; r0 < n; r0 += rc_rows) {
        const int64_t cnt = std::min(rc_rows, n - r0);
        const size_t o = (size_t)r0, k = (size_t)cnt;
        int64_t noc = -1, lead = -1;
        if (!DEV) {
            if ((rc = host_to_device(dc.get(), coef + o * (P + 1), k * rb)) != PVX_OK) return rc;
            rc = pvx_polyroots_run(dc.as<double>(), cnt, order, wr.as<double>(), wi.as<double>(), wk.as<int>(), wst.as<int>(), &noc, &lead, s,
                                   &t_formants_kernels);
        } else {
            rc = pvx_polyroots_run(coef + o * (P + 1), cnt, order, re ? re + o * P : nullptr, im ? im + o * P : nullptr, nkept ? nkept + o : nullptr,
                                   status ? status + o : nullptr, &noc, &lead, s, &t_formants_kernels);
        }
        if (rc != PVX_OK) return rc;
        if (!DEV) {
            if ((re && (rc = device_to_host(re + o * P, wr.get(), k * P * 8)) != PVX_OK) ||
                (im && (rc = device_to_host(im + o * P, wi.get(), k * P * 8)) != PVX_OK) ||
                (nkept && (rc = device_to_host(nkept + o, wk.get(), k * 4)) != PVX_OK) ||
                (status && (rc = device_to_host(status + o, wst.get(), k * 4)) != PVX_OK)) return rc;
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
    if ((npk && (rc = device_to_host(npk + o, d.k.get(), k * 4)) != PVX_OK) ||
        (idx && maxpk && (rc = device_to_host(idx + o * maxpk, d.i.get(), k * maxpk * 4)) != PVX_OK) ||
        (pos && maxpk && (rc = device_to_host(pos + o * maxpk, d.p.get(), k * maxpk * 8)) != PVX_OK) ||
        (val && maxpk && (rc = device_to_host(val + o * maxpk, d.v.get(), k * maxpk * 8)) != PVX_OK)) return rc;
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
        own = std::min(n, std::max<int64_t>(1, (int64_t)(iaif_limit() / std::max(std::max(rb, K * 8), env ? N * 8 : (size_t)8))));
        if ((rc = dc.alloc((size_t)own * rb)) != PVX_OK || (env && (rc = de.alloc((size_t)own * N * 8)) != PVX_OK) ||
            (rc = dl.alloc((size_t)own, K, npk != nullptr, idx != nullptr, pos != nullptr, val != nullptr)) != PVX_OK) return rc;
    }
    for (int64_t r0 = 0; r0 < n; r0 += own) {
        const int64_t cnt = std::min(own, n - r0);
        const size_t o = (size_t)r0, k = (size_t)cnt;
        int64_t over = -1, bad = -1;
        if (!DEV) {
            if ((rc = host_to_device(dc.get(), coef + o * (P + 1), k * rb)) != PVX_OK) return rc;
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
            if ((env && (rc = device_to_host(env + o * N, de.get(), k * N * 8)) != PVX_OK) ||
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
        own = std::min(n, std::max<int64_t>(1, (int64_t)(iaif_limit() / std::max(N * 8, K * 8))));
        if ((rc = dy.alloc((size_t)own * N * 8)) != PVX_OK || (x && (rc = dx.alloc(N * 8)) != PVX_OK) ||
            (sel && (rc = ds.alloc((size_t)own * K * 4)) != PVX_OK) ||
            (rc = dl.alloc((size_t)own, K, npk != nullptr, idx != nullptr, pos != nullptr, val != nullptr)) != PVX_OK) return rc;
        if (x && (rc = host_to_device(dx.get(), x, N * 8)) != PVX_OK) return rc;
    }
    for (int64_t r0 = 0; r0 < n; r0 += own) {
        const int64_t cnt = std::min(own, n - r0);
        const size_t o = (size_t)r0, k = (size_t)cnt;
        int64_t over = -1, bad = -1;
        if (!DEV) {
            if ((rc = host_to_device(dy.get(), y + o * N, k * N * 8)) != PVX_OK ||
                (sel && K && (rc = host_to_device(ds.get(), sel + o * K, k * K * 4)) != PVX_OK)) return rc;
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
        if ((rc = host_to_device(ds.get(), spec, sb)) != PVX_OK) return rc;
        if ((rc = pvx_seg_detect_run(ds.as<double>(), nfr, nband, thresh, maxseg, det ? dd.as<double>() : nullptr, idx ? di.as<int>() : nullptr,
                                     fpos ? dp.as<double>() : nullptr, &total, s, &t_segment_kernels)) != PVX_OK) return rc;
        const size_t got = (size_t)std::min<int64_t>(total, maxseg);
        if ((det && (rc = device_to_host(det, dd.get(), nd * 8)) != PVX_OK) || (idx && got && (rc = device_to_host(idx, di.get(), got * 4)) != PVX_OK) ||
            (fpos && got && (rc = device_to_host(fpos, dp.get(), got * 8)) != PVX_OK)) return rc;
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
    if (sb && (rc = host_to_device(ds.get(), spec, sb)) != PVX_OK) return rc;
    if ((rc = pvx_seg_refine_run(ds.as<double>(), nfine, nband, ranges, tseg, nseg, hop, half, tsr, sr, thr, has_thr, valb ? db.as<double>() : nullptr,
                                 vala ? da.as<double>() : nullptr, cross ? dc.as<int>() : nullptr, out ? dout.as<double>() : nullptr, s,
                                 &t_segment_kernels)) != PVX_OK) return rc;
    if ((valb && (rc = device_to_host(valb, db.get(), cells * 8)) != PVX_OK) || (vala && (rc = device_to_host(vala, da.get(), cells * 8)) != PVX_OK) ||
        (cross && (rc = device_to_host(cross, dc.get(), cells * 4)) != PVX_OK) || (out && (rc = device_to_host(out, dout.get(), (size_t)nseg * 8)) != PVX_OK)) return rc;
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
    if ((rc = host_to_device(dv.get(), v, span * 8)) != PVX_OK) return rc;
    if ((rc = pvx_seg_transitions_run(dv.as<double>(), nser, n, row_stride, elem_stride, escale, tx, tx_stride, trt, mode, pct, thr, d1.as<double>(),
                                      d2.as<double>(), d3.as<double>(), d4.as<int>(), s, &t_segment_kernels)) != PVX_OK) return rc;
    if ((rc = device_to_host(ttr, d1.get(), ob)) != PVX_OK || (rc = device_to_host(vbef, d2.get(), ob)) != PVX_OK ||
        (rc = device_to_host(vaft, d3.get(), ob)) != PVX_OK || (rc = device_to_host(status, d4.get(), (size_t)nser * 4)) != PVX_OK) return rc;
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

// a host array on the device for the length of a call (nullptr stays nullptr)
struct Staged {
    DevMem mem;
    int put(const void* host, size_t bytes) {
        int rc;
        if (!host) return PVX_OK;
        if ((rc = mem.alloc(bytes ? bytes : 8)) != PVX_OK) return rc;
        return bytes ? host_to_device(mem.get(), host, bytes) : PVX_OK;
    }
    int room(size_t bytes) { return mem.alloc(bytes ? bytes : 8); }
    int get(void* host, size_t bytes) { return bytes ? device_to_host(host, mem.get(), bytes) : PVX_OK; }
};

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
    if ((rc = pvx_jump_select_run(dmag.mem.as<double>(), df0.mem.as<double>(), dt.mem.as<double>(), len ? dlen.mem.as<int>() : nullptr, rows, nmax, K, thr,
                                  dm.mem.as<double>(), di.mem.as<int>(), dts.mem.as<double>(), dfs.mem.as<double>(), dn.mem.as<int>(), dst.mem.as<int>(),
                                  s, &t_jumps_kernels)) != PVX_OK) return rc;
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

// the selection on a plan's resident mag and t (one signal): f0 goes up, five F-sized arrays come back
extern "C" int64_t pvx_jump_select_resident(pvx_plan* p, const double* f0, double mag_threshold, double* m, int32_t* isel, double* tsel,
                                            double* fsel, int32_t* nsel, int32_t* status) {
    t_jumps_kernels = "";
    int rc = need_resident(p);
    if (rc != PVX_OK) return rc;
    if (p->res_nsig != 1) { pvx_set_error("pvx_jump_select_resident works on one signal (resident results hold %lld)", (long long)p->res_nsig); return PVX_ERR_INVALID; }
    if (!f0 || !m || !isel || !tsel || !fsel || !nsel || !status) { pvx_set_error("null pvx_jump_select_resident array"); return PVX_ERR_INVALID; }
    if (p->npks > PVX_JUMP_MAX_K) { pvx_set_error("pvx_jump_select_resident: %d peaks per frame (the kernel takes up to %d)", p->npks, PVX_JUMP_MAX_K); return PVX_ERR_UNSUPPORTED; }
    const int64_t F = p->res_F;
    if (F > 0x7fffffffLL) { pvx_set_error("pvx_jump_select_resident: %lld frames", (long long)F); return PVX_ERR_UNSUPPORTED; }
    const size_t n = (size_t)F;
    if ((rc = p->d_desc.grow(n * 36 + 16, Sizing::headroom)) != PVX_OK) return rc;
    const HostOut all = block_ptrs(p->d_res.as<double>(), F, p->npks);
    double* d_f0 = p->d_desc.as<double>();                           // f0 | m | tsel | fsel | isel | nsel, status
    double *d_m = d_f0 + n, *d_ts = d_m + n, *d_fs = d_ts + n;
    int32_t* d_is = (int32_t*)(d_fs + n);
    int32_t* d_ns = d_is + n;
    PVX_HIP_CHECK(hipMemcpyAsync(d_f0, f0, n * 8, hipMemcpyHostToDevice, p->s_host));
    if ((rc = pvx_jump_select_run(all.mag, d_f0, all.t, nullptr, 1, (int)F, p->npks, mag_threshold, d_m, d_is, d_ts, d_fs, d_ns, d_ns + 1, p->s_host,
                                  &t_jumps_kernels)) != PVX_OK) return rc;
    int32_t tail[2];
    if ((rc = device_to_host(m, d_m, n * 8)) != PVX_OK || (rc = device_to_host(isel, d_is, n * 4)) != PVX_OK ||
        (rc = device_to_host(tsel, d_ts, n * 8)) != PVX_OK || (rc = device_to_host(fsel, d_fs, n * 8)) != PVX_OK ||
        (rc = device_to_host(tail, d_ns, 8)) != PVX_OK) return rc;
    *nsel = tail[0];
    *status = tail[1];
    return 1;
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
    if ((rc = pvx_winstat_run(dt.mem.as<double>(), dx.mem.as<double>(), len ? dlen.mem.as<int>() : nullptr, rows, nmax, kind, wl, wr, hop, flags,
                              dout.mem.as<double>(), s, &t_jumps_kernels)) != PVX_OK) return rc;
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
        if ((rc = device_to_host(counts.data(), njump, (size_t)rows * 4)) != PVX_OK) return rc;
        got = counts.data();
    } else {
        Staged dz, dt, dx, dlen, di, dd, dn, dic, dsr, dst;
        if ((rc = dz.put(zs, cells * 8)) != PVX_OK || (rc = dt.put(t, cells * 8)) != PVX_OK || (rc = dx.put(x, cells * 8)) != PVX_OK ||
            (rc = dlen.put(len, (size_t)rows * 4)) != PVX_OK || (rc = zs ? di.room(slots * 4) : di.put(idx, slots * 4)) != PVX_OK ||
            (rc = dd.room(slots * 4)) != PVX_OK || (rc = zs ? dn.room((size_t)rows * 4) : dn.put(njump, (size_t)rows * 4)) != PVX_OK || (rc = dic.room(slots * 16)) != PVX_OK || (rc = dsr.room(slots * 16)) != PVX_OK ||
            (rc = dst.room(slots * 4)) != PVX_OK) return rc;
        if ((rc = pvx_jump_pick_run(zs ? dz.mem.as<double>() : nullptr, dt.mem.as<double>(), dx.mem.as<double>(), len ? dlen.mem.as<int>() : nullptr, rows, nmax, thr, nsl,
                                    maxjump, di.mem.as<int>(), dd.mem.as<int>(), dn.mem.as<int>(), dic.mem.as<double>(), dsr.mem.as<double>(),
                                    dst.mem.as<int>(), s, &t_jumps_kernels)) != PVX_OK) return rc;
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

// ---- result wire format for the multi-GPU gather (k_wire.hip) -------------------------------
extern "C" int pvx_plan_set_wire_format(pvx_plan* plan, int format) {
    if (!plan) { pvx_set_error("null plan"); return PVX_ERR_INVALID; }
    if (format != 1 && format != 2) { pvx_set_error("unknown wire format %d", format); return PVX_ERR_INVALID; }
    if (format == 2 && plan->precision != 32) {
        pvx_set_error("wire format 2 (14 bytes per slot) carries the float32 value a precision-32 analysis computes a frequency from; this plan is at precision %d", plan->precision);
        return PVX_ERR_UNSUPPORTED;
    }
    plan->wire_fmt = format;
    return PVX_OK;
}
extern "C" int pvx_plan_get_wire_format(const pvx_plan* plan) {
    if (!plan) { pvx_set_error("null plan"); return PVX_ERR_INVALID; }
    return plan->wire_fmt;
}

extern "C" int64_t pvx_wire_bytes(const pvx_plan* plan, int64_t rows) {
    if (!plan || rows < 0) { pvx_set_error("bad wire argument"); return PVX_ERR_INVALID; }
    if (plan->nfft / 2 > 65536) { pvx_set_error("wire format holds bin numbers in 16 bits (nfft <= 131072)"); return PVX_ERR_UNSUPPORTED; }
    return (int64_t)pvx_wire_block_bytes(rows, plan->npks, plan->precision, plan->wire_fmt);
}

extern "C" int pvx_pack_rows_dev(const pvx_plan* plan, int64_t rows, const double* d_f, const double* d_mag,
                                 const double* d_ph, const double* d_binno, const double* d_totalmag, void* d_wire,
                                 void* stream) {
    int rc = pvx_require_plan_device(plan);
    if (rc != PVX_OK) return rc;
    if (pvx_wire_bytes(plan, rows) < 0) return PVX_ERR_INVALID;
    if (rows == 0) return PVX_OK;
    if (!d_f || !d_mag || !d_ph || !d_binno || !d_totalmag || !d_wire) { pvx_set_error("null wire array"); return PVX_ERR_INVALID; }
    WireParams wp = {};
    wp.rows = rows; wp.K = plan->npks; wp.precision = plan->precision; wp.fstep = plan->fstep; wp.wire = d_wire;
    wp.fmt = plan->wire_fmt; wp.dt = plan->dt; wp.wfbin = plan->d_wfbin.as<double>();
    wp.f = d_f; wp.mag = d_mag; wp.ph = d_ph; wp.binno = d_binno; wp.totalmag = d_totalmag;
    return pvx_launch_wire(wp, true, (hipStream_t)stream);
}

// run_pv straight into the wire format: what a rank of a multi-GPU job hands to the gather.  k_fused_rev (precision 32, nfft 512 ..
// 2048) writes the block itself; every other plan analyses into a plan-owned result block and packs it.
extern "C" int64_t pvx_analyze_dev_wire(pvx_plan* p, const void* d_x, int x_dtype, int64_t nsamp, int64_t nsig, int64_t sig_stride,
                                        void* d_wire, void* stream) {
    int rc = pvx_require_plan_device(p);
    if (rc != PVX_OK) return rc;
    rc = check_analyze_args(p, d_x, x_dtype, nsamp, nsig, sig_stride, nullptr);
    if (rc != PVX_OK) return rc;
    const int64_t F = pvx_nframes(nsamp, p->nfft, p->hop);
    if (F == 0) return 0;
    if (!d_wire) { pvx_set_error("null wire block"); return PVX_ERR_INVALID; }
    if (pvx_wire_bytes(p, nsig * F) < 0) return PVX_ERR_INVALID;
    const int64_t rows = nsig * F;
    const size_t n = (size_t)rows * (size_t)p->npks, ts = p->precision == 64 ? 8 : 4;
    auto al8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
    unsigned char* w = (unsigned char*)d_wire;
    const Route route = route_for(p, x_dtype, nsig * (F + 1));
    if (route == Route::fused_rev && getenv("PVX_NO_WIRE_OUT") == nullptr) {
        // the sections of the block (k_wire.hip) as the kernel's output arrays
        const size_t fw = p->wire_fmt == 2 ? 4 : 8;                   // (format 2: the float32 the frequency is computed from)
        double* wf = (double*)w;
        double* wm = (double*)(w + al8(n * fw));
        double* wp = (double*)(w + al8(n * fw) + al8(n * ts));
        double* wb = (double*)(w + al8(n * fw) + 2 * al8(n * ts));
        double* wt = (double*)(w + al8(n * fw) + 2 * al8(n * ts) + al8(n * 2));
        rc = analyze_rows(p, route, d_x, x_dtype, nsamp, nsig, sig_stride, F, wf, wm, wp, nullptr, wb, nullptr, wt, nullptr, (hipStream_t)stream, {}, true);
        return rc == PVX_OK ? F : rc;
    }
    const size_t per_frame_out = (size_t)(5 * p->npks + 2) * sizeof(double);
    if ((rc = p->d_wiretmp.grow((size_t)rows * per_frame_out, Sizing::headroom)) != PVX_OK) return rc;
    const HostOut o = block_ptrs(p->d_wiretmp.as<double>(), rows, p->npks);
    rc = analyze_rows(p, route, d_x, x_dtype, nsamp, nsig, sig_stride, F, o.f, o.mag, o.ph, o.realph, o.binno, nullptr, o.totalmag, nullptr, (hipStream_t)stream);
    if (rc != PVX_OK) return rc;
    rc = pvx_pack_rows_dev(p, rows, o.f, o.mag, o.ph, o.binno, o.totalmag, d_wire, stream);
    return rc == PVX_OK ? F : rc;
}

extern "C" int pvx_unpack_rows_dev(const pvx_plan* plan, int64_t rows, const void* d_wire, double* d_f, double* d_mag,
                                   double* d_ph, double* d_realph, double* d_binno, double* d_totalmag, void* stream) {
    int rc = pvx_require_plan_device(plan);
    if (rc != PVX_OK) return rc;
    if (pvx_wire_bytes(plan, rows) < 0) return PVX_ERR_INVALID;
    if (rows == 0) return PVX_OK;
    if (!d_f || !d_mag || !d_ph || !d_realph || !d_binno || !d_totalmag || !d_wire) { pvx_set_error("null wire array"); return PVX_ERR_INVALID; }
    WireParams wp = {};
    wp.rows = rows; wp.K = plan->npks; wp.precision = plan->precision; wp.fstep = plan->fstep; wp.wire = (void*)d_wire;
    wp.fmt = plan->wire_fmt; wp.dt = plan->dt; wp.wfbin = plan->d_wfbin.as<double>();
    wp.of = d_f; wp.omag = d_mag; wp.oph = d_ph; wp.orealph = d_realph; wp.obinno = d_binno; wp.ototalmag = d_totalmag;
    return pvx_launch_wire(wp, false, (hipStream_t)stream);
}

// ---- resynthesis: SinSum.synth (PV.py:1053-1070) -------------------------------------------
extern "C" int64_t pvx_synth_len(int64_t max_end_frame, int nfft, int hop_analysis, int hop_synth, double edge) {
    if (nfft <= 0 || hop_analysis <= 0 || hop_synth <= 0 || max_end_frame < 0) return PVX_ERR_INVALID;
    const double dfr = (double)nfft / (double)hop_analysis / 2.;      // PV.py:1055
    const int64_t edgsamp = (int64_t)(edge * hop_synth * dfr);        // PV.py:1056, integer as under Python 2
    return (max_end_frame + 2) * (int64_t)hop_synth + 2 * edgsamp - edgsamp;   // len(w[edgsamp:]), PV.py:1059, 1070
}

extern "C" int pvx_synth_dev_flags(const double* d_f, const double* d_mag, const double* d_realph, const int32_t* d_partial_id,
                             int64_t F, int K, const int32_t* d_part_start, const int32_t* d_part_len, int64_t P,
                             double sr, int nfft, int hop_analysis, int hop_synth, double edge, int minframes,
                             double* d_w, int64_t wlen, void* stream, int flags) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    if (F <= 0 || K <= 0 || P <= 0 || nfft <= 0 || hop_analysis <= 0 || hop_synth <= 0 || !(sr > 0) || wlen <= 0 || !(edge >= 0)) {
        pvx_set_error("bad resynthesis argument");
        return PVX_ERR_INVALID;
    }
    if (!d_f || !d_mag || !d_realph || !d_partial_id || !d_part_start || !d_part_len || !d_w) { pvx_set_error("null resynthesis array"); return PVX_ERR_INVALID; }
    SynthParams sp;
    sp.f = d_f; sp.mag = d_mag; sp.realph = d_realph; sp.partial_id = d_partial_id;
    sp.part_start = d_part_start; sp.part_len = d_part_len; sp.F = F; sp.P = P; sp.K = K;
    sp.sr = sr; sp.edge = edge; sp.nfft = nfft; sp.hop_a = hop_analysis; sp.hop_s = hop_synth; sp.minframes = minframes;
    sp.w = d_w; sp.wlen = wlen; sp.no_phcor = (flags & PVX_SYNTH_NO_PHCOR) ? 1 : 0;
    sp.f32_samples = (flags & PVX_SYNTH_F32) ? 1 : 0;
    return pvx_launch_synth(sp, (hipStream_t)stream);
}

// one slice of the waveform's segments (internal: pvx_synth_resident overlaps the slices' kernels with their copies)
static int synth_slice(const double* d_f, const double* d_mag, const double* d_realph, const int32_t* d_partial_id, int64_t F, int K,
                       const int32_t* d_part_start, const int32_t* d_part_len, int64_t P, double sr, int nfft, int hop_analysis, int hop_synth,
                       double edge, int minframes, double* d_w, int64_t wlen, hipStream_t stream, int64_t seg0, int64_t seg_count, bool first,
                       void* ws, size_t ws_bytes, unsigned* ws_gen, int f32_samples) {
    SynthParams sp;
    sp.f32_samples = f32_samples;
    sp.skip_prepare = first ? 0 : 1;          // the partial-major copy of the analysis arrays is made with the first slice
    sp.ws = ws; sp.ws_bytes = ws_bytes; sp.ws_gen = ws_gen;
    sp.f = d_f; sp.mag = d_mag; sp.realph = d_realph; sp.partial_id = d_partial_id;
    sp.part_start = d_part_start; sp.part_len = d_part_len; sp.F = F; sp.P = P; sp.K = K;
    sp.sr = sr; sp.edge = edge; sp.nfft = nfft; sp.hop_a = hop_analysis; sp.hop_s = hop_synth; sp.minframes = minframes;
    sp.w = d_w; sp.wlen = wlen; sp.no_phcor = 0; sp.seg0 = seg0; sp.seg_count = seg_count;
    return pvx_launch_synth(sp, stream);
}

static int plan_synth_f32(const pvx_plan* p) {
    const int f32 = (p->precision == 32 && getenv("PVX_SYNTH_F64") == nullptr) ? 1 : 0;
    const_cast<pvx_plan*>(p)->last_synth = f32 ? "k_synth_bodies<f32>" : "k_synth_bodies<f64>";
    return f32;
}

extern "C" int pvx_synth_dev(const double* d_f, const double* d_mag, const double* d_realph, const int32_t* d_partial_id,
                             int64_t F, int K, const int32_t* d_part_start, const int32_t* d_part_len, int64_t P,
                             double sr, int nfft, int hop_analysis, int hop_synth, double edge, int minframes,
                             double* d_w, int64_t wlen, void* stream) {
    return pvx_synth_dev_flags(d_f, d_mag, d_realph, d_partial_id, F, K, d_part_start, d_part_len, P, sr, nfft, hop_analysis,
                               hop_synth, edge, minframes, d_w, wlen, stream, 0);
}

extern "C" int pvx_synth_flags(const double* f, const double* mag, const double* realph, const int32_t* partial_id, int64_t F,
                         int K, const int32_t* part_start, const int32_t* part_len, int64_t P, double sr, int nfft,
                         int hop_analysis, int hop_synth, double edge, int minframes, double* w, int64_t wlen, int flags) {
    int rc = pvx_require_device();
    if (rc != PVX_OK) return rc;
    if (F <= 0 || K <= 0 || P <= 0 || !f || !mag || !realph || !partial_id || !part_start || !part_len || !w) {
        pvx_set_error("bad resynthesis argument");
        return PVX_ERR_INVALID;
    }
    int64_t maxend = 0;                                               // max(self.end), PV.py:1059
    for (int64_t i = 0; i < P; i++) { const int64_t e = (int64_t)part_start[i] + part_len[i] - 1; if (e > maxend) maxend = e; }
    const int64_t need = pvx_synth_len(maxend, nfft, hop_analysis, hop_synth, edge);
    if (need < 0 || need != wlen) { pvx_set_error("output length %lld, expected %lld", (long long)wlen, (long long)need); return PVX_ERR_SIZE; }
    const size_t n = (size_t)F * K;
    DevMem df, dm, dr, dpid, dst, dln, dw;
    if ((rc = df.alloc(n * 8)) != PVX_OK || (rc = dm.alloc(n * 8)) != PVX_OK || (rc = dr.alloc(n * 8)) != PVX_OK ||
        (rc = dpid.alloc(n * 4)) != PVX_OK || (rc = dst.alloc((size_t)P * 4)) != PVX_OK ||
        (rc = dln.alloc((size_t)P * 4)) != PVX_OK || (rc = dw.alloc((size_t)wlen * 8)) != PVX_OK)
        return rc;
    if ((rc = host_to_device(df.get(), f, n * 8)) != PVX_OK || (rc = host_to_device(dm.get(), mag, n * 8)) != PVX_OK || (rc = host_to_device(dr.get(), realph, n * 8)) != PVX_OK ||
        (rc = host_to_device(dpid.get(), partial_id, n * 4)) != PVX_OK || (rc = host_to_device(dst.get(), part_start, (size_t)P * 4)) != PVX_OK ||
        (rc = host_to_device(dln.get(), part_len, (size_t)P * 4)) != PVX_OK) return rc;
    rc = pvx_synth_dev_flags(df.as<const double>(), dm.as<const double>(), dr.as<const double>(), dpid.as<const int32_t>(), F, K,
                             dst.as<const int32_t>(), dln.as<const int32_t>(), P, sr, nfft, hop_analysis, hop_synth, edge, minframes,
                             dw.as<double>(), wlen, nullptr, flags);
    if (rc != PVX_OK) return rc;
    PVX_HIP_CHECK(hipStreamSynchronize(nullptr));
    if ((rc = device_to_host(w, dw.get(), (size_t)wlen * 8)) != PVX_OK) return rc;
    return PVX_OK;
}

extern "C" int pvx_synth(const double* f, const double* mag, const double* realph, const int32_t* partial_id, int64_t F,
                         int K, const int32_t* part_start, const int32_t* part_len, int64_t P, double sr, int nfft,
                         int hop_analysis, int hop_synth, double edge, int minframes, double* w, int64_t wlen) {
    return pvx_synth_flags(f, mag, realph, partial_id, F, K, part_start, part_len, P, sr, nfft, hop_analysis, hop_synth, edge,
                           minframes, w, wlen, 0);
}

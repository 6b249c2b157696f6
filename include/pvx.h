/*
 * pvx.h -- C ABI of libpvx_hip.so, the MI355X (gfx950) implementation of the PyPeVoc
 * phase-vocoder hot path:  PV.run_pv() -> PV.toSinSum() -> SinSum.synth().
 *
 * The reference (goiosunsw/PyPeVoc, pure Python) has no FFI of its own; the boundary is its
 * Python class API.  Each entry point below replaces the body of the reference method cited
 * beside it (PV.py = pypevoc/PVAnalysis.py, PF.py = pypevoc/PeakFinder.py) and is what a
 * ctypes binding inside those methods would call -- see INTEGRATION.md for the stub.
 *
 * Conventions
 *   - plain C types only; every buffer is caller-allocated and caller-owned;
 *   - "host" entry points take host pointers, copy in/out and return after the device has
 *     finished; "_dev" entry points take device pointers (HBM-resident data) and a
 *     hipStream_t passed as void*, and only enqueue work on that stream;
 *   - return value 0 (or a non-negative count) on success, a negative pvx_status on error;
 *     pvx_last_error() returns a thread-local message for the last failure;
 *   - there is NO CPU fallback: without a usable HIP device every call fails with
 *     PVX_ERR_NO_DEVICE.
 *   - array layouts are the reference's: (F, K) float64 C-order, zero padded, valid peaks
 *     left-packed in ascending-bin order (PV.py:226-245, 256-264).
 */
#ifndef PVX_H
#define PVX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PVX_VERSION 100

typedef enum {
    PVX_OK = 0,
    PVX_ERR_NO_DEVICE = -1,   /* no HIP device / runtime failure at init */
    PVX_ERR_INVALID = -2,     /* bad argument */
    PVX_ERR_HIP = -3,         /* a HIP or rocFFT call failed */
    PVX_ERR_ALLOC = -4,       /* device or host allocation failed */
    PVX_ERR_UNSUPPORTED = -5, /* valid request outside what the kernels handle */
    PVX_ERR_SIZE = -6,        /* caller buffer too small / wrong length */
    PVX_ERR_SINGULAR = -7,    /* a frame's Toeplitz system has a zero prediction error (pvx_lpc, pvx_iaif) */
    PVX_ERR_NOCONV = -8       /* a polynomial's root iteration met its bound of iterations (pvx_polyroots, pvx_formants) */
} pvx_status;

/* sample types accepted for the input signal x (PV.py:84 copies whatever the caller passed) */
typedef enum { PVX_F32 = 0, PVX_F64 = 1, PVX_I16 = 2 } pvx_dtype;

/* Every function declared below is an exported entry point of libpvx_hip.so, and nothing else is: the library is built with
 * -fvisibility=hidden, these declarations carry default visibility (tests/test_abi_cpu.py checks both directions). */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* ---- library ------------------------------------------------------------------------- */

/* Select and initialise the HIP device (idempotent per device).  device < 0: current device. */
int pvx_init(int device);
const char* pvx_last_error(void);
int pvx_version(void);
/* Fingerprint of the kernel sources the library was built from: the first 16 hex digits of the sha256 over
 * the .hip and .h files of pypevoc_amd/csrc in name order (pypevoc_amd/_lib.py refuses a library that does not match its sources;
 * bench.py quotes committed profiles only when they carry the same fingerprint). */
const char* pvx_build_fingerprint(void);
/* Name of the device the library is bound to ("" before pvx_init). */
const char* pvx_device_name(void);
/* HIP device index the library is bound to (-1 before pvx_init) */
int pvx_device(void);

/* Number of frames run_pv produces: pos = 0, hop, ... while pos < nsamp - nfft (PV.py:223-249). */
int64_t pvx_nframes(int64_t nsamp, int nfft, int hop);

/* ---- analysis: PV.__init__ constants + PV.run_pv (PV.py:72-131, 150-264) ------------- */

typedef struct pvx_plan pvx_plan; /* opaque: constants, window, rocFFT plan, device workspace */

/*
 * Create an analysis plan.  Replaces the constant set-up of PV.__init__ (PV.py:97-121) and owns
 * everything calc_fft_frame/calc_pv_frame need on the device.
 *   win        nfft window samples = wind(nfft) (PV.py:97); NULL = symmetric Hann (np.hanning)
 *   precision  32: float32 frames/spectra (per-peak arithmetic and outputs stay float64)
 *              64: float64 end to end
 *   max_rows   upper bound on frames processed per internal launch (0 = default); bounds the
 *              device workspace: about max_rows * nfft * 3 * sizeof(real) bytes
 */
int pvx_plan_create(pvx_plan** plan, double sr, int nfft, int hop, int npks, double pkthresh,
                    const double* win, int precision, int64_t max_rows);
int pvx_plan_destroy(pvx_plan* plan);
/* bytes of device workspace the plan holds */
int64_t pvx_plan_workspace_bytes(const pvx_plan* plan);
/*
 * FFT mode of the analysis stage:
 *   0  framing kernel -> rocFFT batched real FFT -> phase/peak kernel (any nfft, both precisions)
 *   1  fused kernel: window, in-register/LDS FFT and peak stage in one wave per frame, no
 *      intermediate arrays in HBM (nfft in {512, 1024, 2048}, precision = 32)
 *   2  (a witness kernel since round 6) fused kernel with several waves per frame (nfft in {2048, 4096, 8192}, precision = 32)
 *   3  mode 1's arithmetic (bit-identical results) with a workgroup of 8 (nfft 2048) or 12 (nfft 512, 1024)
 *      waves walking as many consecutive frames over a shared ring of spectra in LDS: two / three waves per
 *      SIMD (precision = 32; npks <= 120 at nfft 2048: the staging has to fit the LDS next to the ring)
 *   4  mode 1's arithmetic again (bit-identical results) with every wave on its own: a wave walks a contiguous range
 *      of rows DOWNWARDS over one spectrum buffer, the previous spectrum a frame's peaks need arrives one row later;
 *      sliding sample window at hop = nfft/4, nfft/2 (precision = 32, nfft in {512, 1024, 2048})
 *   5  teams of mode 4's waves, 2 / 4 per frame (precision = 32, nfft in {4096, 8192}, npks <= 128); a call of 0x7fffff00
 *      rows or more runs mode 0's path (the plan stays in mode 5)
 * Mode 0 itself runs as one launch for nfft in {512, 1024, 2048} (window + FFT + peaks: k_pv_rev at float64 with npks <= 64,
 * no spectrum workspace; k_stft_pv otherwise), as fused STFT + phase/peak kernel for nfft 4096 / 8192, and through rocFFT otherwise.
 * A new plan uses 4 where it is supported, else 5, else 0 (environment PVX_FFT_MODE overrides; the witness library tries 3 and 1
 * before 5); 1, 2 and 3 are witness kernels of the tests: the product library answers PVX_ERR_UNSUPPORTED for them
 * (tests/libpvx_witness.so carries them).
 */
int pvx_plan_set_fft_mode(pvx_plan* plan, int mode);
int pvx_plan_get_fft_mode(const pvx_plan* plan);
/* The HIP device that was current when the plan was created: its buffers, streams and events live there.  Every entry point
 * that takes a plan fails with PVX_ERR_INVALID when the calling thread is bound to another device (pvx_init(d), or a
 * pvx_batch worker's device) instead of running kernels on buffers of the wrong device. */
int pvx_plan_device(const pvx_plan* plan);
/* Which kernels the plan's last calls ran, as "analysis=<kernel>;synth=<kernel>" (a part is missing until its call has run):
 * k_fused_rev | k_fused_team | k_pv_rev | k_stft_pv | k_stft+k_phase_peaks | k_frames+rocfft+k_phase_peaks (the witness library
 * also k_fused | k_fused_mw | k_fused_ring | k_pv_team) for the analysis, k_synth_bodies<f64> | k_synth_bodies<f32> for the
 * resynthesis.  k_fused_rev<kc8>: the instantiation of k_fused_rev that has the plan's npks (8) as a compile-time constant;
 * plain k_fused_rev is the kernel for any npks (every other plan, or PVX_REV_NO_SPEC=1 in the environment).  For tests and
 * benchmarks that must know what they measured; the string lives in the plan and is valid until its next call. */
const char* pvx_plan_last_kernels(const pvx_plan* plan);
/*
 * Progress reporting: replaces Progress.update (pypevoc/ProgressDisplay.py:82-88), which the
 * reference calls once per frame (PV.py:250-254, 528).  The HOST entry points pvx_analyze and
 * pvx_harmonic_analyze call fn(frames_done, frames_total, user) after every launch chunk has
 * completed on the device and once when all results are back (done == total).  fn = NULL disables.
 * The asynchronous *_dev variants never call it.
 */
typedef void (*pvx_progress_fn)(int64_t frames_done, int64_t frames_total, void* user);
int pvx_plan_set_progress(pvx_plan* plan, pvx_progress_fn fn, void* user);

/*
 * Stage timing for bench.py's roofline line.  While enabled, hipEvents recorded on the launch
 * stream bracket every stage of every chunk (of pvx_harmonic_analyze: its transform).  pvx_plan_get_timing synchronises with
 * those events and returns, accumulated since the last call: ms[0] framing kernel (or k_stft), ms[1] rocFFT, ms[2]
 * phase/peak kernel, ms[3] fused kernel (fft modes 1-5, and mode 0's one-launch form); launches[i] = stage launches counted.
 */
int pvx_plan_set_timing(pvx_plan* plan, int enable);
int pvx_plan_get_timing(pvx_plan* plan, double* ms /*[4]*/, int64_t* launches /*[4]*/);

/*
 * run_pv on `nsig` equal-length signals resident in HBM (nsig = 1: the reference's single
 * signal).  Signal b starts at x + b * sig_stride samples and has nsamp samples.
 *   d_f, d_mag, d_ph, d_realph, d_binno : device float64 [nsig, F, npks]
 *   d_t, d_totalmag                     : device float64 [nsig, F]       (either may be NULL)
 *   d_prev0 : optional device float64 [nfft/2][2] (re, im) -- the spectrum `oldfft` holds before
 *             the first frame (PV.py:121, 209); NULL = zeros.  Used by the streaming
 *             calc_pv_frame mirror; only valid with nsig == 1.
 *   stream  : hipStream_t as void* (NULL = default stream).  Asynchronous.
 * Returns F (frames per signal) or a negative status.
 */
int64_t pvx_analyze_dev(pvx_plan* plan, const void* d_x, int x_dtype, int64_t nsamp,
                        int64_t nsig, int64_t sig_stride,
                        double* d_f, double* d_mag, double* d_ph, double* d_realph, double* d_binno,
                        double* d_t, double* d_totalmag, const double* d_prev0, void* stream);

/* Same with host buffers (copies x in, results out, synchronous).  prev0 may be NULL.
 * If last_spec is not NULL it receives the half spectrum of the last frame, float64 [nfft/2][2]
 * (the value PV.oldfft holds after run_pv, PV.py:209). */
int64_t pvx_analyze(pvx_plan* plan, const void* x, int x_dtype, int64_t nsamp,
                    int64_t nsig, int64_t sig_stride,
                    double* f, double* mag, double* ph, double* realph, double* binno,
                    double* t, double* totalmag, const double* prev0, double* last_spec);

/*
 * The host entry points keep their device buffers in the plan (grow-only; no hipMalloc per call), take the
 * input in chunks that fit PVX_MAX_DEVICE_BYTES (environment; default 2 GiB per buffer), double-buffered --
 * the copy of chunk i+1 and the results of chunk i-1 move while the kernels of chunk i run -- and carry the
 * last spectrum from chunk to chunk on the device (PV.py:209), so a signal larger than HBM runs and the
 * result does not depend on the chunking (bit for bit).  Calls of a few MB go through pinned staging and
 * synchronise once.
 *
 * Resident results: pvx_analyze_resident is pvx_analyze without the copy back -- the reference's arrays
 * stay in the plan, in HBM, in the layout of pvx_analyze_dev.  What follows in the reference's pipeline then
 * runs where the data is, on the plan's stream, and only what the caller asks for crosses PCIe:
 *   pvx_resident_fetch(plan, which, host)   one array; which = PVX_RES_F .. PVX_RES_TOTALMAG
 *   pvx_resident_ptr(plan, which)           its device address (valid until the plan's next analysis)
 *   pvx_track_resident                      PV.toSinSum (PV.py:299-322): returns the number of partials, the
 *                                           table stays resident; *max_end_frame = max(SinSum.end)
 *   pvx_resident_fetch_table                partial_id int32 [F, K], part_start / part_len int32 [P] (any may be NULL)
 *   pvx_synth_resident                      SinSum.synth (PV.py:1053-1070) from the resident arrays and table;
 *                                           w: host float64 [wlen = pvx_synth_len(max_end_frame, ...)]
 *   pvx_f0_resident                         PV.calc_f0 (PV.py:371-391): fm float64 [F], idx int32 [F]
 *   pvx_harmonic_power_resident             PV.calc_harmonic_power (PV.py:266-297, including the row indexing
 *                                           of :278; PVX_ERR_SIZE where the reference raises IndexError):
 *                                           hpower, nharmonics float64 [F, K]
 */
#define PVX_RES_F 0
#define PVX_RES_MAG 1
#define PVX_RES_PH 2
#define PVX_RES_REALPH 3
#define PVX_RES_BINNO 4
#define PVX_RES_T 5
#define PVX_RES_TOTALMAG 6
int64_t pvx_analyze_resident(pvx_plan* plan, const void* x, int x_dtype, int64_t nsamp, int64_t nsig,
                             int64_t sig_stride, const double* prev0, double* last_spec);
int pvx_resident_fetch(pvx_plan* plan, int which, double* host);
const double* pvx_resident_ptr(pvx_plan* plan, int which);
int64_t pvx_track_resident(pvx_plan* plan, double maxpitchjmp, int64_t* max_end_frame);
int pvx_resident_fetch_table(pvx_plan* plan, int32_t* partial_id, int32_t* part_start, int32_t* part_len);
int pvx_synth_resident(pvx_plan* plan, double sr, int hop_synth, double edge, int minframes, double* w, int64_t wlen);
/*
 * run_pv on many independent signals of any lengths, from host buffers, over one or more GPUs of THIS process -- the C-level
 * batch / multi-GPU entry (SURVEY.md 8(b) `pvx_analyze_batch`; the reference's equivalent is a Python loop over PV objects,
 * PV.py:213-264).  The path shards by signal and has no exchange step: the devices never talk to each
 * other, each worker (workers_per_device host threads per device, 0 = 4, each with its own plan and stream so one signal's
 * transfers run under another's kernels) takes the next signal off one queue, longest first, and its results go straight
 * into the caller's arrays.  Every signal's arrays are bit-identical to pvx_analyze of that signal alone.
 *   devices / ndev : the HIP devices to use (an entry may repeat); ndev = 0: the device of pvx_init
 *   items[i]       : x / nsamp in; f .. binno float64 [F, npks] and t, totalmag float64 [F] (either may be NULL) out, caller-
 *                    allocated with F = pvx_nframes(nsamp, nfft, hop); nframes = F or that signal's negative status;
 *                    device = the device that analysed it
 * pvx_batch_run returns the frames analysed (sum of F) or the first negative status (pvx_last_error names the signal); it
 * may be called again and again on one pvx_batch -- the plans and their buffers are kept -- but not concurrently.
 * pvx_analyze_batch = create + run + destroy.
 */
typedef struct pvx_batch pvx_batch;
typedef struct pvx_batch_item {
    const void* x;
    int64_t nsamp;
    double *f, *mag, *ph, *realph, *binno;
    double *t, *totalmag;
    int64_t nframes;
    int32_t device;
    int32_t reserved;
} pvx_batch_item;
int pvx_batch_create(pvx_batch** batch, double sr, int nfft, int hop, int npks, double pkthresh, const double* win /*nfft or NULL = hanning*/,
                     int precision, const int* devices, int ndev, int workers_per_device);
int64_t pvx_batch_run(pvx_batch* batch, int x_dtype, pvx_batch_item* items, int64_t nitems);
int pvx_batch_destroy(pvx_batch* batch);
int64_t pvx_analyze_batch(double sr, int nfft, int hop, int npks, double pkthresh, const double* win, int precision, int x_dtype,
                          pvx_batch_item* items, int64_t nitems, const int* devices, int ndev);

/* Page-locked host memory for result arrays.  pvx_synth_resident recognises such a destination: the waveform
 * (SinSum.synth's return value, PV.py:1070) is written straight into it by the DMA engine (with PVX_SYNTH_ZEROCOPY=1, up
 * to 4 MB, by the kernels' own stores); any other pointer goes through
 * the plan's pinned staging block and one more host copy.  NULL (and pvx_last_error) on failure. */
void* pvx_host_alloc(size_t bytes);
void pvx_host_free(void* p);
int pvx_f0_resident(pvx_plan* plan, double fmin, double fmax, double thr, double* fm, int32_t* idx);
int pvx_harmonic_power_resident(pvx_plan* plan, double f_threshold, double* hpower, double* nharmonics);

/* calc_fft_frame (PV.py:150-158): windowed, 1/wfact-normalised spectra of `nfr` frames starting
 * at sample positions pos[0..nfr); spec: host float64 [nfr][nfft/2+1][2] (bins 0..nfft/2; the
 * remaining bins of the reference's length-nfft result are the conjugate mirror). */
int pvx_stft_frames(pvx_plan* plan, const void* x, int x_dtype, int64_t nsamp,
                    const int64_t* pos, int64_t nfr, double* spec);

/* ---- PeakFinder (PF.py:35-74, 155-194, 113-136) -------------------------------------- */

/*
 * PeakFinder(y, npeaks=, minrattomax=, minval=) followed by filter_by_salience(rad) on `nrows`
 * independent rows y[r][0..n) (host float64).
 *   npeaks    <= 0: "not npeaks" -> n (PF.py:64-67)
 *   thr_kind  0: no threshold given (minamp = min(y)); 1: minrattomax = thr_val; 2: minval = thr_val
 *   rad       salience radius; < 0 skips filter_by_salience
 *   pos       int32 [nrows][cap]: findpos() positions, ascending (PF.py:189)
 *   keep      int8  [nrows][cap]: _keep after filter_by_salience
 *   count     int32 [nrows]
 *   cap       row capacity of pos/keep (>= min(npeaks, n) to hold everything)
 */
int pvx_peakfinder(const double* y, int64_t nrows, int n, int npeaks, int thr_kind, double thr_val,
                   int rad, int32_t* pos, int8_t* keep, int32_t* count, int cap);

/* ---- tracker: PV.toSinSum / SinSum.add_frame (PV.py:299-322, 871-957) ---------------- */

/*
 * Builds the partial table from the analysis arrays of one signal.
 *   f, mag            host float64 [F, K]
 *   maxpitchjmp       semitone threshold (the reference always uses 0.5: PV.py:320-321)
 *   partial_id        int32 [F, K]: partial index of every peak slot, -1 if the slot is empty
 *   part_start/len    int32 [cap]: first frame and number of points of each partial, in the
 *                     reference's creation order (PV.py:819-830)
 *   cap               capacity of part_start/part_len (F*K always suffices)
 * Returns the number of partials or a negative status.
 */
int64_t pvx_track(const double* f, const double* mag, int64_t F, int K, double maxpitchjmp,
                  int32_t* partial_id, int32_t* part_start, int32_t* part_len, int64_t cap);
int64_t pvx_track_dev(const double* d_f, const double* d_mag, int64_t F, int K, double maxpitchjmp,
                      int32_t* d_partial_id, int32_t* d_part_start, int32_t* d_part_len, int64_t cap,
                      void* stream);

/* ---- resynthesis: SinSum.synth / RegPartial.synth (PV.py:1053-1070, 684-756) ---------- */

/* Output length of SinSum.synth: (max(end)+2)*hop_synth + int(edge*hop_synth*nfft/hop_analysis/2). */
int64_t pvx_synth_len(int64_t max_end_frame, int nfft, int hop_analysis, int hop_synth, double edge);

/*
 * SinSum.synth(sr, hop_synth, edge, minframes, phase_preserve=True).
 *   f, mag, realph    host float64 [F, K] analysis arrays
 *   partial_id        int32 [F, K] from pvx_track;  part_start/part_len: int32 [P]
 *   w                 host float64 [wlen], wlen = pvx_synth_len(max(end), ...)
 */
int pvx_synth(const double* f, const double* mag, const double* realph, const int32_t* partial_id,
              int64_t F, int K, const int32_t* part_start, const int32_t* part_len, int64_t P,
              double sr, int nfft, int hop_analysis, int hop_synth, double edge, int minframes,
              double* w, int64_t wlen);
int pvx_synth_dev(const double* d_f, const double* d_mag, const double* d_realph,
                  const int32_t* d_partial_id, int64_t F, int K,
                  const int32_t* d_part_start, const int32_t* d_part_len, int64_t P,
                  double sr, int nfft, int hop_analysis, int hop_synth, double edge, int minframes,
                  double* d_w, int64_t wlen, void* stream);
/*
 * The same with flags.  PVX_SYNTH_NO_PHCOR: RegPartial.synth of a partial built with fstep=None
 * (PV.py:710-713): no frequency-slope phase correction (phcor = phcornext = 0); nfft / hop_analysis then
 * only carry the overlap (hop_analysis / nfft).
 */
#define PVX_SYNTH_NO_PHCOR 1
/* PVX_SYNTH_F32: the sample loop of the partials' bodies in float32 (what pvx_synth_resident does for a plan at precision 32):
 * the seeds of every run of 32 samples still come from the float64 closed form; waveform within 1e-4 max|w| of the float64 one
 * (measured: see DESIGN.md), at about half the time. */
#define PVX_SYNTH_F32 2
int pvx_synth_flags(const double* f, const double* mag, const double* realph, const int32_t* partial_id,
                    int64_t F, int K, const int32_t* part_start, const int32_t* part_len, int64_t P,
                    double sr, int nfft, int hop_analysis, int hop_synth, double edge, int minframes,
                    double* w, int64_t wlen, int flags);
int pvx_synth_dev_flags(const double* d_f, const double* d_mag, const double* d_realph,
                        const int32_t* d_partial_id, int64_t F, int K,
                        const int32_t* d_part_start, const int32_t* d_part_len, int64_t P,
                        double sr, int nfft, int hop_analysis, int hop_synth, double edge, int minframes,
                        double* d_w, int64_t wlen, void* stream, int flags);

/* ---- PVHarmonic.run_pv / calc_pv_frame (PV.py:419-535) --------------------------------------
 *
 * Phase vocoder sampled at the multiples of a caller-supplied fundamental instead of PeakFinder
 * peaks.  Single signal.  Uses the plan's general path (window -> rocFFT -> k_harmonic_rows), any
 * nfft, precision 32 or 64.
 *   f0, nf0        HOST float64 [nf0 >= F]: fundamental of every frame (PV.py:507 indexes it by frame
 *                  number; a shorter array is the reference's IndexError -> PVX_ERR_SIZE).  Frames
 *                  with f0 <= 0 or NaN are skipped: zero rows, residual NaN, and they do NOT become
 *                  the "previous spectrum" of later frames (PV.py:509, 491).
 *   fmin           PVHarmonic.fmin (30.0 in the reference, PV.py:421)
 *   f, mag, ph     float64 [F, npks]: first npks harmonics (frequency may be NaN where the reference's
 *                  is: x/0 with a zero component); residual, t: float64 [F]
 *   prev0          optional [nfft/2][2] spectrum preceding the first analysed frame; last_spec
 *                  (host variant) receives PVHarmonic.oldfft after the loop.
 * A valid f0 below half a bin is rejected (PVX_ERR_INVALID).  Returns F or a negative status.
 */
int64_t pvx_harmonic_analyze(pvx_plan* plan, const void* x, int x_dtype, int64_t nsamp,
                             const double* f0, int64_t nf0, double fmin,
                             double* f, double* mag, double* ph, double* residual, double* t,
                             const double* prev0, double* last_spec);
int64_t pvx_harmonic_analyze_dev(pvx_plan* plan, const void* d_x, int x_dtype, int64_t nsamp,
                                 const double* f0, int64_t nf0, double fmin,
                                 double* d_f, double* d_mag, double* d_ph, double* d_residual,
                                 double* d_t, const double* d_prev0, void* stream);

/* ---- windowed reductions with the analysis framing ---------------------
 *
 * Frames start at i*hop for i*hop < n - wlen: pvx_nframes(n, wlen, hop) of them.  float64.
 *
 * pvx_heterodyne: Heterodyne.heterodyne(x, hetsig, wind, hop) (pypevoc/Heterodyne.py:35-60):
 *   out[i] = 2 * sum_j x[i*hop+j] * hetsig[i*hop+j] * wind[j] / sum(wind)   complex, [nfr][2]
 *   icent[i] = i*hop + wlen/2 (optional).  hetsig: complex128 [n] as [n][2].
 *   (SoundUtils.Heterodyn / HeterodynWithF0Track, SoundUtils.py:106-138, are this with
 *    hetsig = exp(+-2j*pi*phase) built by the caller and wind = windfunc(nwind).)
 * pvx_rms_frames: SoundUtils.RMSWind (SoundUtils.py:71-103):
 *   out[i] = sqrt(sum_j (x[i*hop+j]*wind[j])**2 / sum(wind**2))
 * `wind` is a HOST array in both variants.  Return nfr or a negative status.
 */
int64_t pvx_heterodyne(const double* x, const double* hetsig, int64_t n, const double* wind,
                       int wlen, int hop, double* out, int64_t* icent);
int64_t pvx_heterodyne_dev(const double* d_x, const double* d_hetsig, int64_t n, const double* wind,
                           int wlen, int hop, double* d_out, int64_t* d_icent, void* stream);
int64_t pvx_rms_frames(const double* x, int64_t n, const double* wind, int wlen, int hop, double* out);
int64_t pvx_rms_frames_dev(const double* d_x, int64_t n, const double* wind, int wlen, int hop,
                           double* d_out, void* stream);

/* pvx_funcwind: SoundUtils.FuncWind(func, x, sr, nwind, nhop, power, windfunc) (pypevoc/SoundUtils.py:42-69)
 * for the named reducers: out[i] = func(x[i*hop : i*hop+wlen] * wind) / divisor, with
 * divisor = sum(wind**power) for power > 0, else 1 (SoundUtils.py:55-58; computed by the caller).
 * x_complex != 0: x is complex128 [n] given as [n][2] (Heterodyn passes x * sinsig, :112): SUM and MEAN then
 * write complex results [nfr][2], STD / VAR real ones (numpy: mean(abs(xw - mean(xw))**2)); MAX / MIN of
 * complex frames -> PVX_ERR_UNSUPPORTED.  An arbitrary Python callable has no device form: the Python mirror
 * raises TypeError for anything but these six.  Returns nfr or a negative status. */
typedef enum { PVX_FW_SUM = 0, PVX_FW_MEAN = 1, PVX_FW_MAX = 2, PVX_FW_MIN = 3, PVX_FW_STD = 4, PVX_FW_VAR = 5 } pvx_funcwind_op;
int64_t pvx_funcwind(const double* x, int x_complex, int64_t n, const double* wind, int wlen, int hop,
                     int func, double divisor, double* out);
int64_t pvx_funcwind_dev(const double* d_x, int x_complex, int64_t n, const double* wind, int wlen, int hop,
                         int func, double divisor, double* d_out, void* stream);

/* ---- HeterodyneHarmonic: every harmonic of one f0 track (pypevoc/Heterodyne.py:261-542) -----
 *
 * fvec: the track in cycles per sample (f0 / sr), one value per sample of x.  The heterodyning signal of harmonic h is
 * exp(+2j*pi*h*cumsum(fvec)) (heterodyner_signal, :384-400); it is never materialised: the kernels keep the running sum
 * in cycles and evaluate its harmonics on the spot.  float64, the framing of pvx_heterodyne.
 *
 * pvx_hetharm: extract_partial / extract_partials / calc_adjusted_freq's heterodyne (:460-471, :521-532, :425):
 *   ah[i][k] = 2 * sum_j x[i*hop+j] * exp(+2j*pi*(first+k)*c[i*hop+j]) * wind[j] / sum(wind),  c = cumsum(fvec),
 *   complex [nfr][count][2]; halve_dc != 0 halves the column of harmonic 0 (:530).  icent[i] = i*hop + wlen/2 (optional).
 *   A column does not depend on which other harmonics the call asks for (bit for bit).  Returns nfr.
 * pvx_hetharm_resynth: resynth_partial / resynth / filter_harmonic (:473-499, :534-538) from ah [nfr][nharm_total][2]
 *   (nfr must be pvx_nframes(n, wlen, hop)):
 *   y[t] = sum_{h=first}^{first+count-1} Re(conj(exp(2j*pi*h*c[t])) * hf_h[t]),  hf_h = np.interp(t/sr, th, ah[:, h]),
 *   th[i] = (wlen/2 + i*hop)/sr, clamped to the end values.  filter != 0 zeroes hf_h[t] where f0 < fmin, f0 > fmax,
 *   f0*h > sr/2.2 or |hf_h[t]| < ampthr * max|hf_h| (f0 = fvec*sr).  hf (optional, count == 1): hf_first itself, [n][2].
 *   Returns n, or 0 without touching y when nfr == 0.
 * `wind` is a HOST array in both variants; every other array of the `_dev` forms is device memory, the work runs on
 * `stream` and is synchronised before the return.  Negative status on failure.
 */
int64_t pvx_hetharm(const double* x, int64_t n, const double* fvec, const double* wind, int wlen, int hop,
                    int first, int count, int halve_dc, double* ah, int64_t* icent);
int64_t pvx_hetharm_dev(const double* d_x, int64_t n, const double* d_fvec, const double* wind, int wlen, int hop,
                        int first, int count, int halve_dc, double* d_ah, int64_t* d_icent, void* stream);
int64_t pvx_hetharm_resynth(const double* fvec, int64_t n, const double* ah, int64_t nfr, int nharm_total, int wlen,
                            int hop, int first, int count, int filter, double sr, double fmin, double fmax,
                            double ampthr, double* y, double* hf);
int64_t pvx_hetharm_resynth_dev(const double* d_fvec, int64_t n, const double* d_ah, int64_t nfr, int nharm_total,
                                int wlen, int hop, int first, int count, int filter, double sr, double fmin,
                                double fmax, double ampthr, double* d_y, double* d_hf, void* stream);

/* ---- time-domain periodicity: PeriodSeries (pypevoc/Periodicity.py:251-503) ----------------
 *
 * pvx_periodicity: Periodicity._calc + sort_strength (Periodicity.py:98-236) for the frames centred at
 * idx[0..nidx) (host array; each frame x[idx - nwind/2 : idx + nwind - nwind/2] must lie inside x, else
 * PVX_ERR_INVALID).  method: PVX_PERIOD_XCORR / PVX_PERIOD_AMDF; cand_method: PVX_CAND_*; threshold is
 * PeakFinder's minval (0: min of the similarity slice), vthresh the voicing threshold.  Per frame i:
 * ncands[i] <= ncand candidates sorted by decreasing strength in cand_period / cand_strength[i*ncand ..]
 * (NaN beyond the count) and preferred[i] (-1 when there is none: the reference's `preferred = []`).
 * 1 <= ncand <= 64; nwind <= 32768, else PVX_ERR_UNSUPPORTED.  float64 throughout, no host compute.
 * pvx_periodicity_dev: x and the four outputs are device memory (idx and wind stay host arrays), work on
 * `stream`, synchronised before the return.  Both return nidx or a negative status.  Calls share a per-device
 * workspace kept for the process (grow-only buffers, one rocFFT plan per window length in use: memory does not grow
 * with the number or length of signals) and take turns on it.
 */
typedef enum { PVX_PERIOD_XCORR = 0, PVX_PERIOD_AMDF = 1 } pvx_period_method;
typedef enum { PVX_CAND_FFT = 0, PVX_CAND_MIN = 1, PVX_CAND_SIMILAR = 2, PVX_CAND_OTHER = 3 } pvx_cand_method;
int64_t pvx_periodicity(const double* x, int64_t nsamp, const double* wind, int nwind, const int64_t* idx,
                        int64_t nidx, int method, int cand_method, int mindelay, int maxdelay, double threshold,
                        double vthresh, int ncand, double fftthresh, double* cand_period,
                        double* cand_strength, int32_t* ncands, int32_t* preferred);
int64_t pvx_periodicity_dev(const double* d_x, int64_t nsamp, const double* wind, int nwind, const int64_t* idx,
                            int64_t nidx, int method, int cand_method, int mindelay, int maxdelay,
                            double threshold, double vthresh, int ncand, double fftthresh,
                            double* d_cand_period, double* d_cand_strength, int32_t* d_ncands,
                            int32_t* d_preferred, void* stream);

/* ---- YIN f0 tracking: SoundUtils.f0yin / aubio_f0yin (pypevoc/SoundUtils.py:234-261) --------
 *
 * The reference's entry calls the aubio package; this is the algorithm YIN.md specifies (de Cheveigne & Kawahara,
 * steps 1-5), not a bit-for-bit mirror of aubio.  For each frame xs = x[starts[i] : starts[i] + nwind] (starts: host
 * array, any order, repeats allowed; every frame must lie inside the nsamp samples, else PVX_ERR_INVALID), L = nwind / 2:
 *   d[t]  = sum_{j < L} (xs[j] - xs[j + t])^2, t = 1 .. hi + 1;  S[t] = d[1] + .. + d[t];  d'[t] = d[t] t / S[t]
 *           (the literal 1.0 where S[t] == 0; d'[0] = 1);
 *   pick  = the smallest t in [lo, hi] with d'[t] < tol and d'[t] < d'[t + 1]; without one (flag bit PVX_YIN_FALLBACK)
 *           the first arg-min of d' over [lo, hi];
 *   tau   = pick + 0.5 (s0 - s2) / (s0 - 2 s1 + s2) with s = d'[pick - 1 .. pick + 1] (pick where that denominator is 0),
 *   freq  = sr / tau, conf = 1 - d'[pick];
 *   a frame with S[hi + 1] == 0 (silent or constant) returns freq = conf = tau = 0, pick = 0 and flag = PVX_YIN_SILENT.
 * 2 <= lo <= hi <= L - 2 and nwind >= 8, else PVX_ERR_INVALID; nwind > PVX_YIN_MAX_NWIND: PVX_ERR_UNSUPPORTED and no
 * launch.  tau, flag and pick are nullable.  float64 throughout, every sum in an order fixed by (nwind, hi): a frame's
 * result does not depend on the other frames of the call.  pvx_yin_dev: x and the outputs are device memory (starts stays
 * a host array), work on `stream`, synchronised before the return.  Both return nfr or a negative status; nfr = 0
 * launches nothing.  pvx_yin_last_kernels: what the calling thread's last call ran ("k_yin", "k_yin/seg2", "k_yin/seg4":
 * the sums over j split into that many segments; "" when it had no frame).
 */
#define PVX_YIN_MAX_NWIND 8192
#define PVX_YIN_FALLBACK 1
#define PVX_YIN_SILENT 2
int64_t pvx_yin(const double* x, int64_t nsamp, const int64_t* starts, int64_t nfr, int nwind, int lo, int hi, double tol, double sr,
                double* freq, double* conf, double* tau, int32_t* flag, int32_t* pick);
int64_t pvx_yin_dev(const double* d_x, int64_t nsamp, const int64_t* starts, int64_t nfr, int nwind, int lo, int hi, double tol,
                    double sr, double* d_freq, double* d_conf, double* d_tau, int32_t* d_flag, int32_t* d_pick, void* stream);
const char* pvx_yin_last_kernels(void);

/* ---- Period marks: period_marks_corr / period_marks_peak (pypevoc/Periodicity.py:573-618, 621-709) ------------
 * One walk per row x[row_start[r] : row_stop[r]] (0 <= start <= stop <= nsamp), as MARKS.md states the two walks; times are
 * row times (0 at the row's first sample) and the shared track (tf, f), ntf strictly increasing knots, is read at
 * toff[r] + t (toff null: 0).  Outputs: marks (and vals) padded [nrows][max_marks], count[nrows], status[nrows].
 * status is 0 for a walk that ended by its own loop test, else the OR of:
 *   PVX_MARKS_NO_PEAK     a step's correlation has no local maximum            PVX_MARKS_PAST_END    s + P + W > L after P grew
 *   PVX_MARKS_BAD_F0      f0 <= 0, P < 1, P >= 2^31, t0 < 0, no finite f0      PVX_MARKS_NO_ADVANCE  a NaN-f0 step without a positive delay_t
 *   PVX_MARKS_CAPACITY    max_marks reached                                    PVX_MARKS_STEPS       max_steps reached
 *   PVX_MARKS_SHORT_FIT   (peak) a returned mark had fewer than 3 fit points and is its sample
 * and the row keeps the marks found so far.  pvx_marks_corr: row r starts at mark t0[r]; f_fallback is f0 where interp(t0)
 * is NaN (the reference's nanmean(f)); window >= 2.  The stretch of a step lives in LDS: with Pmax = int(sr / the smallest
 * positive finite value among f and f_fallback), 3 * window + Pmax > PVX_MARKS_CORR_MAX_LDS is PVX_ERR_UNSUPPORTED and
 * launches nothing.  pvx_marks_peak: tf null: nf == 1 (one f0) or nf == nsamp (f per sample of x); 3 <= fit_points <=
 * PVX_MARKS_MAX_FIT_POINTS; count excludes the walk's last mark, as the reference drops it.  The _dev variants take x and
 * the outputs as device memory (the lists stay host memory) and run on `stream`, synchronised on return.  A row's result
 * does not depend on the other rows of the call.  Return nrows, or a negative pvx_status.
 * pvx_marks_last_kernels: what the calling thread's last call ran ("k_marks_corr", "k_marks_peak"; "": nothing). */
#define PVX_MARKS_NO_PEAK 1
#define PVX_MARKS_PAST_END 2
#define PVX_MARKS_BAD_F0 4
#define PVX_MARKS_NO_ADVANCE 8
#define PVX_MARKS_CAPACITY 16
#define PVX_MARKS_STEPS 32
#define PVX_MARKS_SHORT_FIT 64
#define PVX_MARKS_CORR_MAX_LDS 8000
#define PVX_MARKS_MAX_FIT_POINTS 64
int64_t pvx_marks_corr(const double* x, int64_t nsamp, const int64_t* row_start, const int64_t* row_stop, const double* t0,
                       const double* toff, int64_t nrows, const double* tf, const double* f, int64_t ntf, double f_fallback, double sr,
                       int window, double min_per, int64_t max_marks, int64_t max_steps, double* marks, int32_t* count, int32_t* status);
int64_t pvx_marks_corr_dev(const double* d_x, int64_t nsamp, const int64_t* row_start, const int64_t* row_stop, const double* t0,
                           const double* toff, int64_t nrows, const double* tf, const double* f, int64_t ntf, double f_fallback,
                           double sr, int window, double min_per, int64_t max_marks, int64_t max_steps, double* d_marks,
                           int32_t* d_count, int32_t* d_status, void* stream);
int64_t pvx_marks_peak(const double* x, int64_t nsamp, const int64_t* row_start, const int64_t* row_stop, const double* toff,
                       int64_t nrows, const double* tf, const double* f, int64_t ntf, int64_t nf, double sr, int fit_points,
                       int64_t max_marks, int64_t max_steps, double* marks, double* vals, int32_t* count, int32_t* status);
int64_t pvx_marks_peak_dev(const double* d_x, int64_t nsamp, const int64_t* row_start, const int64_t* row_stop, const double* toff,
                           int64_t nrows, const double* tf, const double* f, int64_t ntf, int64_t nf, double sr, int fit_points,
                           int64_t max_marks, int64_t max_steps, double* d_marks, double* d_vals, int32_t* d_count,
                           int32_t* d_status, void* stream);
const char* pvx_marks_last_kernels(void);

/* ---- FFT filter banks: FilterBank.specout, MelFilterBank.mfcc (pypevoc/FFTFilters.py:274-292, 352-374) ----
 *
 * pvx_filterbank: frames start at i*hop while i*hop < n - nwind (:280; n <= nwind: no frame).  Per frame
 *   spec[i][b] = sum_k |fft(x[i*hop : i*hop+nwind] * wind)[k]|^2 * fb[b][k]        (:283-286)
 * with fb [nband][nwind] the reference's weights over the FULL spectrum (host array, read at call time, any shape of
 * row, all-zero rows included) and wind the bare window (no 1/wfact).  cep_mode != 0 also gives the cepstral step on
 * log(spec[i]) (no floor: log(0) = -inf): PVX_CEP_DCT1 .. PVX_CEP_DCT4 = scipy.fftpack.dct(type, norm=None) into
 * cep [nfr][nband]; PVX_CEP_IFFT = np.fft.ifft into cep [nfr][nband][2] (re, im).  A frame whose band energies are all 0
 * gets the reference's row for it ([-inf, nan, ...] DCT1 / DCT2, all nan DCT3 / DCT4, [-inf+0j, nan+nanj, ...] IFFT).
 * x: float32, float64 or int16 samples (pvx_dtype), widened on load; all arithmetic float64.  spec or cep may be NULL.
 * nwind 512 / 1024 / 2048 run one fused kernel per call, any other nwind (odd ones too) k_frames + rocFFT + one kernel
 * per batch of rows.  1 <= nband <= PVX_FBANK_MAX_NBAND, else PVX_ERR_UNSUPPORTED.  Host input is chunked by
 * PVX_MAX_DEVICE_BYTES (frames are independent: device memory does not grow with n).
 * pvx_filterbank_dev: x, spec and cep are device memory (wind and fb stay host arrays), work on `stream`, synchronised
 * before the return.  Both return the frame count or a negative status.  Calls share a per-device workspace kept for the
 * process and take turns on it.  pvx_filterbank_last_kernels: the kernels the calling thread's last call ran
 * ("k_fbank_fused<1024>", "k_frames+rocfft+k_fbank_rows"; "" when it had no frame).
 */
#define PVX_FBANK_MAX_NBAND 128
typedef enum { PVX_CEP_NONE = 0, PVX_CEP_DCT1 = 1, PVX_CEP_DCT2 = 2, PVX_CEP_DCT3 = 3, PVX_CEP_DCT4 = 4, PVX_CEP_IFFT = 5 } pvx_cep_mode;
int64_t pvx_filterbank(const void* x, int x_dtype, int64_t n, const double* wind, int nwind, int hop, const double* fb,
                       int nband, int cep_mode, double* spec, double* cep);
int64_t pvx_filterbank_dev(const void* d_x, int x_dtype, int64_t n, const double* wind, int nwind, int hop,
                           const double* fb, int nband, int cep_mode, double* d_spec, double* d_cep, void* stream);
const char* pvx_filterbank_last_kernels(void);

/* ---- windowed spectral measures (pypevoc/SoundUtils.py: SpecCentWind :142-160, SpecFlux :196-231;
 *      pypevoc/speech/SpeechAnalysis.py: SpectralMoments :82-139) ----
 *
 * Over the half spectrum |X_i[k]|, k = 0 .. nwind/2, of the frames X_i = fft(x[i*hop : i*hop+nwind] * wind):
 *   PVX_SD_RATIO  out[i] = sum_k a[k] |X_i[k]| / sum_k b[k] |X_i[k]|                   out [nfr]
 *   PVX_SD_FLUX   out[i] = sqrt(sum_k a[k] (|X_i[k]| - |X_{i+1}[k]|)^2)              out [nfr], reads frames 0 .. nfr
 *   PVX_SD_PSD    out[k] = (1/nfr) sum_i |X_i[k]|^2, k < nwind/2                      out [nwind/2]; a, b unused
 * a, b: host arrays of nwind/2 + 1 weights per half-spectrum bin (b: RATIO only): the caller folds the reference's bin
 * ranges of the full spectrum onto them (bin k and bin nwind - k share a magnitude).  wind: host array [nwind], the bare
 * window.  nfr is the caller's: the three reference functions count their frames differently (pvx_nframes(n, ..),
 * pvx_nframes(n - hop, ..), int((n - nwind - 1) / hop)); the last frame read must lie inside n, else PVX_ERR_SIZE.
 * nfr = 0: nothing is launched, out is untouched.
 * x: float32, float64 or int16 samples (pvx_dtype), widened on load; all arithmetic float64, every sum in a fixed order:
 * a value does not depend on the grid, on the other frames of the call or on where the samples came from.  The
 * periodogram adds its frames in blocks of PVX_SPECDESC_BLOCK and the blocks' sums in index order.  nwind 512 / 1024 /
 * 2048 run one fused kernel (PSD: and the pass over the block sums), any other nwind k_frames + rocFFT + one kernel per
 * batch of rows; PVX_SPECDESC_ROWS in the environment sends every nwind down the rows route.  Host input is chunked by
 * PVX_MAX_DEVICE_BYTES (PSD: in whole blocks, at least one).  pvx_specdesc_dev: x and out are device memory (wind, a, b
 * stay host arrays), work on `stream`, synchronised before the return.  Both return nfr or a negative status; calls
 * share the filter banks' per-device workspace and take turns on it.  pvx_specdesc_last_kernels: what the calling
 * thread's last call ran ("k_specdesc_fused<1024>", "k_frames+rocfft+k_specdesc_rows"; "" when it had no frame).
 */
#define PVX_SPECDESC_BLOCK 16
typedef enum { PVX_SD_RATIO = 0, PVX_SD_FLUX = 1, PVX_SD_PSD = 2 } pvx_specdesc_measure;
int64_t pvx_specdesc(const void* x, int x_dtype, int64_t n, const double* wind, int nwind, int hop, int64_t nfr, int measure,
                     const double* a, const double* b, double* out);
int64_t pvx_specdesc_dev(const void* d_x, int x_dtype, int64_t n, const double* wind, int nwind, int hop, int64_t nfr,
                         int measure, const double* a, const double* b, double* d_out, void* stream);
const char* pvx_specdesc_last_kernels(void);

/* ---- Welch-averaged cross and auto spectra, block by block (pypevoc/TransferFunctions.py: transferogram :112-185,
 *      tfe :21-26; matplotlib.mlab's csd / psd / cohere behind them) ----
 *
 * Block b = 0 .. nblk - 1 starts at sample start + b*delta of x and of y, its segment s = 0 .. nseg - 1 at s*step further on.
 * With X_s = rfft(x[.. : .. + nwind] * wind) and Y_s likewise, for the bins k = 0 .. nwind/2 (the Nyquist bin included):
 *   sxy[b][k] = (1/nseg) sum_s conj(Y_s[k]) X_s[k]      [nblk][nwind/2 + 1] complex (re, im)
 *   sxx[b][k] = (1/nseg) sum_s |X_s[k]|^2               [nblk][nwind/2 + 1]
 *   syy[b][k] = (1/nseg) sum_s |Y_s[k]|^2               [nblk][nwind/2 + 1]
 * unscaled means: the one-sided factor, Fs and sum(wind^2) of a density, the ratios of a transfer function and of a
 * coherence are the caller's.  y null: the auto spectrum of x alone (sxy, syy unused and may be null; the second
 * transform is skipped).  wind: host array [nwind], the bare window.  nblk, nseg, step, delta are the caller's; the last
 * sample read, start + (nblk-1)*delta + (nseg-1)*step + nwind - 1, must lie inside n (the length of x and of y), else
 * PVX_ERR_SIZE.  nblk = 0: nothing is launched, the outputs are untouched.
 * x, y: float32, float64 or int16 samples (pvx_dtype, one type for both), widened on load; all arithmetic float64.  A
 * bin of a block is one lane's sum, the block's segments added in index order (no atomics): a block's values do not depend
 * on the grid, on the other blocks of the call or on where the samples came from.  nwind 512 / 1024 / 2048 run one fused kernel, any
 * other nwind k_frames + rocFFT + one kernel per batch of whole blocks; PVX_XSPEC_ROWS in the environment sends every nwind
 * down the rows route.  Host input is chunked by PVX_MAX_DEVICE_BYTES in whole blocks (at least one), both signals cut at
 * the same samples.  pvx_xspec_dev: x, y and the outputs are device memory (wind stays a host array), work on `stream`,
 * synchronised before the return.  Both return nblk or a negative status; calls share the filter banks' per-device
 * workspace and take turns on it.  pvx_xspec_last_kernels: what the calling thread's last call ran
 * ("k_xspec_fused<1024>", "k_frames+rocfft+k_xspec_rows"; "" when it had no block).
 */
int64_t pvx_xspec(const void* x, const void* y, int x_dtype, int64_t n, const double* wind, int nwind, int step, int64_t start,
                  int64_t delta, int64_t nblk, int nseg, double* sxy, double* sxx, double* syy);
int64_t pvx_xspec_dev(const void* d_x, const void* d_y, int x_dtype, int64_t n, const double* wind, int nwind, int step,
                      int64_t start, int64_t delta, int64_t nblk, int nseg, double* d_sxy, double* d_sxx, double* d_syy,
                      void* stream);
const char* pvx_xspec_last_kernels(void);

/* ---- delay estimation: full cross-correlations and their peaks, block by block (pypevoc/TransferFunctions.py:
 *      determineDelay :80-109, block_delay :188-196, maxdelwind :199-244; DELAY.md) ----
 *
 * Block b = 0 .. nblk - 1 reads a[start + b*delta : .. + la] and v[start + b*delta : .. + lv] (la != lv is allowed).  Per block:
 *   prepare    each of the two on its own: PVX_DETREND_NONE, PVX_DETREND_CONSTANT (the mean is subtracted) or PVX_DETREND_LINEAR
 *              (the least-squares line is: the mean, then the slope against the centred index, closed form -- scipy.signal.detrend's
 *              default); then the product with win_a [la] / win_v [lv] (host arrays; null: ones)
 *   correlate  c[k] = sum_m a'[m + k - (lv-1)] v'[m], k = 0 .. la + lv - 2: numpy's correlate(a', v', "full")
 *   peak       lag[b] = the k of the largest c[k] (use_abs != 0: of the largest |c[k]|), the lowest k of an exact tie (np.argmax);
 *              peak[b] = c[lag[b]], signed.  A block of which a' or v' is all zero gives lag 0 and peak +0.0
 *   corr       nullable: [nblk][la + lv - 1], every c[k]
 * a, v: float32, float64 or int16 samples (pvx_dtype, one type for both), widened on load; all arithmetic float64, every sum in a
 * fixed order: a block's values do not depend on the grid, on the other blocks of the call, on how the call was cut into batches
 * or chunks, or on where the samples came from.  Two routes, chosen once per call: max(la, lv) <= PVX_XCORR_DIRECT_MAX runs
 * k_xcorr_direct, one workgroup per block with both prepared blocks in LDS and a lag per lane (no rocFFT, no plan); anything
 * longer, and every length with PVX_XCORR_FFT in the environment, pads both to P, the smallest power of two >= la + lv - 1:
 * k_xcorr_prep, two batched real rocFFTs, k_xcorr_mul, one inverse real rocFFT, k_xcorr_peak (which scales by 1/P).  P beyond
 * PVX_XCORR_MAX_P: PVX_ERR_UNSUPPORTED and no launch.  The last sample of the last block must lie inside na samples of a and nv
 * of v, else PVX_ERR_SIZE; la < 1, lv < 1, delta < 0, start < 0 or an unknown detrend code: PVX_ERR_INVALID.  nblk = 0: nothing
 * is launched, the outputs are untouched.  Host input is chunked by PVX_MAX_DEVICE_BYTES in whole blocks (at least one), both
 * signals cut at the same samples.  pvx_xcorr_peak_dev: a, v, lag, peak and corr are device memory (the windows stay host
 * arrays), work on `stream`, synchronised before the return.  Both return nblk or a negative status; calls share a per-device
 * workspace kept for the process (grow-only, one pair of rocFFT plans per P in use) and take turns on it.
 * pvx_xcorr_last_kernels: what the calling thread's last call ran ("k_xcorr_direct",
 * "k_xcorr_prep+rocfft+k_xcorr_mul+rocfft+k_xcorr_peak"; "" when it had no block).
 */
#define PVX_XCORR_DIRECT_MAX 2048
#define PVX_XCORR_MAX_P (1 << 20)
typedef enum { PVX_DETREND_NONE = 0, PVX_DETREND_CONSTANT = 1, PVX_DETREND_LINEAR = 2 } pvx_detrend;
int64_t pvx_xcorr_peak(const void* a, const void* v, int x_dtype, int64_t na, int64_t nv, int la, int lv, int64_t start, int64_t delta,
                       int64_t nblk, int detrend, const double* win_a, const double* win_v, int use_abs, int32_t* lag, double* peak,
                       double* corr);
int64_t pvx_xcorr_peak_dev(const void* d_a, const void* d_v, int x_dtype, int64_t na, int64_t nv, int la, int lv, int64_t start,
                           int64_t delta, int64_t nblk, int detrend, const double* win_a, const double* win_v, int use_abs,
                           int32_t* d_lag, double* d_peak, double* d_corr, void* stream);
const char* pvx_xcorr_last_kernels(void);

/* ---- linear prediction and glottal inverse filtering (pypevoc/speech/glottal.py: lpc :32-34, iaif_ola :36-84,
 *      InverseFilter.apply :190-234; pypevoc/speech/SpeechAnalysis.py: lpc :9-24) ----
 *
 * pvx_lpc: coef[i] = [1, a_1 .. a_order] of the frames v_i = x[i*hop : i*hop+nwind] * wind (wind NULL: the bare frame):
 * r[k] = sum_j v[j+k] v[j], k <= order, and toeplitz(r[:order]) a = -r[1:] by Levinson-Durbin (scipy's solve_toeplitz).
 * coef [nfr][order+1].  0 <= order <= PVX_LPC_MAX_ORDER, 1 <= nwind <= PVX_LPC_MAX_NWIND, else PVX_ERR_UNSUPPORTED.
 *
 * pvx_iaif: Alku's iterative adaptive inverse filtering of the frames x[i*hop : i*hop+nwind], i < nfr, as
 * InverseFilter.apply computes it (GLOTTAL.md restates the steps): the high-pass FIR hp_b [ntaps] with its
 * round_half_even(ntaps/2 - 1) samples of delay removed, the ramp of tract_order + 1 samples in front of the frame, a
 * first-order LPC, n_it rounds of vocal-tract (tract_order) and glottal (glottal_order) LPC, inverse FIR and leaky
 * integration (v[j] += leak * v[j-1]), and the final vocal-tract pass.  lpc_wind [nwind] windows the vectors the LPCs
 * see.  Outputs, each of them nullable:
 *   g, dg   [nfr][nwind]  the frames' glottal flow and its derivative
 *   vt      [nfr][tract_order+1]  the last vocal-tract filter of each frame
 *   gc      [nfr][glottal_order+1]  the last glottal filter; n_it = 0: [nfr][2], the first-order one
 *   glot, dglot [n]  the overlap-add of g * ola_wind and dg * ola_wind (ola_wind [nwind], needed for these two only),
 *           divided by the sum of the windows where that sum is > 0; a sample adds its frames in ascending order
 * nfr is the caller's (iaif_ola: pvx_nframes(n, nwind, hop)); the last sample read, (nfr-1)*hop + nwind - 1, must lie
 * inside n, else PVX_ERR_SIZE.  nfr = 0: nothing is launched, glot and dglot are zeroed.  Limits (compile time):
 * 2 <= nwind <= PVX_IAIF_MAX_NWIND, 1 <= ntaps <= PVX_IAIF_MAX_TAPS, orders 0 .. PVX_LPC_MAX_ORDER, n_it >= 0; beyond
 * them PVX_ERR_UNSUPPORTED and no launch.
 *
 * Both: x float32, float64 or int16 samples (pvx_dtype), widened on load; all arithmetic float64, every sum in a fixed
 * order: a value does not depend on the grid, on the other frames of the call or on where the samples came from.  A
 * frame whose Levinson recursion meets a prediction error of exactly 0 (a silent frame: the reference raises LinAlgError
 * "Singular principal minor") makes the call return PVX_ERR_SINGULAR with the first such frame in *singular_frame
 * (nullable; -1 otherwise); the outputs are then unspecified.  Host input is processed in chunks of whole frames sized
 * by PVX_MAX_DEVICE_BYTES (per buffer; default 256 MiB), a chunk recomputing the frames that overlap its first and last
 * output samples: the bits do not depend on the chunking.  The _dev forms take device memory for x and every output
 * (hp_b and the windows stay host arrays), group their frames the same way, work on `stream` and are synchronised
 * before they return.  All four return nfr or a negative status.  pvx_iaif_last_kernels: what the calling thread's last
 * pvx_iaif / pvx_lpc call ran ("k_iaif_frames+k_iaif_ola", "k_iaif_frames", "k_lpc_frames"; "" when it had no frame).
 */
#define PVX_LPC_MAX_ORDER 128
#define PVX_LPC_MAX_NWIND 16384
#define PVX_IAIF_MAX_NWIND 4096
#define PVX_IAIF_MAX_TAPS 4095
int64_t pvx_lpc(const void* x, int x_dtype, int64_t n, const double* wind, int nwind, int hop, int64_t nfr, int order, double* coef,
                int64_t* singular_frame);
int64_t pvx_lpc_dev(const void* d_x, int x_dtype, int64_t n, const double* wind, int nwind, int hop, int64_t nfr, int order,
                    double* d_coef, int64_t* singular_frame, void* stream);
int64_t pvx_iaif(const void* x, int x_dtype, int64_t n, int nwind, int hop, int64_t nfr, const double* hp_b, int ntaps,
                 const double* lpc_wind, const double* ola_wind, int tract_order, int glottal_order, double leak, int n_it,
                 double* glot, double* dglot, double* g, double* dg, double* vt, double* gc, int64_t* singular_frame);
int64_t pvx_iaif_dev(const void* d_x, int x_dtype, int64_t n, int nwind, int hop, int64_t nfr, const double* hp_b, int ntaps,
                     const double* lpc_wind, const double* ola_wind, int tract_order, int glottal_order, double leak, int n_it,
                     double* d_glot, double* d_dglot, double* d_g, double* d_dg, double* d_vt, double* d_gc,
                     int64_t* singular_frame, void* stream);
const char* pvx_iaif_last_kernels(void);

/* ---- formants and polynomial roots (pypevoc/speech/SpeechAnalysis.py: Formants :220-319, lpc2form :186-209;
 *      pypevoc/speech/glottal.py: lpcc2pole :249-272; FORMANTS.md) ----
 *
 * pvx_polyroots: the roots of n real polynomials coef[i][0] z^order + ... + coef[i][order] (np.roots' argument order), one
 * wave per polynomial.  1 <= order <= PVX_ROOTS_MAX_ORDER, else PVX_ERR_UNSUPPORTED and no launch; a zero leading coefficient
 * is PVX_ERR_INVALID.  re, im [n][order], canonical: a real root has imaginary part +0.0 and complex roots are exact conjugate
 * pairs, trailing coefficients that are exactly 0 give exact zero roots.  Order within a row: first the nkept[i] roots with
 * imag >= 0 by ascending atan2(im, re), equal angles by ascending |z|, then their conjugates in the partners' order.
 * status [n]: 0, or 2 where the iteration met its compile-time bound of iterations without converging; the call then returns
 * PVX_ERR_NOCONV with the first such row in *noconv_row (nullable; -1 otherwise).  re, im, nkept, status are each nullable.
 *
 * pvx_formants: Formants' device half.  d[i] = x[i] - x[i+1] with the last sample unchanged (preemph != 0; else d = x), samples
 * widened to float64 first; y = resample_poly(d, 1, down): y[m] = sum_k taps[ntaps-1-k] dz[m down + k - (ntaps-1)/2] over the
 * zero extension dz of d, m < ceil(n / down), the taps in ascending k (down == 1: y = d, taps unused and nullable; else ntaps
 * is odd); the frames y[i*hop : i*hop+nwind] * wind, i < nfr, go through pvx_lpc's autocorrelation and Levinson recursion at
 * `order` and the roots of [1, a_1 .. a_order] through pvx_polyroots' iteration.  Rows per frame, each nullable:
 *   nkept            the number of roots with imag >= 0
 *   freq, bw [order] atan2(im, re) fs / 2 pi and -0.5 (fs / 2 pi) log |z| of those roots in the order above, NaN beyond nkept
 *   re, im   [order] all roots, canonical and ordered as pvx_polyroots'
 *   lpc    [order+1] [1, a_1 .. a_order]
 * The last decimated sample read, (nfr-1)*hop + nwind - 1, must lie inside ceil(n / down), else PVX_ERR_SIZE.  Limits:
 * 1 <= nwind <= PVX_LPC_MAX_NWIND, 1 <= order <= PVX_ROOTS_MAX_ORDER; beyond them PVX_ERR_UNSUPPORTED and no launch.  A
 * silent frame returns PVX_ERR_SINGULAR and *singular_frame as pvx_lpc does, a frame whose roots did not converge
 * PVX_ERR_NOCONV and *noconv_row.  All arithmetic is float64 with every sum in a fixed order.  Frames are processed in groups
 * sized by PVX_MAX_DEVICE_BYTES (per buffer), a group decimating only the samples its frames read: the bits do not depend on
 * the grouping or on where the samples came from.  The _dev forms take device memory for x (coef) and every output (taps and
 * wind stay host arrays), work on `stream` and are synchronised before they return.  All four return nfr / n or a negative
 * status.  pvx_formants_last_kernels: what the calling thread's last call of the four ran ("k_preemph_decim+k_formant_frames",
 * "k_polyroots"; "" when it launched nothing).
 */
#define PVX_ROOTS_MAX_ORDER 64
int64_t pvx_polyroots(const double* coef, int64_t n, int order, double* re, double* im, int32_t* nkept, int32_t* status,
                      int64_t* noconv_row);
int64_t pvx_polyroots_dev(const double* d_coef, int64_t n, int order, double* d_re, double* d_im, int32_t* d_nkept, int32_t* d_status,
                          int64_t* noconv_row, void* stream);
int64_t pvx_formants(const void* x, int x_dtype, int64_t n, int preemph, int down, const double* taps, int ntaps, const double* wind,
                     int nwind, int hop, int64_t nfr, int order, double fs, int32_t* nkept, double* freq, double* bw, double* re,
                     double* im, double* lpc, int64_t* singular_frame, int64_t* noconv_row);
int64_t pvx_formants_dev(const void* d_x, int x_dtype, int64_t n, int preemph, int down, const double* taps, int ntaps,
                         const double* wind, int nwind, int hop, int64_t nfr, int order, double fs, int32_t* d_nkept, double* d_freq,
                         double* d_bw, double* d_re, double* d_im, double* d_lpc, int64_t* singular_frame, int64_t* noconv_row,
                         void* stream);
const char* pvx_formants_last_kernels(void);

/* ---- LPC spectral envelopes and refined peaks (pypevoc/speech/SpeechAnalysis.py: lpc2form_full :211-218;
 *      pypevoc/PeakFinder.py: findpos :155-194 with the default thresholds, refine :331-372, refine_all :374-413;
 *      ENVELOPE.md) ----
 *
 * pvx_lpc_envelope: for each of n coefficient rows coef[i][0 .. order] (pvx_formants' lpc rows, [1, a_1 .. a_order]; coef[i][0]
 * need not be 1, a zero there is PVX_ERR_INVALID) the envelope y_k = 1 / |sum_j coef[i][j] z_k^j|, z_k = exp(-i pi k / npts),
 * k < npts -- abs(freqz([1], coef[i], worN=npts)[1]) --, one wave per row.  Its peaks are the indices 1 <= k <= npts - 2 with
 * y[k-1] < y[k] >= y[k+1] (a NaN compares false), ascending; each is refined through its two neighbours: c = y[k],
 * b = (y[k+1] - y[k-1]) / 2, a = (y[k+1] + y[k-1]) / 2 - c, lpos = -b / 2 / a, val = a lpos^2 + b lpos + c and pos =
 * np.interp(k + lpos, arange(npts), x) on the axis x_k = k fs / (2 npts).  Outputs, each nullable: env [n][npts]; npk [n], a
 * row's number of peaks; idx [n][maxpk], -1 beyond npk; pos, val [n][maxpk], NaN beyond npk.  A row with more than maxpk peaks
 * makes the call return PVX_ERR_SIZE with the first such row in *overflow_row (nullable; -1 otherwise): its first maxpk peaks
 * are written and npk holds its full count (idx, pos and val all null: nothing can overflow).  A root on the unit circle at a
 * grid point gives inf there, as in scipy: not handled.
 *
 * pvx_peaks_refine: the same scan and refinement on n rows y[i][0 .. npts) with the axis x[npts] (null: arange(npts)).  With
 * sel [n][maxpk], int32 and -1 padded, the scan is skipped and the given indices are refined slot by slot (npk: the slots that
 * are not -1), the fit where y[k] > y[k-1] and y[k] >= y[k+1], else refine's other branch: pos = x[k], val = y[k].  A given
 * index outside 1 .. npts - 2 is PVX_ERR_INVALID.
 *
 * Limits: 1 <= order <= PVX_ROOTS_MAX_ORDER and 1 <= npts <= PVX_ENV_MAX_NPTS, else PVX_ERR_UNSUPPORTED and no launch; npts < 3,
 * n < 0 or maxpk < 0 is PVX_ERR_INVALID.  n = 0 launches nothing.  float64 throughout; a point's value depends on its row and
 * index alone.  Host rows are processed in groups of whole rows sized by PVX_MAX_DEVICE_BYTES (per buffer): a row's bits do not
 * depend on the grouping, on its place in the batch or on where the input came from.  The _dev forms take device memory for
 * every array, work on `stream` and are synchronised before they return.  All four return n or a negative status.
 * pvx_envelope_last_kernels: what the calling thread's last call of the four ran ("k_lpc_envelope", "k_peaks_refine"; "" when
 * it launched nothing).
 */
#define PVX_ENV_MAX_NPTS 16384
int64_t pvx_lpc_envelope(const double* coef, int64_t n, int order, int npts, double fs, int maxpk, double* env, int32_t* npk, int32_t* idx,
                         double* pos, double* val, int64_t* overflow_row);
int64_t pvx_lpc_envelope_dev(const double* d_coef, int64_t n, int order, int npts, double fs, int maxpk, double* d_env, int32_t* d_npk,
                             int32_t* d_idx, double* d_pos, double* d_val, int64_t* overflow_row, void* stream);
int64_t pvx_peaks_refine(const double* y, int64_t n, int npts, const double* x, int maxpk, const int32_t* sel, int32_t* npk, int32_t* idx,
                         double* pos, double* val, int64_t* overflow_row);
int64_t pvx_peaks_refine_dev(const double* d_y, int64_t n, int npts, const double* d_x, int maxpk, const int32_t* d_sel, int32_t* d_npk,
                             int32_t* d_idx, double* d_pos, double* d_val, int64_t* overflow_row, void* stream);
const char* pvx_envelope_last_kernels(void);

/* ---- speech segmentation on band energies (pypevoc/speech/SpeechSegmenter.py: process :203-222, the parabolic fit :224-260,
 *      refine_segment_all_bands :262-302, refine_transition_points :39-124; SEGMENT.md) ----
 *
 * All three stages read band energies as pvx_filterbank writes them, spec [frames][nband], take dB = 10 log10(energy)
 * themselves (no floor: 0 gives -inf, and -inf - -inf a NaN that compares false everywhere) and add in numpy's order, so
 * a value depends on its own frames alone.  1 <= nband <= PVX_FBANK_MAX_NBAND, else PVX_ERR_UNSUPPORTED and no launch.
 *
 * pvx_seg_detect: det[i] = sum_b |dB[i+1][b] - dB[i][b]|, i < nfr - 1 (nullable).  Index 1 <= i <= nfr - 3 is kept iff
 * det[i-1] < det[i], det[i+1] < det[i] (both strict) and det[i] > thresh.  idx [maxseg]: the kept indices, ascending and
 * left-packed; fpos [maxseg]: i + lpos of c = det[i], b = (det[i+1] - det[i-1]) / 2, a = (det[i+1] + det[i-1]) / 2 - c,
 * lpos = -b / 2 / a (each nullable; slots beyond the count are not written).  *count: the full number of kept indices.
 * Returns the number written, or PVX_ERR_SIZE when count > maxseg (the first maxseg are written).  nfr >= 1 (nfr < 2^31);
 * nfr = 1 launches nothing.
 *
 * pvx_seg_refine: per segment s < nseg and band b, with ranges[s] = {ibef0, ibef1, iaft0, iaft1, iall0, iall1} (host array,
 * int32, each range [first, last + 1) of rows of spec, the two sides inside iall): valb / vala = np.median of dB over ibef /
 * iaft (NaN for an empty side or one that holds a NaN); valm = (valb + vala) / 2, or with has_thr min(vala, valb) + thr; the
 * crossings k, 0 <= k <= len(iall) - 2, with (f[k] - valm) (f[k+1] - valm) < 0 over f = dB[iall]; of them the k nearest to
 * len(ibef), the lower of two equally near: cross [nseg][nband], -1 for none.  pk = tfine[k + ibef0] sr with tfine[j] =
 * (j hop + half) / tsr, or tseg[s] (host array) without a crossing; w = |valb - vala|; out[s] = sum_b pk w / sum_b w.
 * valb, vala [nseg][nband], cross and out are each nullable.  A side longer than PVX_SEG_MAX_SIDE or an iall longer than
 * 2 PVX_SEG_MAX_SIDE + 1: PVX_ERR_UNSUPPORTED; a range outside 0 .. nfine or a side outside iall: PVX_ERR_INVALID.  Returns
 * nseg; nseg = 0 launches nothing.
 *
 * pvx_seg_transitions: refine_transition_points on nser series of n points, series s at v[s row_stride + k elem_stride];
 * escale > 0: v holds energies and x = 10 log10(v escale), escale = 0: x = v.  tx: host array of ascending times, [n]
 * (tx_stride 0) or [nser][n] (tx_stride n); trt: host array [nser].  Per series ttr, vbef, vaft and status:
 *   PVX_SEG_OUTSIDE      trt outside tx: (trt, 0, 0)
 *   PVX_SEG_EMPTY_SIDE   no point after trt, or none before it in modes MINMAX and PCT: NaN
 *   PVX_SEG_NO_CROSSING  vbef and vaft are written, ttr is NaN
 * mode PVX_SEG_MINMAX / MEDIAN / MEAN / PCT (np.percentile's linear method at pct and 100 - pct, 0 <= pct <= 100).
 * 1 <= n <= PVX_SEG_MAX_SERIES, else PVX_ERR_UNSUPPORTED.  Returns nser; nser = 0 launches nothing.
 *
 * The _dev forms take device memory for the energies and every output (ranges, tseg, tx and trt stay host arrays), work on
 * `stream` and are synchronised before they return.  pvx_segment_last_kernels: what the calling thread's last call of the
 * six ran ("k_seg_detect", "k_seg_refine", "k_seg_transitions"; "" when it launched nothing).
 */
#define PVX_SEG_MAX_SIDE 256
#define PVX_SEG_MAX_SERIES 4096
typedef enum { PVX_SEG_MINMAX = 0, PVX_SEG_MEDIAN = 1, PVX_SEG_MEAN = 2, PVX_SEG_PCT = 3 } pvx_seg_mode;
typedef enum { PVX_SEG_OK = 0, PVX_SEG_OUTSIDE = 1, PVX_SEG_EMPTY_SIDE = 2, PVX_SEG_NO_CROSSING = 3 } pvx_seg_status;
int64_t pvx_seg_detect(const double* spec, int64_t nfr, int nband, double thresh, int maxseg, double* det, int32_t* idx, double* fpos,
                       int64_t* count);
int64_t pvx_seg_detect_dev(const double* d_spec, int64_t nfr, int nband, double thresh, int maxseg, double* d_det, int32_t* d_idx,
                           double* d_fpos, int64_t* count, void* stream);
int64_t pvx_seg_refine(const double* spec, int64_t nfine, int nband, const int32_t* ranges, const double* tseg, int64_t nseg, int hop,
                       double half, double tsr, double sr, double thr, int has_thr, double* valb, double* vala, int32_t* cross,
                       double* out);
int64_t pvx_seg_refine_dev(const double* d_spec, int64_t nfine, int nband, const int32_t* ranges, const double* tseg, int64_t nseg,
                           int hop, double half, double tsr, double sr, double thr, int has_thr, double* d_valb, double* d_vala,
                           int32_t* d_cross, double* d_out, void* stream);
int64_t pvx_seg_transitions(const double* v, int64_t nser, int n, int64_t row_stride, int64_t elem_stride, double escale, const double* tx,
                            int64_t tx_stride, const double* trt, int mode, double pct, double thr, double* ttr, double* vbef,
                            double* vaft, int32_t* status);
int64_t pvx_seg_transitions_dev(const double* d_v, int64_t nser, int n, int64_t row_stride, int64_t elem_stride, double escale,
                                const double* tx, int64_t tx_stride, const double* trt, int mode, double pct, double thr, double* d_ttr,
                                double* d_vbef, double* d_vaft, int32_t* d_status, void* stream);
const char* pvx_segment_last_kernels(void);

/* ---- pitch jumps on rows of tracks (pypevoc/speech/PitchJumps.py: zscore_wind :50-64, linreg_err :67-84, linreg2_err :87-121,
 *      JumpDetector.detect_jumps :178-207, calc_jump_params :209-242; JUMPS.md) ----
 *
 * Every entry point takes `rows` tracks padded to nmax frames, row r holding len[r] of them (0 <= len[r] <= nmax; a row of
 * length 0 is legal; len NULL: every row holds nmax).  All arrays are float64 / int32; rows * nmax < 2^31.  The number of
 * launches does not depend on rows, and a row's results do not depend on the other rows.
 *
 * pvx_jump_select: m[r][i] = sqrt(sum_k mag[r][i][k]^2), the sum in np.sum's order of a contiguous run of K values (0.0 from
 * len[r] on); isel[r][i] = m > max_i(m) * mag_threshold (strict; a NaN magnitude makes the maximum NaN and selects nothing);
 * tsel, fsel [rows][nmax]: the selected (t, f0) pairs in ascending order, left-packed, 0.0 behind them; nsel [rows] their
 * number; status [rows]: PVX_JUMP_NAN when a magnitude or a selected t / f0 is NaN.  1 <= K <= PVX_JUMP_MAX_K, else
 * PVX_ERR_UNSUPPORTED.  Returns rows.  pvx_jump_select_resident: the same for the one signal of a plan after
 * pvx_analyze_resident -- mag and t are read where they are, f0 is the host array [F] that pvx_f0_resident gave, the outputs
 * are host arrays of F (nsel and status of one) --, so that the (F, K) array does not cross the link.
 *
 * pvx_winstat: out[r][i] for i = wleft, wleft + hop, .. < len[r] - wright, 0.0 elsewhere, over the window j in
 * [i - wleft, i + wright):
 *   PVX_WIN_ZMEAN    (x[i] - mean) / std, std with ddof 0 and two-pass (zscore_wind, kind 'mean')
 *   PVX_WIN_ZMEDIAN  (x[i] - median) / (pct75 - pct25), np.percentile's linear rule (kind 'median'); NaN with a NaN in the window
 *   PVX_WIN_LINREG   (x[i] - line(t[i])) / std(residuals) of the least-squares line over the window (linreg_err)
 *   PVX_WIN_LINREG2  the pooled-variance two-sample t of the left side's [i - wleft, i) residuals against the right side's
 *                    [i, i + wright) about the left line (ttl, flag PVX_WIN_USE_L) and of the right against the left about
 *                    the right line (ttr, PVX_WIN_USE_R): the mean of {ttl, -ttr} as flagged, NaN with neither (linreg2_err)
 * The line is b = sum((t - tm)(x - xm)) / sum((t - tm)^2), a = xm - b tm.  3 <= wleft <= PVX_JUMP_MAX_SIDE; wright the same,
 * or 0 for the kinds other than LINREG2; otherwise (wright < 0 too) PVX_ERR_UNSUPPORTED and no launch.  hop >= 1.  Returns rows.
 *
 * pvx_jump_pick: index 1 <= i <= len[r] - 2 is an up-jump iff zs[i] > zs[i-1], zs[i] > zs[i+1] (both strict) and zs[i] >
 * t_threshold, a down-jump iff zs[i] < zs[i-1], zs[i] < zs[i+1] and zs[i] < -t_threshold (a NaN compares false).  idx, dir
 * [rows][maxjump]: both kinds merged, ascending and left-packed, dir +1 / -1; njump [rows]: the full count.  Per listed jump,
 * with il = max(0, i - nsl), ir = min(i + nsl, len[r]): intcpts [rows][maxjump][2] the lines over [il, i) and [i + 1, ir) at
 * t[i]; sumres [rows][maxjump][2] = sqrt(sum(res^2) / (i - il)) and sqrt(sum(res^2) / (ir - i)) (one more than the points on
 * the right: the reference's divisor); status [rows][maxjump]: PVX_JUMP_SHORT_SIDE when a side has fewer than two points (its
 * values are NaN; the reference raises), PVX_JUMP_NAN when a value is NaN otherwise.  nsl >= 1.  Returns rows, or
 * PVX_ERR_SIZE when a row has more than maxjump jumps (*overflow_row says which; the first maxjump are written and fitted).
 * zs NULL: idx [rows][maxjump] and njump [rows] are the caller's (calc_jump_params on indices set by hand), dir is not
 * read, and only intcpts, sumres and status are written; an index outside its row gives NaN and PVX_JUMP_SHORT_SIDE.
 *
 * Arguments are checked before a device is needed.  The _dev forms take device memory for every array (len too), work on
 * `stream` and are synchronised before they return.  pvx_jumps_last_kernels: what the calling thread's last call of these
 * ran ("k_jump_select", "k_winstat", "k_jump_pick"; "" when it launched nothing).
 */
#define PVX_JUMP_MAX_SIDE 256
#define PVX_JUMP_MAX_K 4096
typedef enum { PVX_WIN_ZMEAN = 0, PVX_WIN_ZMEDIAN = 1, PVX_WIN_LINREG = 2, PVX_WIN_LINREG2 = 3 } pvx_win_kind;
#define PVX_WIN_USE_L 1
#define PVX_WIN_USE_R 2
#define PVX_JUMP_SHORT_SIDE 1
#define PVX_JUMP_NAN 2
int64_t pvx_jump_select(const double* mag, const double* f0, const double* t, const int32_t* len, int64_t rows, int nmax, int K,
                        double mag_threshold, double* m, int32_t* isel, double* tsel, double* fsel, int32_t* nsel, int32_t* status);
int64_t pvx_jump_select_dev(const double* d_mag, const double* d_f0, const double* d_t, const int32_t* d_len, int64_t rows, int nmax, int K,
                            double mag_threshold, double* d_m, int32_t* d_isel, double* d_tsel, double* d_fsel, int32_t* d_nsel,
                            int32_t* d_status, void* stream);
int64_t pvx_jump_select_resident(pvx_plan* plan, const double* f0, double mag_threshold, double* m, int32_t* isel, double* tsel,
                                 double* fsel, int32_t* nsel, int32_t* status);
int64_t pvx_winstat(const double* t, const double* x, const int32_t* len, int64_t rows, int nmax, int kind, int wleft, int wright, int hop,
                    int flags, double* out);
int64_t pvx_winstat_dev(const double* d_t, const double* d_x, const int32_t* d_len, int64_t rows, int nmax, int kind, int wleft, int wright,
                        int hop, int flags, double* d_out, void* stream);
int64_t pvx_jump_pick(const double* zs, const double* t, const double* x, const int32_t* len, int64_t rows, int nmax, double t_threshold,
                      int nsl, int maxjump, int32_t* idx, int32_t* dir, int32_t* njump, double* intcpts, double* sumres, int32_t* status,
                      int64_t* overflow_row);
int64_t pvx_jump_pick_dev(const double* d_zs, const double* d_t, const double* d_x, const int32_t* d_len, int64_t rows, int nmax,
                          double t_threshold, int nsl, int maxjump, int32_t* d_idx, int32_t* d_dir, int32_t* d_njump, double* d_intcpts,
                          double* d_sumres, int32_t* d_status, int64_t* overflow_row, void* stream);
const char* pvx_jumps_last_kernels(void);

/* ---- fricative descriptors of many snippets of one signal (pypevoc/speech/SpeechAnalysis.py: FricativeDataFromSnip
 *      :349-384; FRICATIVES.md) ----
 *
 * Snippet r = 0 .. nrows - 1 is x[starts[r] : starts[r] + L], one L per call; starts is a host array in every form, in any
 * order, overlaps allowed.  With nper = min(nwind, L), nov = nper/2, step = nper - nov and nseg = (L - nov)/step (scipy's
 * count), segment s is the nper samples from starts[r] + s*step and, for the bins k = 0 .. nper/2,
 *   X_s = rfft((seg_s - mean(seg_s)) * win)       the mean subtracted in the time domain, before the window
 *   psd[r][k] = c[k] (1/nseg) sum_s |X_s[k]|^2 / (sr sum(win^2))       [nrows][nper/2 + 1]
 * c[k] = 2, but 1 at k = 0 and, for even nper, at the last bin: scipy.signal.welch(x, fs=sr, nperseg=nwind) with its
 * defaults.  win: host array [nper], NULL for the periodic Hann window.  x: float32, float64 or int16 samples (pvx_dtype),
 * widened on load; all arithmetic float64.
 *
 * The descriptors of a row (S, freq) of nb >= 2 bins, desc[r] = f_max, slope_left, slope_right, cent, stdev, skew, kurt:
 * with y = 10 log10 S and imax = argmax S (first index on ties), f_max is freq interpolated at the three-point refinement
 * of y around max(imax, 1) (the bin itself unless it is a strict maximum of its neighbours; freq[nb-1] at the last bin),
 * the slopes are 1000 x the least-squares slopes of y over freq on the bins 0 .. imax and imax .. nb-1 (centred sums),
 * the last four are the centre, standard deviation, skewness and excess kurtosis of the distribution S over freq.  freq is
 * a host array [nb] in every form (the caller's np.fft.rfftfreq).  status[r]: PVX_FRIC_END_PEAK when imax is 0 or nb-1 (the
 * fit over one point is NaN), PVX_FRIC_BAD_BIN when a bin is zero, negative or not finite (every output that reads that
 * bin's logarithm is NaN; a row whose sum is zero is NaN throughout).  Nothing is clamped.  rms[r]: the population standard
 * deviation of all L samples of the snippet.
 *
 * pvx_welch writes psd, pvx_fric_desc the descriptors of given psd rows, pvx_fricative both and rms in one call (psd may be
 * NULL there).  A row is one wave's work with a fixed summation order: its values do not depend on the grid, on the other
 * rows of the call, on their order or on where the samples came from, and pvx_fric_desc on the psd rows of pvx_fricative
 * returns that call's descriptors bit for bit.  nper 512 / 1024 / 2048 run one fused kernel for the spectra, any other
 * nper a framing kernel + rocFFT + an accumulation kernel per batch of whole snippets; PVX_FRIC_ROWS in the environment
 * sends every nper down the rows route.  A host call copies the span of samples its rows cover; when that exceeds
 * PVX_MAX_DEVICE_BYTES it runs groups of consecutive rows (at least one), each with its own span.  PVX_ERR_SIZE for a
 * snippet that leaves the n samples (the message names the row), L < 2, nrows < 0 or nb < 2; nrows = 0 returns 0 and
 * launches nothing.  The _dev forms take device memory for the samples and every output, work on `stream` and are
 * synchronised before they return.  All return nrows or a negative status; calls share the filter banks' per-device
 * workspace and take turns on it.  pvx_fric_last_kernels: what the calling thread's last call ran
 * ("k_fric_fused<1024>+k_fric_desc+k_fric_rms", "k_fric_frames+rocfft+k_fric_acc", "k_fric_desc"; "" when it had no row).
 */
#define PVX_FRIC_END_PEAK 1
#define PVX_FRIC_BAD_BIN 2
int64_t pvx_welch(const void* x, int x_dtype, int64_t n, const int64_t* starts, int64_t nrows, int L, int nwind, const double* win,
                  double sr, double* psd);
int64_t pvx_welch_dev(const void* d_x, int x_dtype, int64_t n, const int64_t* starts, int64_t nrows, int L, int nwind, const double* win,
                      double sr, double* d_psd, void* stream);
int64_t pvx_fric_desc(const double* psd, int64_t nrows, int nb, const double* freq, double* desc, int32_t* imax, int32_t* status);
int64_t pvx_fric_desc_dev(const double* d_psd, int64_t nrows, int nb, const double* freq, double* d_desc, int32_t* d_imax,
                          int32_t* d_status, void* stream);
int64_t pvx_fricative(const void* x, int x_dtype, int64_t n, const int64_t* starts, int64_t nrows, int L, int nwind, const double* win,
                      double sr, const double* freq, double* psd, double* desc, int32_t* imax, int32_t* status, double* rms);
int64_t pvx_fricative_dev(const void* d_x, int x_dtype, int64_t n, const int64_t* starts, int64_t nrows, int L, int nwind,
                          const double* win, double sr, const double* freq, double* d_psd, double* d_desc, int32_t* d_imax,
                          int32_t* d_status, double* d_rms, void* stream);
const char* pvx_fric_last_kernels(void);

/* ---- multi-GPU result gather: compact wire format --------------------------------------
 *
 * The reference has no multi-device path; its results are the five float64 [F, K] arrays of
 * PV.run_pv (PV.py:256-264), 40 B per peak slot.  For the gather of sharded results to one GPU
 * (RCCL over xGMI, link-bound) a shard's rows are packed to 18 B (precision 32) or 26 B
 * (precision 64) per slot: f (f64), mag, ph (f32|f64), binno (u16) + totalmag (f64) per row;
 * realph = ph + pi*(fbin[binno] - f)/fstep (PV.py:146, 207) is recomputed by the receiver.
 * pvx_unpack_rows_dev(pvx_pack_rows_dev(x)) == x bit for bit for anything pvx_analyze* produced
 * with the same plan parameters.  `rows` = frames of all signals of the shard; all pointers are
 * device memory; launches are asynchronous on `stream`.
 */
/* Wire format of a plan: 1 (default) as above; 2, for plans at precision 32: 14 B per slot.  There a peak's frequency is a float64
 * function of its bin and ONE float32 value (the unwrapped phase offset of PV.py:140-147, or one of twelve cases after a silent
 * frame): the block carries that value instead of f and the receiver evaluates the kernels' own expression -- the same bits.  Every
 * function below follows the plan's format; pack of arrays that no precision-32 analysis wrote leaves NaN frequencies in format 2.
 * PVX_ERR_UNSUPPORTED for format 2 on a precision-64 plan. */
int pvx_plan_set_wire_format(pvx_plan* plan, int format);
int pvx_plan_get_wire_format(const pvx_plan* plan);
int64_t pvx_wire_bytes(const pvx_plan* plan, int64_t rows);
int pvx_pack_rows_dev(const pvx_plan* plan, int64_t rows, const double* d_f, const double* d_mag,
                      const double* d_ph, const double* d_binno, const double* d_totalmag,
                      void* d_wire, void* stream);
/* run_pv of nsig device-resident signals straight into a wire block of pvx_wire_bytes(plan, nsig * F) bytes: what a rank of a
 * multi-GPU job hands to the gather (bench.py).  The fused float32 kernel of nfft 512 / 1024 / 2048 writes the block itself -- 18 (14 in
 * format 2) bytes per slot instead of 40, and no packing pass behind the analysis --; any other plan analyses into a plan-owned block and packs
 * it.  pvx_unpack_rows_dev of the block gives the arrays pvx_analyze_dev would have written, bit for bit.  Returns F. */
int64_t pvx_analyze_dev_wire(pvx_plan* plan, const void* d_x, int x_dtype, int64_t nsamp, int64_t nsig, int64_t sig_stride,
                             void* d_wire, void* stream);
int pvx_unpack_rows_dev(const pvx_plan* plan, int64_t rows, const void* d_wire, double* d_f,
                        double* d_mag, double* d_ph, double* d_realph, double* d_binno,
                        double* d_totalmag, void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* PVX_H */

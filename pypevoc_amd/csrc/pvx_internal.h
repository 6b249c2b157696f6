// pvx_internal.h -- shared declarations of libpvx_hip (gfx950 only; no host fallback).
#pragma once

#include <hip/hip_runtime.h>
#include <rocfft/rocfft.h>
#include <stdint.h>

#include "pvx.h"

// ---- error plumbing -------------------------------------------------------------------------
void pvx_set_error(const char* fmt, ...);

#define PVX_HIP_CHECK(call)                                                                     \
    do {                                                                                        \
        hipError_t e__ = (call);                                                                \
        if (e__ != hipSuccess) {                                                                \
            pvx_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__,     \
                          __LINE__);                                                            \
            return PVX_ERR_HIP;                                                                 \
        }                                                                                       \
    } while (0)

#define PVX_FFT_CHECK(call)                                                                     \
    do {                                                                                        \
        rocfft_status s__ = (call);                                                             \
        if (s__ != rocfft_status_success) {                                                     \
            pvx_set_error("%s failed: rocfft_status %d (%s:%d)", #call, (int)s__, __FILE__,     \
                          __LINE__);                                                            \
            return PVX_ERR_HIP;                                                                 \
        }                                                                                       \
    } while (0)

int pvx_require_device();  // PVX_OK or PVX_ERR_NO_DEVICE (sets the message)

// workgroups of `threads` threads and `lds` bytes of dynamic LDS of kernel `fn` that are RESIDENT on a CU together, registers included
// (hipOccupancyMaxActiveBlocksPerMultiprocessor, remembered per (device, kernel, threads, lds)); <= 0: unknown.  The general path's
// kernels size their grids as CUs x workgroups per CU: a grid sized by LDS alone launches workgroups that wait for a slot and
// then run by themselves -- nfft 512 at float64 asked for four workgroups of four waves per CU where registers admit three:
// 450 -> 505 M frames/s with the grid that fits.
int pvx_resident_blocks(const void* fn, int threads, size_t lds);

// ---- row space ------------------------------------------------------------------------------
// The analysis works on a global "row space": every signal owns F+1 consecutive rows, row 0 of a
// signal being an all-zero frame (the reference's initial oldfft = zeros, PV.py:121) and row q > 0
// being frame q-1.  A launch covers global rows [R0, R0+nrows); workspace row j holds global row
// R0-1+j, so every processed row finds its predecessor in workspace row j-1.

struct FrameParams {
    const void* x;        // input samples (InT)
    int64_t nsamp;        // samples per signal
    int64_t sig_stride;   // samples between signal starts
    int64_t F;            // frames per signal
    int64_t R0;           // first global row of this launch (workspace row 1)
    int64_t ws_rows;      // workspace rows to write (= nrows + 1)
    int64_t total_rows;   // nsig * (F + 1)
    int nfft, hop;
    const void* win;      // window * (1/wfact), T[nfft]
    int win_symmetric = 0; // w[n] == w[nfft-1-n] for every n (np.hanning and its kind): k_stft_pv may keep half of it
    void* frames;         // T [ws_rows][ldi]
    int64_t ldi;          // elements per workspace row
    // optional candidate output of the split transform (pvx_stft.h: StftParams)
    void* cand_y = nullptr;
    unsigned short* cand_bin = nullptr;
    double* cand_stats = nullptr;
    int cand_cap = 0;
    double cand_thr = 0.0;
};

struct PeaksParams {
    const void* spec;     // complex<T> [ws_rows][ldo]
    int64_t ldo;          // complex elements per row
    int64_t F, R0, nrows;
    int nfft, hop, N2, K, rad;
    double thr;           // pkthresh (PF minrattomax)
    double sr, fstep, dt;
    const double* wfbin;  // [N2] 2*pi*round_half_even(k*fstep*dt)  (PV.py:116-118)
    const double* prev0;  // optional [N2][2] spectrum preceding frame 0 of signal 0
    double *f, *mag, *ph, *realph, *binno, *t, *totalmag;
    int frames_per_wave;
    // optional: the rows' candidate peaks left by the split transform (row rel + 1 of the workspace = this launch's row rel)
    const void* cand_y = nullptr;
    const unsigned short* cand_bin = nullptr;
    const double* cand_stats = nullptr;
    int cand_cap = 0;
};

struct PeakRowsParams {   // standalone PeakFinder
    const double* y;      // [nrows][n]
    int64_t nrows;
    int n, npeaks, thr_kind, rad, cap;
    double thr_val;
    int32_t* pos;         // [nrows][cap]
    int8_t* keep;         // [nrows][cap]
    int32_t* count;       // [nrows]
};

struct FusedParams {      // k_fused.hip: window + FFT + untangle + peaks in one wave per frame
    const void* x;        // input samples
    int64_t sig_stride, F, total_rows;
    int hop, K, rad;
    double thr, sr, fstep, dt;
    const double* wfbin;
    const double* prev0;
    double *f, *mag, *ph, *realph, *binno, *t, *totalmag;
    const void* win;      // float[nfft] window / wfact
    const void* twiddle;  // float2[nfft] W_nfft^j
    float* spec_out;      // optional: half spectrum (nfft/2 complex) of global row spec_row
    int64_t spec_row;
    int64_t blocks_override;
    // k_fused_rev.hip: where a wave leaves the first spectrum it computes for the wave below it in its workgroup (whose last
    // frame needs it as its previous spectrum): float2 [workgroups x waves][nfft / 2], or NULL -- every wave then computes
    // the row below its range itself.  pvx_fused_rev_stash_bytes: what the launch of these parameters would use.
    void* stash;
    size_t stash_bytes;
    // k_fused_rev.hip: 1 = f / mag / ph / binno / totalmag point at the sections of a wire block (k_wire.hip; realph and t unused)
    int wire = 0;
};
size_t pvx_fused_rev_stash_bytes(const FusedParams& p, int nfft);
int pvx_fused_supported(int nfft, int precision, int K);
int pvx_launch_fused(const FusedParams& p, int nfft, int x_dtype, hipStream_t s);
int pvx_fused_mw_supported(int nfft, int precision, int K);     // k_fused_mw.hip: several waves per frame
int pvx_launch_fused_mw(const FusedParams& p, int nfft, int x_dtype, hipStream_t s);
int pvx_fused_ring_supported(int nfft, int precision, int K);   // k_fused_ring.hip: workgroup-shared spectrum ring
int pvx_launch_fused_ring(const FusedParams& p, int nfft, int x_dtype, hipStream_t s);
int pvx_fused_rev_supported(int nfft, int precision, int K);    // k_fused_rev.hip: independent waves, rows in descending order
// (*kc: the npks the launched instantiation has as a constant, 0 for the generic kernel -- pvx_plan_last_kernels' <kcN> suffix)
int pvx_launch_fused_rev(const FusedParams& p, int nfft, int x_dtype, hipStream_t s, int* kc = nullptr);
int pvx_fused_team_supported(int nfft, int precision, int K);   // k_fused_team.hip: nfft 4096 / 8192 as teams of k_fused_rev-shaped waves
int pvx_launch_fused_team(const FusedParams& p, int nfft, int x_dtype, hipStream_t s);
int pvx_fused_team_table_len(int nfft);                          // complex entries it wants appended to the W_nfft^j table
void pvx_fused_team_table(int nfft, const float* tw, float* out);

// k_stft.hip: fused float64 STFT into the spectrum workspace
int pvx_stft_supported(int nfft, int precision);
struct FrameParams;

// launchers (defined in the .hip files)
int pvx_launch_frames(const FrameParams& p, int x_dtype, int precision, hipStream_t s);
int pvx_launch_narrow(const double* src, float* dst, int64_t n, hipStream_t s);   // dst[i] = (float) src[i]
int pvx_launch_stft(const FrameParams& fp, void* spec, int64_t ldo, const void* twiddle, int x_dtype, int precision, hipStream_t s);
int pvx_launch_phase_peaks(const PeaksParams& p, int precision, hipStream_t s);
// k_stft_pv.hip: k_stft + k_phase_peaks in one launch (nfft 512..2048 while the peak search fits the transform buffer)
int pvx_stft_pv_supported(int nfft, int precision, int K);
int pvx_stft_pv_takes(int nfft, int precision, int x_dtype, int hop);
int pvx_launch_stft_pv(const FrameParams& fp, const PeaksParams& pp, void* spec, int64_t ldo, const void* twiddle, int x_dtype,
                       int precision, hipStream_t s);
// k_pv_rev.hip: the float64 analysis in one launch with the spectrum rows kept on chip (rows walked downwards; nfft 512 .. 2048, npks <= 64)
struct PvRevParams {
    const void* x;        // input samples
    int64_t sig_stride, F, total_rows;
    int64_t row_begin, row_end;   // the global rows this launch analyses (all: 0, total_rows)
    int hop, K, rad;
    double thr, sr, fstep, dt;
    const double* wfbin;
    const double* prev0;
    double *f, *mag, *ph, *realph, *binno, *t, *totalmag;
    const void* win;      // double[nfft] window / wfact
    const void* twiddle;  // complex double [nfft] W_nfft^j
    double* spec_out;     // optional: half spectrum (nfft/2 complex float64) of global row spec_row
    int64_t spec_row;
    int64_t blocks_override;
    int win_symmetric;
    void* stage;          // nfft 2048: double [workgroups x waves][64][5], the kept peaks' values between the frames (pvx_pv_rev_stage_bytes)
    size_t stage_bytes;
};
int pvx_pv_rev_supported(int nfft, int precision, int K);
int pvx_pv_rev_takes(int nfft, int x_dtype, int hop);
size_t pvx_pv_rev_stage_bytes(int nfft);
int pvx_launch_pv_rev(const PvRevParams& p, int nfft, int x_dtype, hipStream_t s);
// k_pv_team.hip: the same at nfft 4096 / 8192 with a team of waves per frame (hop nfft/4 or nfft/2, npks <= 64)
int pvx_pv_team_supported(int nfft, int precision, int K, int hop);
size_t pvx_pv_team_stage_bytes(int nfft);
int pvx_launch_pv_team(const PvRevParams& p, int nfft, int x_dtype, hipStream_t s);
int pvx_launch_peak_rows(const PeakRowsParams& p, hipStream_t s);
size_t pvx_phase_peaks_lds_bytes(int N2, int K, int precision, int waves);

struct TrackParams {
    const double* f;      // [F][K]
    const double* mag;
    int64_t F;
    int K;
    double maxjmp;
    int32_t* partial_id;  // [F][K]
    int32_t* part_start;  // [cap]
    int32_t* part_len;    // [cap]
    int64_t cap;
    // workspace
    int32_t* link;        // [F][K]  >= 0: continues that slot of frame-1; -1: empty slot; <= -2: starts a partial,
                          //         -(link + 2) = its rank among the new partials of its frame (creation order)
    int32_t* newcount;    // [F]     partials created at each frame
    int64_t* newbase;     // [F+1]   exclusive scan of newcount
    int32_t* root;        // [F][K]  flattened index of the first point of the slot's partial
    unsigned char* succ;  // [F][K]  1 if a peak of the next frame continues this one
    int64_t* npartials;   // [1]
    int64_t* maxend;      // [1]  last frame that holds a point of any partial = max(SinSum.end) (PV.py:1059)
    int chunk, fpw;       // frames per k_track_links workgroup = chunk length of the root step (a power of two), and
                          // frames a wave takes in turn (set by pvx_launch_track)
    // k_track_links_lane (npks <= 8): per chunk of 256 frames the partials it creates (flag bits as newcount), the last
    // frame with a peak, and the scan of the totals; nullptr: newbase holds the scan over all frames
    int32_t* chunktot = nullptr;     // [ceil(F / 256)]
    int32_t* chunklast = nullptr;    // [ceil(F / 256)]
    int64_t* chunkbase = nullptr;    // [ceil(F / 256) + 1]
    // rows wider than 8 slots that hold at most 8 valid peaks (the reference's default npks is 20; a tone has a handful) go
    // through k_track_links_lane too: it works on slots 0 .. 7 and stores gen into *wide when a frame has a valid peak beyond;
    // the caller then launches again with wide = nullptr (the wave-per-frame kernels)
    unsigned* wide = nullptr;        // [1], read by the host with the result words (page-locked host memory when the caller has some)
    unsigned* wide_dev = nullptr;    // [1], the same in device memory: what the launch's later kernels look at
    unsigned gen = 0;                // the call's number (never 0)
    int64_t* ambiguous;   // [1]  set by k_track_links when the reference's (magnitude, partial index) order of
                          //      the previous partials would decide an assignment (k_track.hip header)
};
int pvx_launch_track(const TrackParams& p, hipStream_t s);
int pvx_launch_track_sequential(const TrackParams& p, hipStream_t s);   // exact loop on one wave, after a flag

struct SynthParams {
    const double *f, *mag, *realph;   // [F][K]
    const int32_t* partial_id;        // [F][K]
    const int32_t *part_start, *part_len;
    int64_t F, P;
    int K;
    double sr, edge;
    int nfft, hop_a, hop_s, minframes;
    double* w;
    int64_t wlen;
    int no_phcor;         // PVX_SYNTH_NO_PHCOR: fstep=None partials (PV.py:710-713)
    int f32_samples = 0;  // PVX_SYNTH_F32 (plans at precision 32): the bodies' sample loop in float32 (k_synth_bodies<R, float>)
    int64_t seg0 = 0;     // first output segment (hop) of this launch ...
    int64_t seg_count = 0;   // ... and how many (0: all from seg0 on)
    // device workspace of pvx_synth_ws_bytes() bytes (nullptr: a grow-only buffer per stream, owned by the library);
    // skip_prepare: the partial-major copy of the analysis arrays is already in `ws` (a later slice of the same waveform)
    void* ws = nullptr;
    size_t ws_bytes = 0;
    unsigned* ws_gen = nullptr;   // with ws: the owner's call counter for it, 0 after every (re)allocation (k_synth.hip: segment flags)
    int skip_prepare = 0;
};
int pvx_launch_synth(const SynthParams& p, hipStream_t s);
size_t pvx_synth_ws_bytes(int64_t F, int K, int64_t P, int nfft, int hop_a, int hop_s, double edge);

// PVHarmonic.run_pv (k_harmonic.hip): f0-guided bin sampling on the spectra of the general path
struct HarmParams {
    const void* spec;     // complex<T> workspace rows of this chunk [nrows+1][ldo]
    int64_t ldo;
    int64_t fr_begin, nfr;    // frames [fr_begin, fr_begin + nfr) of the signal are analysed by this launch
    int64_t ws_off;           // workspace row of frame fr_begin
    int nfft, hop, N2, K;
    double sr, fstep, dt, fmin;
    const double* wfbin;
    const double* prev0;      // optional [N2][2]: spectrum preceding the first valid frame
    const void* carry;        // complex<T>[N2]: spectrum of the last valid frame of the earlier chunks
    const double* f0;         // [F] fundamental per frame (<= 0 or NaN: frame skipped)
    const int32_t* prevrow;   // [F] workspace row of the previous VALID frame's spectrum; -1: there is
                              // none (zero spectrum or prev0); -2: it is in `carry`
    double *f, *mag, *ph, *residual, *t;
};
int pvx_launch_harmonic(const HarmParams& p, int precision, hipStream_t s);

// windowed reductions with the analysis framing (k_reduce.hip)
struct ReduceParams {
    const double* x;          // [n]
    const double* hetsig;     // [n][2] complex (heterodyne only)
    const double* wind;       // [wlen]
    int64_t nfr;
    int wlen, hop;
    double norm;              // sum(wind) | sum(wind**2)
    double* out;              // [nfr][2] | [nfr]
    int64_t* icent;           // [nfr] optional (heterodyne)
};
int pvx_launch_reduce(const ReduceParams& p, int mode, hipStream_t s);
// FuncWind's named reducers (func: pvx_funcwind_op); x complex128 when cpx (p.x then points at [n][2])
int pvx_launch_funcwind(const ReduceParams& p, int func, bool cpx, hipStream_t s);

// harmonic heterodyne on one f0 track (k_hetharm.hip, Heterodyne.py:261-542).  Every pointer is device memory.
#define PVX_HH_TILE 2048          // samples per block of the phase scan
#define PVX_HH_GROUP 8            // harmonics a wave of k_hh_extract walks by complex multiplication
#define PVX_HH_MAX_HARM (1 << 20) // first + count: far beyond sr / 2 / f0 of any track, keeps the index arithmetic in int
inline int64_t pvx_hh_tiles(int64_t n) { return (n + PVX_HH_TILE - 1) / PVX_HH_TILE; }
// cyc[t] = fvec[0] + .. + fvec[t] (np.cumsum's indexing), in cycles; tsum: pvx_hh_tiles(n) doubles of workspace
int pvx_launch_hh_phase(const double* fvec, int64_t n, double* cyc, double* tsum, hipStream_t s);
struct HhExtractParams {
    const double* x;          // [n]
    const double* cyc;        // [n] running sum of fvec (pvx_launch_hh_phase)
    const double* wind;       // [wlen]
    int64_t nfr;
    int wlen, hop;
    int first, count;         // harmonics first .. first + count - 1
    int halve_dc;             // column of harmonic 0 is halved (extract_partials, Heterodyne.py:530)
    double norm;              // sum(wind)
    double* ah;               // [nfr][count][2]
    int64_t* icent;           // [nfr] optional
};
int pvx_launch_hh_extract(const HhExtractParams& p, hipStream_t s);
struct HhResynthParams {
    const double* fvec;       // [n] cycles per sample
    const double* cyc;        // [n]
    const double* ah;         // [nfr][nharm_total][2]
    int64_t n, nfr;
    int nharm_total, wlen, hop, first, count, filter;
    double sr, fmin, fmax, ampthr;
    double* amax;             // [count] workspace: max_i |ah[i][h]| (filter only)
    double* y;                // [n]
    double* hf;               // [n][2] optional, count == 1: the interpolated (and filtered) amplitude itself
};
int pvx_launch_hh_resynth(const HhResynthParams& p, hipStream_t s);

// time-domain periodicity (k_period.hip, Periodicity.py:98-236).  Lag ranges lo[r]..hi[r] are the similarity lags a frame
// reads; ns..ne the normaliser slice in the index space of the reference's array (amdf: lag; xcorr: nwind-1+lag).
#define PVX_PERIOD_MAX_NCAND 64
#define PVX_PERIOD_MAX_NWIND 32768
struct PeriodParams {
    const double* x;            // [nsamp] device
    int64_t nsamp;
    const double* wind;         // [nwind] device (filled in by pvx_period_run)
    int nwind;
    const int64_t* idx;         // [nfr] frame centres, device (filled in by pvx_period_run)
    int64_t nfr;
    int amdf, cand_method, mindelay, maxdelay, ncand;
    double threshold, vthresh, fftthresh;
    int lo[2], hi[2];
    int ns, ne;
    double* cand_period;        // [nfr][ncand]
    double* cand_strength;
    int32_t* ncands;            // [nfr]
    int32_t* preferred;         // [nfr]
    // filled in by pvx_period_run
    const double* wnorm = nullptr;
    double* xw_out = nullptr;
    double* scratch = nullptr;
    int* err = nullptr;
};
// p.x and the outputs are device memory; the window and the frame centres are host arrays (copied into a per-device
// workspace the calls share, one at a time)
int pvx_period_run(PeriodParams p, const double* h_wind, const int64_t* h_idx, hipStream_t s);

// YIN f0 tracking (k_yin.hip; include/pvx.h: pvx_yin; YIN.md): the frames x[starts[i] : starts[i] + nwind], lags 1 .. hi + 1.
struct YinParams {
    const double* x;            // [nsamp] device
    int64_t nsamp;
    const int64_t* starts;      // [nfr] frame starts, device (filled in by pvx_yin_run)
    int64_t nfr;
    int nwind, lo, hi;
    double tol, sr;
    double* freq;               // [nfr] device
    double* conf;
    double* tau;                // nullable
    int32_t* flag;              // nullable
    int32_t* pick;              // nullable
    int nblk = 0, nseg = 0, seglen = 0;   // the split of a frame's work (filled in by pvx_yin_run from nwind and hi alone)
};
// p.x and the outputs are device memory, h_starts a host array (the entry point checked every frame against nsamp).
// Synchronises the stream; *kernels names what ran.
int pvx_yin_run(YinParams p, const int64_t* h_starts, hipStream_t s, const char** kernels);

// Period marks (k_marks.hip; include/pvx.h: pvx_marks_corr / pvx_marks_peak; MARKS.md): one walk per row x[row_start : row_stop].
// The row lists and the track are device pointers the run functions fill in from the host lists of MarksRows.
struct MarksRows {
    const int64_t *row_start, *row_stop;   // [nrows], host
    const double *t0, *toff;               // [nrows], host (t0: the corr walk only; toff may be null)
    const double *tf, *f;                  // the shared track, host: ntf knots and nf values (tf null: nf == 1 or nf == nsamp)
    int64_t ntf, nf;
};
struct MarksCorrParams {
    const double* x;            // device
    int64_t nsamp, nrows;
    const int64_t *row_start, *row_stop;
    const double *t0, *toff, *tf, *f;
    int ntf;
    double f_fallback;          // f0 where interp(t0) is NaN (the reference's nanmean(f))
    double sr, min_per;
    int W, cap;                 // window_size; doubles of LDS the stretch may take (>= W + the largest P)
    int max_marks;
    int64_t max_steps;
    double* marks;              // [nrows][max_marks]
    int32_t *count, *status;    // [nrows]
};
struct MarksPeakParams {
    const double* x;
    int64_t nsamp, nrows;
    const int64_t *row_start, *row_stop;
    const double *toff, *tf, *f;
    int ntf, fmode;             // fmode 0: f[0] everywhere; 1: f[row_start + i]; 2: interp(toff + i / sr, tf, f)
    double sr;
    int fit_points, max_marks;
    int64_t max_steps;
    double *marks, *vals;       // [nrows][max_marks]
    int32_t *count, *status;
};
// launch and synchronise the stream; *kernels names what ran
int pvx_marks_corr_run(MarksCorrParams p, const MarksRows& h, hipStream_t s, const char** kernels);
int pvx_marks_peak_run(MarksPeakParams p, const MarksRows& h, hipStream_t s, const char** kernels);

// FFT filter banks (k_fbank.hip, FFTFilters.py:274-292, 352-374): band energies and cepstra of frames 0 .. nfr of the device
// signal d_x (frame i starts at i * hop).  The window, fb [nband][nwind] (full spectrum) are host arrays; d_spec / d_cep device
// memory (either may be null).  Synchronises the stream; *kernels names what ran.
int pvx_fbank_run(const void* d_x, int x_dtype, int64_t nfr, const double* h_wind, int nwind, int hop, const double* h_fb, int nband,
                  int cep_mode, double* d_spec, double* d_cep, hipStream_t s, const char** kernels);

// windowed spectral measures (k_specdesc.hip; include/pvx.h: pvx_specdesc): nfr values (PSD: frames) of the device signal d_x.
// The window and the weights h_a / h_b [nwind/2 + 1] are host arrays, d_out device memory.  PSD: d_out [nwind/2] carries the
// running sum between the calls of one signal: `first` starts it from zero, total > 0 marks the last call and divides by it;
// the calls before the last one take whole blocks of PVX_SPECDESC_BLOCK frames.  Synchronises the stream.
int pvx_specdesc_run(const void* d_x, int x_dtype, int64_t nfr, const double* h_wind, int nwind, int hop, int meas, const double* h_a,
                     const double* h_b, double* d_out, bool first, int64_t total, hipStream_t s, const char** kernels);

// Welch-averaged cross and auto spectra, block by block (k_xspec.hip; include/pvx.h: pvx_xspec): nblk blocks of nseg segments
// of the device signals d_x, d_y (d_y null: the auto spectrum of d_x alone), which point at the first block's first sample.
// The window is a host array, the outputs device memory ([nblk][nwind/2 + 1], d_sxy complex).  Synchronises the stream.
int pvx_xspec_run(const void* d_x, const void* d_y, int x_dtype, const double* h_wind, int nwind, int step, int64_t delta, int64_t nblk,
                  int nseg, double* d_sxy, double* d_sxx, double* d_syy, hipStream_t s, const char** kernels);

// fricative descriptors (k_fric.hip; include/pvx.h: pvx_fricative): nrows snippets d_x[h_starts[r] : + L] of the device signal d_x.
// d_x non-null: the Welch spectra into d_psd [nrows][nper/2 + 1] (nper = min(nwind, L); h_win [nper] nullable: the periodic Hann
// window; d_psd nullable when d_desc is given).  d_desc non-null: the descriptors of the psd rows into d_desc [nrows][7], d_imax,
// d_status (h_freq [nper/2 + 1] a host array) and, with d_x, the snippets' RMS into d_rms.  d_x null: the descriptors of the rows
// of d_psd alone.  Synchronises the stream.
int pvx_fric_run(const void* d_x, int x_dtype, const int64_t* h_starts, int64_t nrows, int L, int nwind, const double* h_win, double sr,
                 const double* h_freq, double* d_psd, double* d_desc, int32_t* d_imax, int32_t* d_status, double* d_rms, hipStream_t s,
                 const char** kernels);

// full cross-correlations and their peaks, block by block (k_xcorr.hip; include/pvx.h: pvx_xcorr_peak): nblk blocks of the device
// signals d_a (la samples a block) and d_v (lv), which point at the first block's first sample.  The windows are host arrays
// (nullable: ones), the outputs device memory (d_corr [nblk][la + lv - 1], nullable).  Synchronises the stream.
// pvx_xcorr_fft_route: whether a call of these lengths takes the fft route; pvx_xcorr_padded: its padded length P, 0 beyond
// PVX_XCORR_MAX_P (la, lv >= 1)
bool pvx_xcorr_fft_route(int la, int lv);
int pvx_xcorr_padded(int la, int lv);
int pvx_xcorr_run(const void* d_a, const void* d_v, int x_dtype, int la, int lv, int64_t delta, int64_t nblk, int detrend, const double* h_win_a,
                  const double* h_win_v, int use_abs, int32_t* d_lag, double* d_peak, double* d_corr, hipStream_t s, const char** kernels);

// glottal inverse filtering and frame-wise LPC (k_iaif.hip; include/pvx.h: pvx_iaif, pvx_lpc).  The tables are host arrays.
struct IaifCall {
    int x_dtype, nwind, hop, ntaps, pt, pg, n_it;
    double leak;
    const double *h_b, *h_hw, *h_ow;   // [ntaps], [nwind], [nwind] (h_ow: only with an overlap-add)
};
// Frames f0 .. f0 + nf - 1 of a signal, d_x pointing at the first sample of frame f0: g, dg into rows 0 .. nf - 1 of d_g / d_dg
// [nf][nwind], the filters into d_vt [nf][pt + 1] and d_gc [nf][(n_it ? pg : 1) + 1] (all four required, device memory).  With
// d_glot or d_dglot: the overlap-add of the signal's samples s0 .. s0 + ns - 1 into their elements 0 .. ns - 1, from these rows
// (which must hold every frame that covers one of the samples).  *singular: the first row whose LPC was singular, or -1.
// Synchronises the stream.
int pvx_iaif_run(const IaifCall& c, const void* d_x, int64_t f0, int64_t nf, double* d_g, double* d_dg, double* d_vt, double* d_gc, int64_t s0,
                 int64_t ns, double* d_glot, double* d_dglot, int64_t* singular, hipStream_t s, const char** kernels);
// coefficient rows of nf frames (frame i at d_x[i * hop]); h_wind may be null.  Synchronises the stream.
int pvx_lpc_run(const void* d_x, int x_dtype, int64_t nf, const double* h_wind, int nwind, int hop, int order, double* d_coef, int64_t* singular,
                hipStream_t s, const char** kernels);

// formant tracking and polynomial roots (k_formant.hip; include/pvx.h: pvx_formants, pvx_polyroots).  The tables are host arrays.
struct FormantCall {
    int x_dtype;
    int64_t n;                         // the length of the whole signal (the zero extension begins there)
    int preemph, down, ntaps, nwind, hop, order;
    double fs;
    const double *h_taps, *h_wind;     // [ntaps] (down > 1 only), [nwind]
};
struct FormantRows {                   // device rows of the group's first frame on; each nullable
    int* nkept;
    double *freq, *bw, *re, *im, *lpc;
};
// Frames f0 .. f0 + nf - 1 of the decimated signal: d_x[i - x0] is sample i of the signal and holds every sample those
// frames' decimated samples read (and one more for the difference); d_y takes the (nf - 1) * hop + nwind decimated samples.
// *singular / *noconv: the first row (from 0) whose LPC was singular / whose roots met the iteration bound, or -1.
// Synchronises the stream.
int pvx_formants_run(const FormantCall& c, const void* d_x, int64_t x0, int64_t f0, int64_t nf, double* d_y, const FormantRows& out,
                     int64_t* singular, int64_t* noconv, hipStream_t s, const char** kernels);
// canonical, ordered roots of n coefficient rows [order + 1]; d_re / d_im / d_nkept / d_status nullable.  Synchronises the stream.
int pvx_polyroots_run(const double* d_coef, int64_t n, int order, double* d_re, double* d_im, int* d_nkept, int* d_status, int64_t* noconv,
                      int64_t* leadzero, hipStream_t s, const char** kernels);

// LPC spectral envelopes and refined peaks (k_lpcenv.hip; include/pvx.h: pvx_lpc_envelope, pvx_peaks_refine).  Every pointer is
// device memory; the outputs are each nullable.  *overflow: the first row (from 0) with more than maxpk peaks, *invalid: the first
// row with a zero leading coefficient / a selected index outside 1 .. npts - 2; -1 otherwise.  Synchronises the stream.
int pvx_lpcenv_run(const double* d_coef, int64_t n, int order, int npts, double fs, int maxpk, double* d_env, int* d_npk, int* d_idx,
                   double* d_pos, double* d_val, int64_t* overflow, int64_t* invalid, hipStream_t s, const char** kernels);
int pvx_peaks_refine_run(const double* d_y, int64_t n, int npts, const double* d_x, int maxpk, const int* d_sel, int* d_npk, int* d_idx,
                         double* d_pos, double* d_val, int64_t* overflow, int64_t* invalid, hipStream_t s, const char** kernels);

// speech segmentation on device band energies (k_segment.hip; include/pvx.h: pvx_seg_detect, pvx_seg_refine, pvx_seg_transitions).
// The small tables (ranges, tseg, tx, trt) are host arrays, staged by the call; all three synchronise the stream.
int pvx_seg_detect_run(const double* d_spec, int64_t nfr, int nband, double thresh, int maxseg, double* d_det, int* d_idx, double* d_fpos,
                       int64_t* count, hipStream_t s, const char** kernels);
int pvx_seg_refine_run(const double* d_spec, int64_t nfine, int nband, const int32_t* h_ranges, const double* h_tseg, int64_t nseg, int hop,
                       double half, double tsr, double sr, double thr, int has_thr, double* d_valb, double* d_vala, int* d_cross,
                       double* d_out, hipStream_t s, const char** kernels);
int pvx_seg_transitions_run(const double* d_v, int64_t nser, int n, int64_t row_stride, int64_t elem_stride, double escale,
                            const double* h_tx, int64_t tx_stride, const double* h_trt, int mode, double pct, double thr, double* d_ttr,
                            double* d_vbef, double* d_vaft, int* d_status, hipStream_t s, const char** kernels);

// pitch jumps on device rows (k_jumps.hip; include/pvx.h: pvx_jump_select, pvx_winstat, pvx_jump_pick).  Every pointer is device
// memory and no output is nullable (d_len may be null: every row holds nmax); all three synchronise the stream.
int pvx_jump_select_run(const double* d_mag, const double* d_f0, const double* d_t, const int* d_len, int64_t rows, int nmax, int K, double thr,
                        double* d_m, int* d_isel, double* d_tsel, double* d_fsel, int* d_nsel, int* d_status, hipStream_t s,
                        const char** kernels);
int pvx_winstat_run(const double* d_t, const double* d_x, const int* d_len, int64_t rows, int nmax, int kind, int wl, int wr, int hop, int flags,
                    double* d_out, hipStream_t s, const char** kernels);
int pvx_jump_pick_run(const double* d_zs, const double* d_t, const double* d_x, const int* d_len, int64_t rows, int nmax, double thr, int nsl,
                      int maxjump, int* d_idx, int* d_dir, int* d_njump, double* d_intcpts, double* d_sumres, int* d_status, hipStream_t s,
                      const char** kernels);

// result wire format for the multi-GPU gather (k_wire.hip)
struct WireParams {
    int64_t rows;                     // frames (all signals of the shard)
    int K, precision;
    int fmt = 1;                      // 1: f as float64 (18 / 26 B per slot); 2 (precision 32): the float32 it is computed from (14 B)
    double fstep;
    double dt = 0.0;                  // fmt 2: hop / sr and the plan's wfbin table (what peak_math computes a frequency from)
    const double* wfbin = nullptr;
    void* wire;
    const double *f, *mag, *ph, *binno, *totalmag;                    // pack: inputs
    double *of, *omag, *oph, *orealph, *obinno, *ototalmag;           // unpack: outputs
};
size_t pvx_wire_block_bytes(int64_t rows, int K, int precision, int fmt = 1);
int pvx_launch_wire(const WireParams& p, bool pack, hipStream_t s);

// frame descriptors and helpers on the result arrays (k_desc.hip)
int pvx_launch_f0(const double* f, const double* mag, int64_t F, int K, double fmin, double fmax, double thr, double* fm,
                  int32_t* im, hipStream_t s);
int pvx_launch_hpower_rows(const double* f, const double* mag, int64_t F, int K, double* rowpow, int32_t* top, hipStream_t s);
int pvx_launch_hpower(const double* f, int64_t F, int K, double f_threshold, const double* rowpow, double* hpower,
                      double* nharm, hipStream_t s);
int pvx_launch_fill_t(double* t, int64_t F, int64_t nsig, int hop, int nfft, double sr, hipStream_t s);
int pvx_launch_spec_to_prev(double* dst, const void* src, int n, int src_is_float, hipStream_t s);

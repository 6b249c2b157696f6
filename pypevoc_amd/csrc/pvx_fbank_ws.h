// pvx_fbank_ws.h -- host only: the per-device workspace that the FFT filter banks (k_fbank.hip) and the windowed spectral
// measures (k_specdesc.hip) share: the tables of the call, the rows route's buffers and its rocFFT plans.  Kept for the
// process, grow-only, held for a whole call (execution and the final synchronisation included): callers on one device take
// turns, whichever of the two families they belong to.  Defined in k_fbank.hip.
#pragma once
#include <map>
#include <mutex>
#include <vector>

#include "pvx_internal.h"
#include "pvx_mem.h"

struct FftPlan {
    RealFft fft;
    int64_t batch = 0;
};
struct FbankWs {
    std::mutex mu;
    std::vector<double> h_tab;                                        // host image of `tab` (alive until the call's copy is done)
    std::vector<int> h_band;
    DevMem tab, band, frames, spec;                                   // (exactly as large as the largest request so far)
    DevMem work;                                                      // the one rocFFT work buffer the plans share
    DevMem part;                                                      // k_specdesc.hip: the periodogram's block partials
    std::map<int, FftPlan> plans;                                     // nwind -> plan of the rows route
};

// the workspace of the current device (created on first use, never erased); the caller locks ws->mu for its call
int pvx_fbank_workspace(FbankWs** ws);
// the rows route's plan for nwind: pvx_fbank_rows_batch(nwind) transforms of nwind reals into nwind/2 + 1 complex values each
int pvx_fbank_ensure_plan(FbankWs& w, int nwind, FftPlan** out);

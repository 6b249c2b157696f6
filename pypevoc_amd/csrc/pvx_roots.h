// pvx_roots.h -- the roots of one real polynomial per wave, in float64 (np.roots' place in pypevoc/speech/SpeechAnalysis.py:
// lpc2form :186-209 and glottal.py: lpcc2pole :249-272), for kernels that hold the coefficients in LDS (k_formant.hip).
// Device only; design, the canonical-root rule and the bounds: FORMANTS.md.
//
//   wave_roots   c[0] z^p + c[1] z^(p-1) + ... + c[p], c[0] != 0, p <= PVX_ROOTS_MAX_ORDER: one lane per root
//
// Aberth-Ehrlich: lane i holds the iterate z_i, runs Horner for p(z_i), p'(z_i) and the bound sum |c_k| |z_i|^(p-k), reads
// the other iterates through __shfl in index order for sum_j 1 / (z_i - z_j), and steps by w / (1 - w sum), w = p / p'.  A
// lane stops where |p(z_i)| <= q 2^-53 sum |c_k| |z_i|^(q-k) (half of Horner's own rounding bound) or where its step no
// longer moves z_i; the wave stops when every lane has (a vote), and after kMaxIter iterations whatever the lanes say: the
// loop is bounded at compile time, a polynomial that reaches the bound gets the status kNoConv and returns.  Trailing
// coefficients that are exactly 0 are exact zero roots, taken out before the iteration.  Nothing here depends on the grid
// or on another wave: the roots' bits are a function of the coefficients alone.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "pvx.h"

namespace pvxroots {

constexpr int kMaxIter = 200;                                        // the vowels of the fixtures need 12, degree 64 below 60
constexpr int kOk = 0, kNoConv = 2, kLeadZero = 3;                   // (1 is a singular frame's: k_formant.hip)
static_assert(PVX_ROOTS_MAX_ORDER <= 64, "wave_roots holds one root per lane");

__device__ __forceinline__ void lds_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// All 64 lanes of a wave call this with the same c (LDS, visible to the wave) and p >= 1.  sre / sim [p] (LDS) receive the
// roots in canonical form and order: a real root has imaginary part +0.0, complex roots are exact conjugate pairs; first
// the *nkept roots with imag >= 0 by ascending atan2(im, re), equal angles by ascending |z|, then the conjugates with
// imag < 0 in their partners' order.  Returns kOk or kNoConv (wave-uniform); the arrays are visible to the wave afterwards.
__device__ inline int wave_roots(const double* c, int p, double* sre, double* sim, int* nkept) {
    const int lane = threadIdx.x & 63;
    int q = p;
    while (q > 0 && c[q] == 0.0) q--;                                // (wave-uniform) the polynomial that is iterated has degree q
    double zr = 0.0, zi = 0.0;
    bool all_done = true;
    if (q > 0) {
        // start: a circle whose radius is the geometric mean of the roots' moduli, turned off the real axis so that no
        // two starting points are mirror images (real arithmetic would keep such a pair a pair for ever)
        const double rad = exp(log(fabs(c[q] / c[0])) / (double)q);
        double sn, cs;
        sincos((6.283185307179586 * (double)lane + 0.7) / (double)q, &sn, &cs);
        zr = rad * cs;
        zi = rad * sn;
        bool done = lane >= q;
        const double tol = (double)q * 0x1p-53;
        all_done = false;
        for (int it = 0; it < kMaxIter; it++) {
            double pr = c[0], pi = 0.0, dr = 0.0, di = 0.0, s = fabs(c[0]);
            const double az = hypot(zr, zi);
            for (int k = 1; k <= q; k++) {
                const double ndr = fma(dr, zr, fma(-di, zi, pr)), ndi = fma(dr, zi, fma(di, zr, pi));
                const double npr = fma(pr, zr, fma(-pi, zi, c[k])), npi = fma(pr, zi, pi * zr);
                dr = ndr; di = ndi; pr = npr; pi = npi;
                s = fma(s, az, fabs(c[k]));
            }
            double sr = 0.0, si = 0.0;                               // sum over j != i of 1 / (z_i - z_j), j ascending
            for (int j = 0; j < q; j++) {
                const double dx = zr - __shfl(zr, j), dy = zi - __shfl(zi, j);
                const double m = dx * dx + dy * dy;
                if (j != lane && m > 0.0) { sr += dx / m; si -= dy / m; }
            }
            if (!done) {
                if (hypot(pr, pi) <= tol * s) {
                    done = true;
                } else {
                    const double dm = dr * dr + di * di;
                    const double wr = (pr * dr + pi * di) / dm, wi = (pi * dr - pr * di) / dm;    // w = p / p'
                    const double er = 1.0 - (wr * sr - wi * si), ei = -(wr * si + wi * sr);       // 1 - w sum
                    const double em = er * er + ei * ei;
                    const double sx = (wr * er + wi * ei) / em, sy = (wi * er - wr * ei) / em;    // the step
                    zr -= sx;
                    zi -= sy;
                    if (hypot(sx, sy) <= 0x1p-52 * hypot(zr, zi)) done = true;
                }
            }
            if (__all(done)) { all_done = true; break; }
        }
    }
    // canonical form: every iterate looks for the iterate nearest its conjugate (itself included; the lowest index among
    // equals).  One that finds itself is real.  Two that find each other are a pair: the member with the larger imaginary
    // part gives both their real part and the size of the imaginary one.  One whose choice is not returned looks again
    // among those still without a partner, in the next round (wave-uniform votes; the nearest two of a round always find each
    // other, so a round settles some, and the rounds are bounded as the iteration is: whatever is left then is real).  A
    // pair's members are an iterate and its mirror image, whose residuals are the same number.
    bool open = lane < q;
    for (int round = 0; round < PVX_ROOTS_MAX_ORDER && __any(open); round++) {
        int best = lane;
        double bd = INFINITY;
        for (int j = 0; j < q; j++) {
            const double dx = zr - __shfl(zr, j), dy = -zi - __shfl(zi, j);
            const double m = dx * dx + dy * dy;
            const int oj = __shfl((int)open, j);
            if (open && oj && m < bd) { bd = m; best = j; }
        }
        const int back = __shfl(best, best);
        const double or_ = __shfl(zr, best), oi = __shfl(zi, best);
        if (open && best == lane) {
            zi = 0.0;
            open = false;
        } else if (open && back == lane) {
            const bool mine = zi > oi || (zi == oi && lane < best);
            const double mi = fabs(mine ? zi : oi);
            zr = mine ? zr : or_;
            zi = mi == 0.0 ? 0.0 : (mine ? mi : -mi);
            open = false;
        }
    }
    if (open) zi = 0.0;
    if (lane >= q) {
        zr = 0.0;                                                    // lanes q .. p - 1: the exact zero roots
        zi = 0.0;
    }
    // order: a rank count across the lanes, per class (0 kept, 1 dropped conjugate, 2 no root)
    const int cls = lane >= p ? 2 : (zi >= 0.0 ? 0 : 1);
    const double ang = atan2(fabs(zi), zr), mag = hypot(zr, zi);
    int rank = 0;
    for (int j = 0; j < p; j++) {
        const double aj = __shfl(ang, j), mj = __shfl(mag, j);
        const int cj = __shfl(cls, j);
        if (cj == cls && (aj < ang || (aj == ang && (mj < mag || (mj == mag && j < lane))))) rank++;
    }
    const int nk = __popcll(__ballot(cls == 0));
    if (cls < 2) {
        const int pos = cls == 0 ? rank : nk + rank;
        sre[pos] = zr;
        sim[pos] = zi;
    }
    lds_sync();
    *nkept = nk;
    return all_done ? kOk : kNoConv;
}

}  // namespace pvxroots

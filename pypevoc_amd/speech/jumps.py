"""pypevoc/speech/PitchJumps.py on the GPU: the windowed statistics zscore_wind :50-64, linreg_err :67-84 and linreg2_err
:87-121, JumpDetector :140-270 and segment_and_detect_jumps :273-290.

The pitch track comes from the mirror's PV (run_pv, calc_f0) and stays on its resident chain: the frame magnitudes and the
selection by magnitude are taken where the (F, K) array is (pvx_jump_select_resident), the windowed two-sided regression
t-test, the strict-extremum pick and the per-jump line fits are kernels of k_jumps.hip (pvx_winstat, pvx_jump_pick;
JUMPS.md).  jumps_rows is the batched form on host or device rows.  Nothing per frame or per jump happens in Python and
there is no CPU fallback.

Deviations from the reference (JUMPS.md has the list): the lines are the centred closed form, not np.polyfit's SVD; window
sides are 3 .. 256 points and a negative wright is refused; a NaN in a track gives NaN outputs and a status bit where
np.polyfit raises; a jump with fewer than two points on a side gives NaN and a status bit where the reference raises;
segment_and_detect_jumps joins the regions' tables with pandas.concat (the reference's DataFrame.append is gone from
pandas 2)."""
import ctypes
import sys

import numpy as np

from .. import _lib
from ..PVAnalysis import PV

JUMP_MAX_SIDE = 256                                                   # PVX_JUMP_MAX_SIDE of include/pvx.h
JUMP_MAX_K = 4096                                                     # PVX_JUMP_MAX_K
WIN_ZMEAN, WIN_ZMEDIAN, WIN_LINREG, WIN_LINREG2 = 0, 1, 2, 3          # pvx_win_kind
WIN_USE_L, WIN_USE_R = 1, 2
JUMP_SHORT_SIDE, JUMP_NAN = 1, 2                                      # status bits


def last_kernels():
    """The kernel the calling thread's last jump stage ran: 'k_jump_select', 'k_winstat', 'k_jump_pick' ('' when it
    launched nothing)."""
    return _lib.load().pvx_jumps_last_kernels().decode()


def _check(rc, what):
    if rc == _lib.PVX_ERR_UNSUPPORTED:
        raise NotImplementedError("%s: %s" % (what, (_lib.load().pvx_last_error() or b"").decode()))
    if rc == _lib.PVX_ERR_INVALID:
        raise ValueError("%s: %s" % (what, (_lib.load().pvx_last_error() or b"").decode()))
    return _lib.check(rc, what)


def _i32p(a):
    return a.ctypes.data_as(_lib.c_int32_p)


def nextpow2(x):
    return int(2**np.ceil(np.log2(x)))


def _check_sides(what, kind, wleft, wright):
    """The limits of pvx_winstat, answered before anything is staged."""
    right_ok = 3 <= wright <= JUMP_MAX_SIDE or (wright == 0 and kind != WIN_LINREG2)
    if not (3 <= wleft <= JUMP_MAX_SIDE) or not right_ok:
        raise NotImplementedError("%s: window sides %d and %d: the kernel takes 3 .. %d points a side (PVX_JUMP_MAX_SIDE; wright 0 "
                                  "for the kinds other than linreg2_err; the reference's negative-wright branch is not mirrored)"
                                  % (what, wleft, wright, JUMP_MAX_SIDE))


def _winstat_row(t, x, kind, wleft, wright, hop, flags, what):
    """One row of pvx_winstat on host arrays."""
    hop = 1 if hop is None else int(hop)
    wleft, wright = int(wleft), int(wright)
    _check_sides(what, kind, wleft, wright)
    if hop < 1:
        raise ValueError("%s: hop must be at least 1" % what)
    x = np.ascontiguousarray(x, dtype=np.float64)
    t = x if t is None else np.ascontiguousarray(t, dtype=np.float64)
    if x.ndim != 1 or t.shape != x.shape:
        raise ValueError("%s: t and x must be 1-D arrays of one length" % what)
    n = len(x)
    out = np.zeros(n)
    if n == 0:
        return out
    _lib.init()
    _check(_lib.load().pvx_winstat(_lib.dptr(t), _lib.dptr(x), None, 1, n, kind, wleft, wright, hop, flags, _lib.dptr(out)), "pvx_winstat")
    return out


def zscore_wind(x, wleft=5, wright=5, hop=None, kind='mean'):
    """(x[i] - centre) / spread over x[i - wleft : i + wright] for i = wleft, wleft + hop, .. < len(x) - wright, 0 elsewhere
    (:50-64): kind 'mean' the mean and np.std, 'median' the median and the interquartile range."""
    if kind not in ('mean', 'median'):
        raise ValueError("kind %r: 'mean' or 'median' are known" % (kind,))    # (the reference: UnboundLocalError)
    return _winstat_row(None, x, WIN_ZMEAN if kind == 'mean' else WIN_ZMEDIAN, wleft, wright, hop, 0, "zscore_wind")


def linreg_err(t, x, wleft=5, wright=5, hop=None):
    """The distance of x[i] from the least-squares line over the window, in standard deviations of the window's
    residuals (:67-84)."""
    return _winstat_row(t, x, WIN_LINREG, wleft, wright, hop, 0, "linreg_err")


def linreg2_err(t, x, wleft=5, wright=5, hop=None, use_l=True, use_r=True):
    """The two-sample t of the residuals of the wleft points before i against those of the wright points from i on, about
    the left side's line (use_l) and, negated and the sides swapped, about the right side's (use_r); their mean (:87-121)."""
    flags = (WIN_USE_L if use_l > 0 else 0) | (WIN_USE_R if use_r > 0 else 0)
    return _winstat_row(t, x, WIN_LINREG2, wleft, wright, hop, flags, "linreg2_err")


def _not_mirrored(name, where):
    def stub(*args, **kwargs):
        raise NotImplementedError("%s (pypevoc/speech/PitchJumps.py:%s) is not mirrored: see INTEGRATION.md" % (name, where))
    stub.__name__ = name
    return stub


avg_interpolator = _not_mirrored("avg_interpolator", "124-137")
file_reader = _not_mirrored("file_reader", "292-302")
pitch_jump_file = _not_mirrored("pitch_jump_file", "305-309")


def _maxjump(n):
    return max(int(n) - 2, 0)                                         # the strict interior extrema of n points: no overflow


def _split(idx, dirs, count):
    idx, dirs = idx[:count].astype(np.intp), dirs[:count]
    return idx[dirs > 0], idx[dirs < 0]


class JumpDetector(object):
    """The register breaks of a voice (:140-270): a pitch track from the phase vocoder, and the frames where the track's
    linear trend before a frame and after it disagree.

    min_freq: the lowest pitch looked for, Hz (it sets the transform's length).  pitch_t_hop: seconds between two pitch
    values.  regressor_t: seconds of track on either side of a frame that the t-test's lines are fitted to; slope_t, the
    same for the per-jump fits of calc_jump_params, starts equal to it and is an attribute of its own.  t_threshold: how
    large the t-value's extremum has to be for a jump.  mag_threshold: a frame takes part when its magnitude exceeds this
    share of the loudest frame's."""

    def __init__(self, min_freq=70, pitch_t_hop=0.02, regressor_t=0.5, t_threshold=10, mag_threshold=0.01):
        self.min_freq, self.pitch_t_hop = min_freq, pitch_t_hop
        self.regressor_t = self.slope_t = regressor_t
        self.t_threshold, self.mag_threshold = t_threshold, mag_threshold
        self._selected = None
        self._picked = None

    def detect_pitch(self, w, sr):
        """The pitch track of w (:167-176): PV at nfft = nextpow2(2 sr / min_freq), hop = nextpow2(sr pitch_t_hop), its
        calc_f0, and per frame the magnitude sqrt(sum(mag^2)).  A host signal stays on PV's resident chain: f0, t and the
        magnitudes -- F-sized arrays -- are all that comes back.  ValueError when w gives no frame (the reference: numpy's
        AxisError, a subclass)."""
        nfft = nextpow2(sr / self.min_freq * 2)
        n_hop = nextpow2(sr * self.pitch_t_hop)
        pv = PV(w, sr, nfft=nfft, hop=n_hop, progress=False)
        pv.run_pv()
        F = pv.nframes
        if F == 0:
            raise ValueError("detect_pitch: no frame: the signal is not longer than the window (%d samples)" % nfft)
        f0 = np.ascontiguousarray(pv.calc_f0(), dtype=np.float64)
        thr = float(self.mag_threshold)
        m, tsel, fsel = np.empty(F), np.empty(F), np.empty(F)
        isel, nsel, status = np.empty(F, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
        lib = _lib.load()
        if pv._on_device():
            _check(lib.pvx_jump_select_resident(pv._plan.handle, _lib.dptr(f0), thr, _lib.dptr(m), _i32p(isel), _lib.dptr(tsel),
                                                _lib.dptr(fsel), _i32p(nsel), _i32p(status)), "pvx_jump_select_resident")
            t = np.asarray(pv.t)
        else:                                                         # (a signal in GPU memory: PV's results are host arrays)
            mag = np.ascontiguousarray(pv.mag, dtype=np.float64)
            t = np.ascontiguousarray(pv.t, dtype=np.float64)
            _check(lib.pvx_jump_select(_lib.dptr(mag), _lib.dptr(f0), _lib.dptr(t), None, 1, F, mag.shape[1], thr, _lib.dptr(m), _i32p(isel),
                                       _lib.dptr(tsel), _lib.dptr(fsel), _i32p(nsel), _i32p(status)), "pvx_jump_select")
        self._kernels = last_kernels()
        self.mag = m
        self.t = t
        self.f0 = f0
        self.nfft = nfft
        self.nhop = n_hop
        # what the selection gave, for detect_jumps -- as long as nobody replaces the arrays or the threshold
        self._selected = (m, t, f0, thr, isel.astype(bool), tsel[:nsel[0]].copy(), fsel[:nsel[0]].copy(), int(status[0]))

    def _select(self):
        """(isel, tsel, fsel, status) of the current mag, t, f0 and mag_threshold (:180-182)."""
        s = self._selected
        thr = float(self.mag_threshold)
        if s is not None and s[0] is self.mag and s[1] is self.t and s[2] is self.f0 and s[3] == thr:
            return s[4], s[5], s[6], s[7]
        # arrays set by hand: the same kernel on the magnitudes as one peak per frame (sqrt(m m) = m)
        m = np.ascontiguousarray(self.mag, dtype=np.float64)
        t = np.ascontiguousarray(self.t, dtype=np.float64)
        f0 = np.ascontiguousarray(self.f0, dtype=np.float64)
        if m.ndim != 1 or t.shape != m.shape or f0.shape != m.shape:
            raise ValueError("mag, t and f0 must be 1-D arrays of one length")
        F = len(m)
        isel = np.zeros(F, dtype=np.int32)
        if F == 0:
            raise ValueError("detect_jumps: an empty track")          # (the reference: np.max of an empty array)
        mo, tsel, fsel = np.empty(F), np.empty(F), np.empty(F)
        nsel, status = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
        _lib.init()
        _check(_lib.load().pvx_jump_select(_lib.dptr(m), _lib.dptr(f0), _lib.dptr(t), None, 1, F, 1, thr, _lib.dptr(mo), _i32p(isel),
                                           _lib.dptr(tsel), _lib.dptr(fsel), _i32p(nsel), _i32p(status)), "pvx_jump_select")
        return isel.astype(bool), tsel[:nsel[0]].copy(), fsel[:nsel[0]].copy(), int(status[0])

    def detect_jumps(self):
        """The jumps of the selected track (:178-207): the frames louder than mag_threshold times the loudest, the
        two-sided regression t-test over int(regressor_t / pitch_t_hop) frames a side, and its strict maxima above
        t_threshold (up) and strict minima below -t_threshold (down)."""
        wle = int(self.regressor_t / self.pitch_t_hop)
        isel, tsel, fsel, status = self._select()
        self.isel = isel
        self.status = status
        le = linreg2_err(tsel, fsel, wleft=wle, wright=wle, use_l=True)
        self.le = le
        n = len(le)
        maxjump = _maxjump(n)
        slots = max(maxjump, 1)
        idx, dirs, st = (np.zeros(slots, dtype=np.int32) for _ in range(3))
        njump = np.zeros(1, dtype=np.int32)
        intcpts, sumres = np.empty((slots, 2)), np.empty((slots, 2))
        nsl = max(int(self.slope_t / self.pitch_t_hop), 1)
        if n > 0:
            _check(_lib.load().pvx_jump_pick(_lib.dptr(le), _lib.dptr(tsel), _lib.dptr(fsel), None, 1, n, float(self.t_threshold), nsl, maxjump,
                                             _i32p(idx), _i32p(dirs), _i32p(njump), _lib.dptr(intcpts), _lib.dptr(sumres), _i32p(st), None),
                   "pvx_jump_pick")
        ijup, ijdn = _split(idx, dirs, int(njump[0]))
        self.down_jump_indices = ijdn
        self.up_jump_indices = ijup
        self.down_jump_times = tsel[ijdn]
        self.up_jump_times = tsel[ijup]
        # the launch fitted the jumps' lines too: calc_jump_params takes them while nothing they depend on has changed
        c = int(njump[0])
        self._picked = (self.isel, self.t, self.f0, nsl, idx[:c].copy(), intcpts[:c].copy(), sumres[:c].copy(), st[:c].copy())

    def calc_jump_params(self):
        """Per jump, in ascending order, the pitch just before and just after it -- the lines through up to
        int(slope_t / pitch_t_hop) selected frames on either side, evaluated at the jump: intcpts [jumps][2] -- and the
        sides' residues: sumres [jumps][2] (:209-242).  jump_status [jumps] has JUMP_SHORT_SIDE where a side holds fewer
        than two frames (NaN; the reference raises) and JUMP_NAN where a value is NaN otherwise."""
        tsel = np.ascontiguousarray(np.asarray(self.t)[self.isel], dtype=np.float64)
        fsel = np.ascontiguousarray(np.asarray(self.f0)[self.isel], dtype=np.float64)
        nsl = int(self.slope_t / self.pitch_t_hop)
        if nsl < 1:
            raise ValueError("calc_jump_params: slope_t is shorter than one pitch hop")
        alli = np.sort(np.concatenate((self.up_jump_indices, self.down_jump_indices))).astype(np.int32)
        nj, n = len(alli), len(tsel)
        if nj == 0:
            self.intcpts, self.sumres, self.jump_status = np.array([]), np.array([]), np.zeros(0, dtype=np.int32)
            return
        p = self._picked
        if p is not None and p[0] is self.isel and p[1] is self.t and p[2] is self.f0 and p[3] == nsl and np.array_equal(p[4], alli):
            self.intcpts, self.sumres, self.jump_status = p[5].copy(), p[6].copy(), p[7].copy()
            return
        if alli.min() < 0 or alli.max() >= n:
            raise IndexError("calc_jump_params: a jump index outside the %d selected frames" % n)
        intcpts, sumres = np.empty((nj, 2)), np.empty((nj, 2))
        status, njump = np.zeros(nj, dtype=np.int32), np.array([nj], dtype=np.int32)
        _lib.init()
        _check(_lib.load().pvx_jump_pick(None, _lib.dptr(tsel), _lib.dptr(fsel), None, 1, n, 0.0, nsl, nj, _i32p(alli), None, _i32p(njump),
                                         _lib.dptr(intcpts), _lib.dptr(sumres), _i32p(status), None), "pvx_jump_pick")
        self.intcpts = intcpts
        self.sumres = sumres
        self.jump_status = status

    def process(self, w, sr):
        """detect_pitch, detect_jumps and calc_jump_params of the signal w at sr Hz in one call (:247-255).  Returns the
        times of all jumps, up and down, ascending."""
        self.detect_pitch(w, sr)
        self.detect_jumps()
        self.calc_jump_params()
        return self._jump_times()

    def _jump_times(self):
        return np.sort(np.concatenate([self.up_jump_times, self.down_jump_times]))

    def jump_table_columns(self):
        """The columns of get_jump_table as a dict of arrays (:258-268).  IndexError without a jump, as in the reference
        (intcpts is then an empty 1-D array)."""
        return _table_columns(self._jump_times(), self.intcpts, self.sumres)

    def get_jump_table(self):
        import pandas
        return pandas.DataFrame(self.jump_table_columns())


def _table_columns(times, intcpts, sumres):
    """One table row per jump: its time, the lines' pitch just before and after it, their midpoint and step, and the two
    sides' residues with their sum.  The names and their order are the reference's (:261-268)."""
    before, after = intcpts[:, 0], intcpts[:, 1]
    res_before, res_after = sumres[:, 0], sumres[:, 1]
    return dict(segment_time=times, f_before=before, f_after=after, f_cent=(before + after) / 2, df=after - before,
                residue_before=res_before, residue_after=res_after, residue_total=res_before + res_after)


def jumps_rows(t, f0, mag, lengths=None, pitch_t_hop=0.02, regressor_t=0.5, t_threshold=10, mag_threshold=0.01, slope_t=None):
    """detect_jumps and calc_jump_params of every row in three launches, whatever the number of rows.

    t, f0: [rows][nmax] frame times and pitch tracks; mag: [rows][nmax][K] peak magnitudes (or [rows][nmax]: the frames'
    magnitudes themselves); lengths: the rows' frame counts (None: nmax each; 0 is legal).  Host arrays, or float64 torch
    tensors on the GPU (lengths then an int32 tensor or a host sequence), which are read in place.  The detector's
    arguments are JumpDetector's; slope_t None: regressor_t.  Returns a dict: 'nsel' [rows], 'isel' [rows][nmax] (bool),
    'le' [rows][nmax] (the t-test series over the selected frames, 0 behind them), per row the lists 'up_jump_indices',
    'down_jump_indices', 'up_jump_times', 'down_jump_times', 'jump_times', 'intcpts' [jumps][2], 'sumres' [jumps][2] and
    'jump_status' [jumps], and 'status' [rows]: the OR of JUMP_NAN from the selection and of the row's jump_status.  A
    row's results are the same bits alone and in any batch."""
    import torch
    wle = int(regressor_t / pitch_t_hop)
    nsl = int((regressor_t if slope_t is None else slope_t) / pitch_t_hop)
    _check_sides("jumps_rows", WIN_LINREG2, wle, wle)
    if nsl < 1:
        raise ValueError("jumps_rows: slope_t is shorter than one pitch hop")
    dev = _lib.bound_torch_device()

    def on_device(a, dtype):
        if isinstance(a, torch.Tensor):
            if a.device != dev or a.dtype != dtype:
                raise ValueError("device rows must be %s tensors on %s" % (dtype, dev))
            return a.contiguous()
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64 if dtype == torch.float64 else np.int32)).to(dev)

    dt, df0, dmag = on_device(t, torch.float64), on_device(f0, torch.float64), on_device(mag, torch.float64)
    if dt.dim() != 2 or df0.shape != dt.shape or dmag.dim() not in (2, 3) or tuple(dmag.shape[:2]) != tuple(dt.shape):
        raise ValueError("t, f0 [rows][nmax] and mag [rows][nmax][K] are expected")
    rows, nmax = int(dt.shape[0]), int(dt.shape[1])
    K = 1 if dmag.dim() == 2 else int(dmag.shape[2])
    if K > JUMP_MAX_K:
        raise NotImplementedError("jumps_rows: %d peaks per frame: the kernel takes up to %d (PVX_JUMP_MAX_K)" % (K, JUMP_MAX_K))
    if K < 1:
        raise ValueError("jumps_rows: mag without peaks")
    dlen = None
    if lengths is not None:
        dlen = on_device(lengths, torch.int32)
        if tuple(dlen.shape) != (rows,):
            raise ValueError("lengths must be [rows]")
        hl = dlen.cpu().numpy()
        if len(hl) and (hl.min() < 0 or hl.max() > nmax):
            raise ValueError("lengths must lie in 0 .. nmax")
    empty = {'nsel': np.zeros(rows, dtype=np.int32), 'isel': np.zeros((rows, nmax), dtype=bool), 'le': np.zeros((rows, nmax)),
             'status': np.zeros(rows, dtype=np.int32)}
    for k in ('up_jump_indices', 'down_jump_indices', 'up_jump_times', 'down_jump_times', 'jump_times', 'intcpts', 'sumres', 'jump_status'):
        empty[k] = [np.zeros((0, 2)) if k in ('intcpts', 'sumres') else np.zeros(0, dtype=np.intp if 'indices' in k else
                                                                                 (np.int32 if k == 'jump_status' else np.float64))
                    for _ in range(rows)]
    if rows == 0 or nmax == 0:
        return empty
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def new(shape, dtype):
        return torch.empty(shape, dtype=dtype, device=dev)

    def ptr(a):
        return ctypes.c_void_p(a.data_ptr()) if a is not None else None

    cells = rows * nmax
    dm, dts, dfs, dle = (new(cells, torch.float64) for _ in range(4))
    dis, dns, dss = new(cells, torch.int32), new(rows, torch.int32), new(rows, torch.int32)
    _check(lib.pvx_jump_select_dev(ptr(dmag), ptr(df0), ptr(dt), ptr(dlen), rows, nmax, K, float(mag_threshold), ptr(dm), ptr(dis), ptr(dts),
                                   ptr(dfs), ptr(dns), ptr(dss), stream), "pvx_jump_select_dev")
    kernels = [last_kernels()]
    _check(lib.pvx_winstat_dev(ptr(dts), ptr(dfs), ptr(dns), rows, nmax, WIN_LINREG2, wle, wle, 1, WIN_USE_L | WIN_USE_R, ptr(dle), stream),
           "pvx_winstat_dev")
    kernels.append(last_kernels())
    maxjump = _maxjump(nmax)
    slots = max(rows * maxjump, 1)
    didx, ddir, dst, dnj = new(slots, torch.int32), new(slots, torch.int32), new(slots, torch.int32), new(rows, torch.int32)
    dic, dsr = new(slots * 2, torch.float64), new(slots * 2, torch.float64)
    _check(lib.pvx_jump_pick_dev(ptr(dle), ptr(dts), ptr(dfs), ptr(dns), rows, nmax, float(t_threshold), nsl, maxjump, ptr(didx), ptr(ddir),
                                 ptr(dnj), ptr(dic), ptr(dsr), ptr(dst), None, stream), "pvx_jump_pick_dev")
    kernels.append(last_kernels())
    out = empty
    out['kernels'] = tuple(kernels)
    out['nsel'] = dns.cpu().numpy()
    out['isel'] = dis.cpu().numpy().reshape(rows, nmax).astype(bool)
    out['le'] = dle.cpu().numpy().reshape(rows, nmax)
    status = dss.cpu().numpy().copy()
    if maxjump > 0:
        nj = dnj.cpu().numpy()
        idx, dirs = didx.cpu().numpy().reshape(rows, maxjump), ddir.cpu().numpy().reshape(rows, maxjump)
        jst = dst.cpu().numpy().reshape(rows, maxjump)
        ic, sr_ = dic.cpu().numpy().reshape(rows, maxjump, 2), dsr.cpu().numpy().reshape(rows, maxjump, 2)
        tsel = dts.cpu().numpy().reshape(rows, nmax)
        for r in range(rows):
            c = int(nj[r])
            if c == 0:
                continue
            up, dn = _split(idx[r], dirs[r], c)
            out['up_jump_indices'][r], out['down_jump_indices'][r] = up, dn
            out['up_jump_times'][r], out['down_jump_times'][r] = tsel[r][up], tsel[r][dn]
            out['jump_times'][r] = tsel[r][idx[r, :c]]
            out['intcpts'][r], out['sumres'][r], out['jump_status'][r] = ic[r, :c].copy(), sr_[r, :c].copy(), jst[r, :c].copy()
            status[r] |= int(np.bitwise_or.reduce(jst[r, :c]))
    out['status'] = status
    return out


def segment_and_detect_jumps(w, sr, **kwargs):
    """The pitch jumps of every sounding region of w (:273-290): SilenceDetector(w, sr, fmin=50, fmax=1000) finds the
    regions, each gets its pitch track (one PV run per region), and the jump stages of all regions run as one batch
    (jumps_rows).  Returns (jump table with rec_time and region_nbr, segments) as pandas frames; a region without a jump
    is reported on stderr and left out, as in the reference.  The regions' tables are joined with pandas.concat: the
    reference's DataFrame.append no longer exists in pandas 2."""
    import pandas
    from .chunker import SilenceDetector
    sc = SilenceDetector(w, sr, fmin=50, fmax=1000)
    jd = JumpDetector(**kwargs)
    tracks = []
    if _lib.is_device_array(w):
        import torch
        w = torch.as_tensor(w)                                        # (sliced below, in place)
    for tst, tend in zip(sc.tst, sc.tend):
        jd.detect_pitch(w[int(tst * sr):int(tend * sr)], sr)
        tracks.append((jd.t, jd.f0, jd.mag))
    frames = []
    if tracks:
        lengths = np.array([len(tr[0]) for tr in tracks], dtype=np.int32)
        rows = np.zeros((3, len(tracks), int(lengths.max())))
        for r, tr in enumerate(tracks):
            for k in range(3):
                rows[k, r, :lengths[r]] = tr[k]
        res = jumps_rows(rows[0], rows[1], rows[2], lengths, pitch_t_hop=jd.pitch_t_hop, regressor_t=jd.regressor_t,
                         t_threshold=jd.t_threshold, mag_threshold=jd.mag_threshold, slope_t=jd.slope_t)
        for ii, (tst, tend) in enumerate(zip(sc.tst, sc.tend)):
            if len(res['jump_times'][ii]) == 0:
                sys.stderr.write("Jump table empty between {:.2f} and {:.2f}\n".format(tst, tend))
                continue
            dfi = pandas.DataFrame(_table_columns(res['jump_times'][ii], res['intcpts'][ii], res['sumres'][ii]))
            dfi['rec_time'] = dfi['segment_time'] + tst
            dfi['region_nbr'] = ii
            frames.append(dfi)
    df = pandas.concat(frames, ignore_index=True) if frames else pandas.DataFrame()
    segments = pandas.DataFrame({'nbr': np.arange(len(sc.tst)), 'start': sc.tst, 'end': sc.tend})
    return df, segments

"""The jump stages' entry points (pvx_jump_select, pvx_winstat, pvx_jump_pick; JUMPS.md) on hand-built rows against
tests/jumps_refs.py, at the smallest shapes where the kernels can go wrong: window sides around a wave's width and at the cap,
row lengths that give no index, one index and a workgroup's four-index seam, ragged batches with an empty row, 65 rows.

Bounds.  Discrete outputs are equal everywhere; the builders assert a margin of 1e-6 on every comparison that decides one,
or build it from exactly representable values.  Continuous outputs, per row and kind: the unit is the larger of the two
float64 restatements' (numpy's summation order, the kernel's butterfly order) greatest relative distance from the
np.longdouble evaluation on that row; the device may be 8 units from the long-double evaluation.  A row whose unit is under
a quarter ulp says nothing and is drawn again."""
import ctypes

import numpy as np
import pytest

from . import jumps_refs as R

pytestmark = pytest.mark.gpu

QUARTER_ULP = 2.0**-54
WORST = {}                                                            # kind -> (worst device distance, largest unit, worst ratio), printed


def lib():
    from pypevoc_amd import _lib as L
    L.init()
    return L, L.load()


def i32p(a):
    from pypevoc_amd import _lib as L
    return a.ctypes.data_as(L.c_int32_p)


def note(kind, err, unit):
    e, u, r = WORST.get(kind, (0.0, 0.0, 0.0))
    WORST[kind] = (max(e, err), max(u, unit), max(r, err / (8 * unit) if unit else 0.0))


def bounded(kind, dev, plain, bfly, ld, what, zeros=False):
    """dev within 8 units of ld; returns False when the row's unit says nothing.  zeros: 0.0 exactly where ld has it (the
    indices of pvx_winstat where nothing is computed)."""
    ld = np.asarray(ld)
    assert np.array_equal(np.isnan(dev), np.isnan(ld.astype(np.float64))), what
    assert not zeros or np.array_equal(dev == 0, ld == 0), what
    unit = max(R.rel_distance(plain, ld), R.rel_distance(bfly, ld))
    if unit < QUARTER_ULP:
        return False
    err = R.rel_distance(dev, ld)
    assert err <= 8 * unit, (what, err, unit)
    note(kind, err, unit)
    return True


# ---- select -------------------------------------------------------------------------------------------------------------
def call_select(mag, f0, t, lens, thr):
    L, l = lib()
    rows, nmax, K = mag.shape
    mag, f0, t = (np.ascontiguousarray(a, dtype=np.float64) for a in (mag, f0, t))
    m, tsel, fsel = np.full((rows, nmax), -1.0), np.full((rows, nmax), -1.0), np.full((rows, nmax), -1.0)
    isel = np.full((rows, nmax), -1, dtype=np.int32)
    nsel, status = np.full(rows, -1, dtype=np.int32), np.full(rows, -1, dtype=np.int32)
    ln = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    rc = l.pvx_jump_select(L.dptr(mag), L.dptr(f0), L.dptr(t), None if ln is None else i32p(ln), rows, nmax, K, thr, L.dptr(m), i32p(isel),
                           L.dptr(tsel), L.dptr(fsel), i32p(nsel), i32p(status))
    assert rc == rows, (rc, l.pvx_last_error())
    assert l.pvx_jumps_last_kernels() == b"k_jump_select"
    return m, isel, tsel, fsel, nsel, status


@pytest.mark.parametrize("K", [1, 7, 8, 9, 20, 129])
def test_select_against_numpy(K):
    rng = np.random.default_rng(100 + K)
    lens = np.array([300, 0, 257, 120, 1], dtype=np.int32)
    rows, nmax = len(lens), 300
    mag = rng.uniform(0.0, 1.0, (rows, nmax, K)) * rng.choice([1e-3, 1.0], (rows, nmax, 1), p=[0.4, 0.6])
    t = np.cumsum(rng.uniform(0.01, 0.03, (rows, nmax)), axis=1)
    f0 = rng.uniform(100., 400., (rows, nmax))
    thr = 0.05
    m, isel, tsel, fsel, nsel, status = call_select(mag, f0, t, lens, thr)
    for r, n in enumerate(lens):
        rm, risel, rts, rfs = R.select(mag[r, :n], f0[r, :n], t[r, :n], thr)
        if n:
            level = rm.max() * thr
            assert (np.abs(rm - level) >= 1e-6 * level).all()            # the builder's margin
            ld = R.select(mag[r, :n], f0[r, :n], t[r, :n], thr, ar=R.LONG)[0]
            assert np.array_equal(m[r, :n], rm), (K, r)                   # numpy's summation order, term for term
            bounded("m", m[r, :n], rm, rm, ld, "m K %d row %d" % (K, r))
        assert not m[r, n:].any() and not isel[r, n:].any()
        assert np.array_equal(isel[r, :n].astype(bool), risel) and nsel[r] == risel.sum(), (K, r)
        c = nsel[r]
        assert np.array_equal(tsel[r, :c], rts) and np.array_equal(fsel[r, :c], rfs), (K, r)
        assert not tsel[r, c:].any() and not fsel[r, c:].any() and status[r] == 0


def test_select_edges():
    # a frame exactly at the threshold (strict >), from exactly representable values: level = 4 * 0.25 = 1
    mag = np.array([[4.0, 1.0, 1.0 + 2.0**-52, 0.5, 2.0, 1.0 - 2.0**-53]])[:, :, None]
    t = np.arange(6.0)[None]
    f0 = 100.0 + t
    m, isel, tsel, fsel, nsel, status = call_select(mag, f0, t, None, 0.25)
    assert np.array_equal(m[0], mag[0, :, 0]) and list(isel[0]) == [1, 0, 1, 0, 1, 0] and nsel[0] == 3
    assert list(tsel[0]) == [0., 2., 4., 0., 0., 0.] and list(fsel[0]) == [100., 102., 104., 0., 0., 0.]
    # an all-zero track selects nothing; one loud frame; a NaN magnitude selects nothing and sets the bit; a NaN in a selected f0
    n = 260
    rows = np.zeros((4, n, 3))
    rows[1] = 1e-6
    rows[1, 257] = 1.0
    rows[2] = 1.0
    rows[2, 5, 1] = np.nan
    rows[3] = 1.0
    t = np.tile(np.arange(n, dtype=np.float64), (4, 1))
    f0 = t + 50.0
    f0[3, 259] = np.nan
    m, isel, tsel, fsel, nsel, status = call_select(rows, f0, t, None, 0.01)
    assert list(nsel) == [0, 1, 0, n] and list(status) == [0, 0, 2, 2]
    assert not isel[0].any() and np.flatnonzero(isel[1]).tolist() == [257] and tsel[1, 0] == 257. and fsel[1, 0] == 307.
    assert np.isnan(m[2, 5]) and not isel[2].any() and np.isnan(fsel[3, 259]) and np.array_equal(tsel[3], t[3])


# ---- winstat ------------------------------------------------------------------------------------------------------------
def call_winstat(t, x, lens, kind, wl, wr, hop, flags):
    L, l = lib()
    rows, nmax = x.shape
    t, x = np.ascontiguousarray(t, dtype=np.float64), np.ascontiguousarray(x, dtype=np.float64)
    out = np.full((rows, nmax), -7.0)
    ln = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    rc = l.pvx_winstat(L.dptr(t), L.dptr(x), None if ln is None else i32p(ln), rows, nmax, kind, wl, wr, hop, flags, L.dptr(out))
    assert rc == rows, (rc, l.pvx_last_error())
    return out


def track(seed, n):
    """A nondegenerate row: jittered times, a line with noise and a step."""
    rng = np.random.default_rng(seed)
    t = np.cumsum(0.02 + 0.002 * rng.random(max(n, 1)))[:n]
    x = 200.0 + 30.0 * t + 0.5 * rng.standard_normal(n)
    x[n // 2:] += 6.0
    return t, x


KINDS = [("zmean", R.ZMEAN, 0), ("zmedian", R.ZMEDIAN, 0), ("linreg", R.LINREG, 0), ("linreg2 l+r", R.LINREG2, 3), ("linreg2 l", R.LINREG2, 1),
         ("linreg2 r", R.LINREG2, 2), ("linreg2 none", R.LINREG2, 0)]


def reference_row(t, x, kind, wl, wr, hop, flags):
    return [R.winstat(t, x, kind, wl, wr, hop, flags, ar=ar) for ar in (R.PLAIN, R.BFLY, R.LONG)]


@pytest.mark.parametrize("w", [3, 25, 31, 32, 33, 256])
def test_winstat_against_the_restatements(w):
    """Row lengths 0, 2w (no index), 2w + 1 (one), 2w + 2, 2w + 4, 2w + 5 (a workgroup's four indices and the one behind them)
    and 513, ragged in one batch with the empty row; hop 1 and 3; every kind and flag set."""
    lens = [0, 2 * w, 2 * w + 1, 2 * w + 2, 2 * w + 4, 2 * w + 5, 513]
    nmax = max(lens) + 2
    for name, kind, flags in KINDS:
        for hop in (1, 3):
            t, x = np.zeros((len(lens), nmax)), np.zeros((len(lens), nmax))
            refs = []
            for r, n in enumerate(lens):
                for seed in range(1000 * w + 40 * r, 1000 * w + 40 * r + 40):        # (a row whose unit says nothing is drawn again,
                    tr, xr = track(seed, n)                                          # and one with a degenerate window: JUMPS.md)
                    if n > 2 * w and R.window_spreads(tr, xr, kind, w, w, hop).min() < 1e-6:
                        continue
                    plain, bfly, ld = reference_row(tr, xr, kind, w, w, hop, flags)
                    unit = max(R.rel_distance(plain, ld), R.rel_distance(bfly, ld))
                    if n <= 2 * w or name == "linreg2 none" or unit >= QUARTER_ULP:
                        break
                else:
                    raise AssertionError("no row without a degenerate window and with a unit of a quarter ulp in 40 draws: %s w %d n %d" % (name, w, n))
                t[r, :n], x[r, :n] = tr, xr
                refs.append((plain, bfly, ld))
            t[:, -2:], x[:, -2:] = np.nan, np.nan                     # the padding is never read
            for r, n in enumerate(lens):
                t[r, n:], x[r, n:] = np.nan, np.nan
            out = call_winstat(t, x, lens, kind, w, w, hop, flags)
            for r, n in enumerate(lens):
                what = "%s w %d hop %d n %d" % (name, w, hop, n)
                assert not out[r, n:].any(), what
                plain, bfly, ld = refs[r]
                computed = np.zeros(n, dtype=bool)
                computed[w:n - w:hop] = True
                assert not out[r, :n][~computed].any(), what
                if name == "linreg2 none":
                    assert np.isnan(out[r, :n][computed]).all(), what
                    continue
                assert np.isfinite(out[r, :n][computed]).all(), what
                said = bounded(name, out[r, :n], plain, bfly, ld, what, zeros=True)
                assert said or n <= 2 * w, what


def test_winstat_asymmetric_sides_and_a_right_side_of_zero():
    t, x = track(7, 140)
    for name, kind, flags in KINDS[:3]:
        for wl, wr, hop in ((5, 0, 1), (40, 0, 3), (7, 30, 1), (256, 0, 1), (64, 3, 200)):
            tt, xx = track(8, 600) if wl == 256 or hop == 200 else (t, x)   # (hop 200: one index per workgroup, three workgroups)
            out = call_winstat(tt[None], xx[None], None, kind, wl, wr, hop, flags)[0]
            assert R.window_spreads(tt, xx, kind, wl, wr, hop).min() >= 1e-6   # no degenerate window (JUMPS.md)
            plain, bfly, ld = reference_row(tt, xx, kind, wl, wr, hop, flags)
            assert bounded(name, out, plain, bfly, ld, "%s %d/%d hop %d" % (name, wl, wr, hop), zeros=True)
    assert R.window_spreads(t, x, R.LINREG2, 9, 21, 2).min() >= 1e-6
    out = call_winstat(t[None], x[None], None, R.LINREG2, 9, 21, 2, 3)[0]
    assert bounded("linreg2 l+r", out, *reference_row(t, x, R.LINREG2, 9, 21, 2, 3), "linreg2 9/21")


def test_winstat_rows_do_not_depend_on_the_batch():
    """One row alone, three ragged rows with an empty one and 65 rows give the same bits per row."""
    w = 32
    lens = np.array([(2 * w + 5, 0, 513, 2 * w + 1, 300)[r % 5] for r in range(65)], dtype=np.int32)
    nmax = 513
    t, x = np.zeros((65, nmax)), np.zeros((65, nmax))
    for r, n in enumerate(lens):
        t[r, :n], x[r, :n] = track(500 + r % 7, n)
    for name, kind, flags in KINDS[:4]:
        big = call_winstat(t, x, lens, kind, w, w, 1, flags)
        three = call_winstat(t[:3], x[:3], lens[:3], kind, w, w, 1, flags)
        assert np.array_equal(big[:3], three), name
        for r in (0, 2, 3, 64):
            n = lens[r]
            alone = call_winstat(t[r:r + 1, :n], x[r:r + 1, :n], None, kind, w, w, 1, flags)
            assert np.array_equal(alone[0], big[r, :n]), (name, r)
        assert np.array_equal(big[0], big[35]), name                  # (the rows repeat with period 35)


def test_winstat_limits_launch_nothing():
    L, l = lib()
    t, x = track(1, 600)
    out = np.empty(600)
    for wl, wr in ((2, 5), (257, 5), (5, 257), (5, -1), (5, 2)):
        for kind in range(4):
            assert l.pvx_winstat(L.dptr(t), L.dptr(x), None, 1, 600, kind, wl, wr, 1, 3, L.dptr(out)) == L.PVX_ERR_UNSUPPORTED
            assert l.pvx_jumps_last_kernels() == b""
    # a row shorter than the window launches nothing and is all zeros
    o = call_winstat(t[None, :50], x[None, :50], None, R.LINREG2, 25, 25, 1, 3)
    assert not o.any() and l.pvx_jumps_last_kernels() == b""


# ---- pick ---------------------------------------------------------------------------------------------------------------
def call_pick(zs, t, x, lens, thr, nsl, maxjump, want_rc=None):
    L, l = lib()
    rows, nmax = zs.shape
    zs, t, x = (np.ascontiguousarray(a, dtype=np.float64) for a in (zs, t, x))
    idx, dirs, st = (np.full((rows, max(maxjump, 1)), -9, dtype=np.int32) for _ in range(3))
    nj = np.full(rows, -9, dtype=np.int32)
    ic, sr = np.full((rows, max(maxjump, 1), 2), -9.0), np.full((rows, max(maxjump, 1), 2), -9.0)
    over = ctypes.c_int64(-5)
    ln = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    rc = l.pvx_jump_pick(L.dptr(zs), L.dptr(t), L.dptr(x), None if ln is None else i32p(ln), rows, nmax, thr, nsl, maxjump, i32p(idx), i32p(dirs),
                         i32p(nj), L.dptr(ic), L.dptr(sr), i32p(st), ctypes.byref(over))
    assert rc == (rows if want_rc is None else want_rc), (rc, l.pvx_last_error())
    return idx, dirs, nj, ic, sr, st, over.value


def check_pick_row(zs, t, x, thr, nsl, got, what):
    idx, dirs, nj, ic, sr, st = got
    ridx, rdirs = R.pick(zs, thr)
    c = len(ridx)
    assert nj == c and np.array_equal(idx[:c], ridx) and np.array_equal(dirs[:c], rdirs), what
    fits = [R.jump_fits(ridx, t, x, nsl, ar=ar) for ar in (R.PLAIN, R.BFLY, R.LONG)]
    assert np.array_equal(st[:c], fits[0][2]), what
    if c:                                                             # (a row whose unit said nothing would have to be drawn again)
        assert bounded("intcpts", ic[:c], fits[0][0], fits[1][0], fits[2][0], what + " intcpts"), what
        assert bounded("sumres", sr[:c], fits[0][1], fits[1][1], fits[2][1], what + " sumres"), what


def test_pick_edges():
    n = 12
    zs = np.zeros((4, n))
    # extrema at 1 and n - 2, a plateau (5, 6), a value equal to the threshold (8), up and down interleaved
    zs[0] = [0, 20, 0, -20, 0, 15, 15, 0, 10, 0, 30, 0]
    # end points that would win and must not; nothing strict inside
    zs[1] = [100, 50, 20, 0, -20, -50, -100, -200, -300, -400, -500, -900]
    # NaN compares false on both sides; -10 is not below -threshold
    zs[2] = [0, np.nan, 30, 0, -10, 0, -10.000001, 0, np.nan, np.nan, 0, 0]
    zs[3] = [0, 11, 0, 11, 0, -11, 0, 0, 0, 0, 0, 0]                  # row 3 holds 7 frames: index 5 is its n - 2
    lens = [n, n, n, 7]
    t, x = np.zeros((4, n)), np.zeros((4, n))
    for r in range(4):
        t[r], x[r] = track(900 + r, n)
    idx, dirs, nj, ic, sr, st, over = call_pick(zs, t, x, lens, 10.0, 4, n - 2)
    assert over == -1
    assert list(idx[0, :3]) == [1, 3, 10] and list(dirs[0, :3]) == [1, -1, 1] and nj[0] == 3
    assert nj[1] == 0 and nj[2] == 1 and idx[2, 0] == 6 and dirs[2, 0] == -1
    assert nj[3] == 3 and list(idx[3, :3]) == [1, 3, 5] and list(dirs[3, :3]) == [1, 1, -1]
    # a side clipped to one point: NaN and the status bit (index 1: one point before; index 10 of 12: one point after)
    assert st[0, 0] == 1 and np.isnan(ic[0, 0, 0]) and np.isnan(sr[0, 0, 0]) and np.isfinite(ic[0, 0, 1]) and np.isfinite(sr[0, 0, 1])
    assert st[0, 1] == 0 and st[0, 2] == 1 and np.isnan(ic[0, 2, 1]) and np.isfinite(ic[0, 2, 0])
    for r in range(4):
        check_pick_row(zs[r, :lens[r]], t[r, :lens[r]], x[r, :lens[r]], 10.0, 4, (idx[r], dirs[r], nj[r], ic[r], sr[r], st[r]), "row %d" % r)


def test_pick_across_a_tile_seam_and_nsl_other_than_the_window():
    n = 600
    rng = np.random.default_rng(31)
    zs = np.zeros((2, n))
    for r in range(2):
        for i in (1, 60, 254, 255, 256, 257, 400, 511, 512, 513, 598):
            zs[r, i] = (20.0 + rng.random()) * (1 if (i + r) % 2 else -1)
    t, x = np.zeros((2, n)), np.zeros((2, n))
    for r in range(2):
        t[r], x[r] = track(950 + r, n)
    for nsl in (25, 4, 300):                                          # (no side of two points: its residue is rounding noise)
        idx, dirs, nj, ic, sr, st, over = call_pick(zs, t, x, [n, 520], 10.0, nsl, n - 2)
        for r, ln in enumerate((n, 520)):
            check_pick_row(zs[r, :ln], t[r, :ln], x[r, :ln], 10.0, nsl, (idx[r], dirs[r], nj[r], ic[r], sr[r], st[r]), "seam row %d nsl %d" % (r, nsl))
    assert nj[0] == 11


def test_pick_overflow_reports_the_full_count():
    L, l = lib()
    n = 40
    zs = np.tile(np.where(np.arange(n) % 2, 20.0, -20.0), (3, 1))
    zs[:, :3] = 0.0                                                   # (the first jump at 3: no side of fewer than three points)
    zs[1] = 0.0
    t, x = track(77, n)
    t, x = np.tile(t, (3, 1)), np.tile(x, (3, 1))
    idx, dirs, nj, ic, sr, st, over = call_pick(zs, t, x, None, 10.0, 5, 5, want_rc=L.PVX_ERR_SIZE)
    assert over == 0 and list(nj) == [36, 0, 36] and list(idx[0]) == [3, 4, 5, 6, 7] and list(dirs[2]) == [1, -1, 1, -1, 1]
    ridx = np.arange(3, 8)
    fits = [R.jump_fits(ridx, t[0], x[0], 5, ar=ar) for ar in (R.PLAIN, R.BFLY, R.LONG)]
    for r in (0, 2):                                                  # the first maxjump jumps are written and fitted
        assert np.array_equal(idx[r], ridx) and np.array_equal(st[r], fits[0][2]) and not st[r].any()
        assert bounded("intcpts", ic[r], fits[0][0], fits[1][0], fits[2][0], "overflow row %d intcpts" % r)
        assert bounded("sumres", sr[r], fits[0][1], fits[1][1], fits[2][1], "overflow row %d sumres" % r)


# ---- the batched detector -----------------------------------------------------------------------------------------------
def detector_rows(rows, nmax, K, seed):
    rng = np.random.default_rng(seed)
    lens = np.array([(nmax, 0, nmax - 37, 60, nmax - 1)[r % 5] for r in range(rows)], dtype=np.int32)
    t, f0, mag = np.zeros((rows, nmax)), np.zeros((rows, nmax)), np.zeros((rows, nmax, K))
    for r, n in enumerate(lens):
        rr = np.random.default_rng(seed + r % 5)
        tt = 0.016 + 0.032 * np.arange(n)
        f = 150.0 * 2.0**(1.2 * tt / max(tt[-1], 1.0) if n else tt) + 0.05 * rr.standard_normal(n)
        for k, at in enumerate((n // 4, n // 2, 3 * n // 4)):
            f[at:] *= (1.12, 0.9, 1.12)[k]
        t[r, :n], f0[r, :n] = tt, f
        mag[r, :n] = rr.uniform(0.05, 0.3, (n, K))
        quiet = rr.random(n) < 0.08
        mag[r, :n][quiet] *= 1e-4
    return t, f0, mag, lens


def check_rows_margins(ref, thr_t, wle):
    """The builder's part: no degenerate window in the selected track, and a margin on every comparison of the pick."""
    if len(ref["tsel"]) > 2 * wle:
        assert R.window_spreads(ref["tsel"], ref["fsel"], R.LINREG2, wle, wle).min() >= 1e-6
    le = ref["le"]
    for i in range(1, len(le) - 1):
        for a, b in ((le[i], le[i - 1]), (le[i], le[i + 1]), (le[i], thr_t), (le[i], -thr_t)):
            assert abs(a - b) >= 1e-6 or (a == 0 and b == 0), (i, a, b)


def test_jumps_rows_against_the_restatement_and_across_batches():
    import torch
    from pypevoc_amd.speech.jumps import jumps_rows
    rows, nmax, K = 65, 187, 20
    t, f0, mag, lens = detector_rows(rows, nmax, K, 4000)
    big = jumps_rows(t, f0, mag, lens)
    assert big["kernels"] == ("k_jump_select", "k_winstat", "k_jump_pick")
    dev = jumps_rows(torch.from_numpy(t).cuda(), torch.from_numpy(f0).cuda(), torch.from_numpy(mag).cuda(), torch.from_numpy(lens).cuda())
    njumps = 0
    for r in range(5):                                                # (the rows repeat with period 5)
        n = lens[r]
        m = np.sqrt(np.sum(mag[r, :n]**2, axis=1))
        if n:
            level = m.max() * 0.01
            assert (np.abs(m - level) >= 1e-6 * level).all()
        ref = R.detect(m, t[r, :n], f0[r, :n])
        ld = R.detect(m, t[r, :n], f0[r, :n], ar=R.LONG)
        bf = R.detect(m, t[r, :n], f0[r, :n], ar=R.BFLY)
        check_rows_margins(ref, 10, 25)
        c = int(ref["isel"].sum())
        what = "row %d" % r
        assert big["nsel"][r] == c and np.array_equal(big["isel"][r, :n], ref["isel"]) and not big["isel"][r, n:].any(), what
        assert np.array_equal(big["up_jump_indices"][r], ref["up_idx"]) and np.array_equal(big["down_jump_indices"][r], ref["dn_idx"]), what
        assert np.array_equal(big["jump_times"][r], ref["tsel"][ref["idx"]]) and big["status"][r] == 0, what
        if c > 50:
            assert bounded("le (rows)", big["le"][r, :c], ref["le"], bf["le"], ld["le"], what + " le", zeros=True)
        assert not big["le"][r, c:].any()
        if len(ref["idx"]):
            assert bounded("intcpts", big["intcpts"][r], ref["intcpts"], bf["intcpts"], ld["intcpts"], what + " intcpts"), what
            assert bounded("sumres", big["sumres"][r], ref["sumres"], bf["sumres"], ld["sumres"], what + " sumres"), what
        njumps += len(ref["idx"])
    assert njumps >= 6
    keys = ("nsel", "isel", "le", "status")
    lists = ("up_jump_indices", "down_jump_indices", "jump_times", "intcpts", "sumres", "jump_status")
    for k in keys:
        assert np.array_equal(big[k], dev[k]), k                      # host rows and device rows: the same bits
    for r in (0, 1, 2, 3, 4, 64):
        n = lens[r]
        alone = jumps_rows(t[r:r + 1, :max(n, 1)], f0[r:r + 1, :max(n, 1)], mag[r:r + 1, :max(n, 1)], lens[r:r + 1])
        assert alone["nsel"][0] == big["nsel"][r] and np.array_equal(alone["le"][0, :n], big["le"][r, :n]), r
        for k in lists:
            assert np.array_equal(alone[k][0], big[k][r]) and np.array_equal(dev[k][r], big[k][r]), (k, r)
        assert np.array_equal(big["le"][r], big["le"][r % 5]) and np.array_equal(big["intcpts"][r], big["intcpts"][r % 5])


def test_measured_errors_are_printed():
    """(runs last in this file: the worst device distances beside the units, for JUMPS.md's table)"""
    for k, (e, u, r) in sorted(WORST.items()):
        print("%-14s worst distance %.2e  largest unit %.2e  worst distance / (8 units) %.3f" % (k, e, u, r))
    assert WORST

"""Pins tests/synth_refs.py before it judges k_synth.hip (tests/test_synth_diff_gpu.py): the plain restatement against the
reference's recorded waveforms and against the oracle, the float64 round-off of every case against a 64-bit-mantissa run of
the same statements, the amplitude scale, and the branches of pvx_launch_synth that the cases are meant to reach."""
import numpy as np
import pytest

from . import synth_refs as R
from .conftest import load_golden

CASES = R.cases()
NAMES = [c.name for c in CASES]
_memo = {}


def _oracle(oracle, c):
    if c.name not in _memo:
        w = oracle.synth(*R.args(c))
        w.setflags(write=False)
        _memo[c.name] = w
    return _memo[c.name]


def test_matches_the_recorded_parameter_waveforms(oracle):
    """Fixture S1 (edge 0 .. 2, minframes 1 .. 6, synthesis hops 128 / 256 / 300): all seven waveforms of the reference."""
    g = load_golden("S1_synth_params")
    pid, st, ln = oracle.track(g["f"], g["mag"])
    n = 0
    for k in g:
        if k.startswith("w_") and not k.startswith("w_hop"):
            h, e100, mf = (int(v) for v in k[2:].split("_"))
            w = R.synth(g["f"], g["mag"], g["realph"], pid, st, ln, g["sr"], g["nfft"], g["hop"], h, e100 / 100.0, mf)
            ref = g[k]
            assert w.shape == ref.shape, k
            np.testing.assert_allclose(w, ref, rtol=0, atol=1e-10 * max(1.0, np.abs(ref).max()), err_msg=k)
            n += 1
    assert n == 7


@pytest.mark.parametrize("name", ["G11_odd_hop300", "G7_perlman"])
def test_matches_the_recorded_analysis_waveforms(oracle, name):
    """A non-dyadic nfft / hop at two synthesis hops (float64 waveforms: 1e-10) and the 100-peak recording (stored as float32: 2e-7)."""
    g = load_golden(name)
    pid, st, ln = oracle.track(g["f"], g["mag"])
    hops = [int(k[5:]) for k in g if k.startswith("w_hop")]
    assert hops
    for h in hops:
        w = R.synth(g["f"], g["mag"], g["realph"], pid, st, ln, g["sr"], g["nfft"], g["hop"], h, 1.0, 3)
        ref = g["w_hop%d" % h]
        assert w.shape == ref.shape
        tol = 1e-10 if ref.dtype == np.float64 else 2e-7
        np.testing.assert_allclose(w, ref, rtol=0, atol=tol * max(1.0, np.abs(ref).max()))


@pytest.mark.parametrize("name", NAMES)
def test_matches_the_oracle(oracle, name):
    c = CASES[NAMES.index(name)]
    ref = _oracle(oracle, c)
    w = R.synth(*R.args(c))
    assert w.dtype == ref.dtype == np.float64 and w.shape == ref.shape == (R.plan(c).wlen,)
    assert np.abs(w - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    if c.minframes == 9:
        assert not np.any(ref) and not np.any(np.signbit(ref)) and not np.any(w) and not np.any(np.signbit(w))


@pytest.mark.parametrize("group", R.GROUPS)
def test_cases_keep_their_headroom(oracle, group, capsys):
    """max|oracle - longdouble| <= 0.1 bound(case): float64 round-off of the reference's own statements uses a tenth of what
    the kernel is allowed.  A condition on the inputs: a case that misses it is changed."""
    if not R.has_longdouble():
        pytest.skip("np.longdouble has a %d-bit mantissa here: no wider run of the reference" % (np.finfo(np.longdouble).nmant + 1))
    worst, worst_abs, bad = 0.0, 0.0, []
    for c in R.group(group):
        ref = _oracle(oracle, c)
        wl = R.synth(*R.args(c), dtype=np.longdouble)
        assert wl.dtype == np.longdouble and wl.shape == ref.shape
        d = float(np.abs(ref - wl).max())
        b = R.bound(c, ref)
        worst, worst_abs = max(worst, d / b), max(worst_abs, d)
        if not d <= 0.1 * b:
            bad.append((c.name, d, b))
    with capsys.disabled():
        print("\n[synth headroom] %-9s worst |oracle - longdouble| = %.2e = %.3f of the bound" % (group, worst_abs, worst))
    assert not bad, bad


@pytest.mark.parametrize("name", NAMES)
def test_envelope_bounds_the_waveform(name):
    c = CASES[NAMES.index(name)]
    S = R.envelope(*R.args(c))
    w = R.synth(*R.args(c))
    assert S.dtype == np.float64 and S.shape == w.shape and np.all(S >= 0)
    assert np.all(S >= np.abs(w))
    if c.minframes == 9:
        assert not np.any(S)
    else:
        assert S.max() > 0


def test_tables_hold_what_they_promise():
    for c in CASES:
        F, K = c.f.shape
        assert 8 <= F <= 16 and c.sr == 44100.0, c.name
        assert set(np.unique(c.ln)) <= set(range(1, 9)), c.name
        if K >= 8:
            assert set(np.unique(c.ln)) == set(range(1, 9)), c.name
        assert np.any(c.st == 0) and np.any(c.st + c.ln == F), c.name
        EF = max(R.plan(c).EF, 2)
        assert np.any((c.st >= 1) & (c.st <= EF)), c.name
        full = np.all(c.pid >= 0, axis=1)
        empty = np.all(c.pid < 0, axis=1)
        assert empty[1:-1].any(), c.name                                 # a frame in the middle without a peak
        a = int(np.flatnonzero(empty)[0]) + 1                            # ... and behind it K partials that start and end together
        blk = np.flatnonzero((c.st == a))
        assert len(blk) == K and len(set(c.ln[blk])) == 1 and full[a], c.name
        if K > 1:                                                        # a partial's slot changes from row to row
            moved = any(len(set(int(np.flatnonzero(c.pid[int(c.st[q]) + j] == q)[0]) for j in range(int(c.ln[q])))) > 1
                        for q in range(len(c.st)) if c.ln[q] > 1)
            assert moved, c.name
        live = c.pid >= 0
        assert np.any(live & (c.mag == 0)) and np.any(live & (c.f == 0)) and np.any(live & (c.f == c.sr / 2)), c.name
        assert np.any(c.realph > 0) and np.any(c.realph < 0), c.name
        assert np.abs(c.realph).max() <= (1e6 if c.name == "bigphase" else 1e3), c.name
    assert np.abs(CASES[NAMES.index("bigphase")].realph).max() > 1e5


def test_cases_reach_the_branches_they_name():
    """Recomputed from pvx_launch_synth's own formulas (synth_refs.plan): the paths the matrix is there for."""
    reached = {}
    for c in CASES:
        pl = R.plan(c)
        assert c.meant, c.name
        assert set(c.meant) <= pl.branches, (c.name, sorted(set(c.meant) - pl.branches))
        for b in c.meant:
            reached.setdefault(b, []).append(c.name)
    for b, names in reached.items():
        assert len(names) >= 2, (b, names)
    for b in ("rows", "copy", "regular", "irregular", "edges_inline", "edges_kernel", "tile_clamp", "tile_fit", "expm1i_series",
              "expm1i_sincos", "attack_spans_segments", "attack_cropped", "silent", "hop_below_run", "hop_not_8n"):
        assert b in reached, b
    by = {c.name: R.plan(c) for c in CASES}
    for nfft, hop_a in ((1024, 768), (1000, 300), (1024, 100)):
        for h in (33, 256):
            assert by["overlap_%d_%d_h%d" % (nfft, hop_a, h)].irregular
    assert not by["overlap_2048_64_h33"].direct and not by["overlap_2048_64_h256"].direct
    assert by["overlap_2048_128_h33"].direct and by["overlap_2048_128_h33"].dfr == 8 and by["overlap_2048_64_h33"].dfr == 16
    assert by["K_16_h8"].direct and not by["K_17_h8"].direct
    for name in ("steep_h8", "steep_h64", "steep_h8_wide"):
        x = by[name].x
        assert np.any(x >= 2.0 ** -6) and np.any(x < 2.0 ** -6), name
    # every forced run length walks its records in one tile on some cases and in several on others
    for run in (8, 16, 32):
        kinds = set("tile_clamp" in R.plan(c, run).branches for c in CASES if c.group in ("hop", "K", "steep"))
        assert kinds == {True, False}, run
    assert by["steep_h8_wide"].x.max() >= 0.25
    # edgsam (1 / overlap / 2) and edgsamp (nfft / hop / 2) truncate alike on every case: no start sample is negative, so the
    # reference leaves nothing ambiguous
    assert all(pl.edgsam == pl.edgsamp and not pl.dropped for pl in by.values())
    assert max(by[n].wlen for n in by) < 20000

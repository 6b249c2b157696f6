"""k_synth.hip against the oracle on the seeded edge cases of tests/synth_refs.py (hand-built partial tables: synthesis hops
of 1 .. 1536 samples, every nfft / hop path, rows of 1 .. 128 peaks, edges of 0 .. 7.4 segments, silent tables, slopes on both
sides of expm1i's threshold), through pypevoc_amd.PVAnalysis._device_synth (pvx_synth_flags).

Bounds (SYNTH.md, "Fixtures and tolerances"):
  float64 loop   |w - ref| <= 1e-10 max(1, Phi / 1e4) max(1, max|ref|), Phi = max|realph| + pi hop_s -- the 1e-10 this kernel is held
                 to on fixtures whose phases reach 1e4 rad, scaled with the ulp of the phase argument (bigphase only)
  float32 loop   |w - ref|[n] <= 4e-5 max(S), S the amplitude scale (synth_refs.envelope): the recurrence's R^2 / 2 x 6e-8 at R = 32
                 (3.1e-5, the kernel's header) plus the float32 rounding of the ramp and of the sum
tests/test_synth_refs_cpu.py shows that float64 round-off of the reference itself stays below a tenth of the first on every case.
Every test prints its worst error in units of its bound (pytest -s).
"""
import numpy as np
import pytest

from . import synth_refs as R

pytestmark = pytest.mark.gpu

CASES = R.cases()
F32_GROUPS = ("hop", "K", "steep", "edge")
SHAPE_GROUPS = ("hop", "K", "steep")
_ref, _env = {}, {}


@pytest.fixture(scope="module")
def dev():
    from pypevoc_amd import PVAnalysis, _lib
    _lib.init()          # raises if the HIP extension or the GPU is missing: no silent fallback

    def run(c, flags=0):
        return PVAnalysis._device_synth(*R.args(c), flags=flags)
    run.F32 = _lib.PVX_SYNTH_F32
    return run


def ref_of(oracle, c):
    if c.name not in _ref:
        w = oracle.synth(*R.args(c))
        w.setflags(write=False)
        _ref[c.name] = w
    return _ref[c.name]


def env_of(c):
    if c.name not in _env:
        S = R.envelope(*R.args(c))
        S.setflags(write=False)
        _env[c.name] = S
    return _env[c.name]


def err64(c, w, ref):
    """|w - ref| in units of the float64 bound; shape, dtype and the silent cases' exact +0.0 asserted on the way."""
    assert w.shape == ref.shape and w.dtype == ref.dtype == np.float64, (c.name, w.shape, ref.shape)
    if c.minframes == 9:
        assert not np.any(ref) and not np.any(w) and not np.any(np.signbit(w)), c.name
    return float(np.abs(w - ref).max()) / R.bound(c, ref)


def err32(c, w, ref):
    assert w.shape == ref.shape and w.dtype == np.float64, (c.name, w.shape, ref.shape)
    smax = float(env_of(c).max())
    d = float(np.abs(w - ref).max())
    return d / (4e-5 * smax) if smax > 0 else (0.0 if d == 0 else np.inf)


def report(what, worst):
    name, e = max(worst, key=lambda t: t[1])
    print("\n[synth diff] %-34s worst %.3f of its bound (%s)" % (what, e, name))
    bad = [(n, v) for n, v in worst if not v <= 1.0]
    assert not bad, (what, bad)


@pytest.mark.parametrize("group", R.GROUPS)
def test_float64_loop(dev, oracle, group):
    worst = []
    for c in R.group(group):
        worst.append((c.name, err64(c, dev(c), ref_of(oracle, c))))
    report("float64 " + group, worst)


@pytest.mark.parametrize("group", F32_GROUPS)
def test_float32_loop(dev, oracle, group):
    worst, differs = [], 0
    for c in R.group(group):
        ref = ref_of(oracle, c)
        w32 = dev(c, dev.F32)
        worst.append((c.name, err32(c, w32, ref)))
        differs += int(not np.array_equal(w32, dev(c)))
    report("float32 " + group, worst)
    assert differs == len(R.group(group))        # (a flag that is ignored would give the float64 waveform, bit for bit)


@pytest.mark.parametrize("group", SHAPE_GROUPS)
def test_run_lengths_and_slices(dev, oracle, group, monkeypatch):
    """Runs of 8 / 16 / 32 samples per thread, each held to the reference; the waveform in slices of 1 and 3 segments: the same
    additions in the same order, bit for bit."""
    worst, worst32 = [], []
    for c in R.group(group):
        ref = ref_of(oracle, c)
        for run in ("8", "16", "32"):
            monkeypatch.setenv("PVX_SYNTH_RUN", run)
            w = dev(c)
            worst.append((c.name + " run " + run, err64(c, w, ref)))
            w32 = dev(c, dev.F32)
            worst32.append((c.name + " run " + run, err32(c, w32, ref)))
            for sl in ("1", "3"):
                monkeypatch.setenv("PVX_SYNTH_SLICE", sl)
                assert np.array_equal(dev(c), w), (c.name, run, sl)
                assert np.array_equal(dev(c, dev.F32), w32), (c.name, run, sl, "f32")
                monkeypatch.delenv("PVX_SYNTH_SLICE")
            monkeypatch.delenv("PVX_SYNTH_RUN")
    report("float64 runs 8/16/32 " + group, worst)
    report("float32 runs 8/16/32 " + group, worst32)


def test_partial_major_copy_equals_the_rows(dev, monkeypatch):
    """Every case that reads its rows in place (K <= 16, dfr <= 9.5), through the partial-major copy instead: bit-identical."""
    n = 0
    for c in CASES:
        if not R.plan(c).direct:
            continue
        assert c.f.shape[1] <= 16 and R.plan(c).dfr <= 9.5
        w = dev(c)
        monkeypatch.setenv("PVX_SYNTH_CSR", "1")
        wc = dev(c)
        monkeypatch.delenv("PVX_SYNTH_CSR")
        assert np.array_equal(w, wc), c.name
        n += 1
    assert n >= 40


@pytest.mark.parametrize("var", ["PVX_SYNTH_EDGES_KERNEL", "PVX_SYNTH_NO_CUTS"])
def test_edges_kernel_and_general_bodies(dev, oracle, var, monkeypatch):
    """The attacks and releases as a launch of their own, and every body through k_synth_extras' predicated loop: each within
    the bound of the reference, on every case."""
    worst = []
    for c in CASES:
        monkeypatch.setenv(var, "1")
        w = dev(c)
        monkeypatch.delenv(var)
        worst.append((c.name, err64(c, w, ref_of(oracle, c))))
    report("float64 " + var, worst)


def test_workspace_reuse(dev, oracle):
    """One workspace (the null stream's) for every case in turn, then in reverse, then large / small / large: the segment flags and
    records that a call leaves behind change nothing in the next."""
    first = [dev(c) for c in CASES]
    worst = [(c.name, err64(c, w, ref_of(oracle, c))) for c, w in zip(CASES, first)]
    for c, w in reversed(list(zip(CASES, first))):
        assert np.array_equal(dev(c), w), c.name
    by = {c.name: (c, w) for c, w in zip(CASES, first)}
    big = max(CASES, key=lambda c: (c.f.size, R.plan(c).wlen))
    small = min(CASES, key=lambda c: (R.plan(c).wlen, c.f.size))
    assert big.f.shape[1] == 128 and R.plan(small).wlen < 32
    for c in (big, small, big):
        assert np.array_equal(dev(c), by[c.name][1]), c.name
    report("float64 one workspace", worst)

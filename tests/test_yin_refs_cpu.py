"""tests/yin_refs.py checked on its own, without a GPU: a plain float64 evaluation lies inside its bounds, wrong readings of
the text fall outside, the reference's own decisions are far from every flip on all frames the GPU tests compare, and a
signal with an exact integer period gives the exact answer."""
import math

import numpy as np
import pytest

from . import yin_refs as R


def plain_case(name, variant=None):
    case = R.CASE[name]
    x = R.signal(case.sig)
    starts, lo, hi, tol = R.case_params(case)
    return [R.yin_frame_plain(x[s:s + case.nwind], tol, lo, hi, R.SR, variant) for s in starts]


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_float64_lies_inside_the_bounds(name):
    refs = R.case_refs(name)
    worst, wtau = 0.0, 0.0
    for i, (ref, got) in enumerate(zip(refs, plain_case(name))):
        pick, tau, freq, conf, flag = got
        assert R.frame_errors(ref, pick, tau, freq, conf, flag) == [], (name, i)
        w, dt = R.worst_ratio(ref, tau, freq, conf)
        worst, wtau = max(worst, w), max(wtau, dt)
    print("%s: %d frames, worst |error| / bound %.3g, worst |dtau| %.3g" % (name, len(refs), worst, wtau))


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_wrong_variants_fall_outside_the_bounds(variant):
    outside = {}
    for name in ("a256", "a255", "e_noise256"):
        refs = R.case_refs(name)
        outside[name] = sum(bool(R.frame_errors(ref, *got)) for ref, got in zip(refs, plain_case(name, variant)))
    print(variant, outside)
    assert outside["a256"] > 0 and outside["a255"] > 0, outside
    if variant != "argmin":                                          # (on noise the reference takes the arg-min itself)
        assert outside["e_noise256"] == len(R.case_refs("e_noise256")), outside


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_reference_decisions_are_far_from_flipping(name):
    refs = R.case_refs(name)
    low = [(i, m) for i, ref in enumerate(refs) for m in ref.margins if not m.tagged and not m.value >= R.MARGIN_FLOOR]
    assert low == [], (name, low[:5])
    every = [m.value for ref in refs for m in ref.margins if not m.tagged]
    print("%s: %d decisions, smallest untagged margin %.3g, %d tagged ties"
          % (name, len(every), min(every) if every else math.inf, sum(m.tagged for ref in refs for m in ref.margins)))


def impulse_pairs(n, period=80):
    x = np.zeros(n)
    x[0::period] = 1.0
    x[3::period] = 0.5
    return x


def test_exact_integer_period():
    x = impulse_pairs(512)
    ref = R.yin_frame_ref(x, 0.15, 2, 254, R.SR)
    assert ref.dprime[80] == 0.0 and ref.pick == 80 and ref.flag == 0
    assert ref.conf == 1.0 and abs(ref.tau - 80.0) <= 0.5
    pick, tau, freq, conf, flag = R.yin_frame_plain(x, 0.15, 2, 254, R.SR)
    assert (pick, conf, flag) == (80, 1.0, 0) and abs(tau - 80.0) <= 0.5


def test_silent_and_tied_frames_are_tagged():
    refs = R.case_refs("d_silence")
    assert {r.flag for r in refs} >= {0, R.SILENT}
    for r in refs:
        if r.flag == R.SILENT:
            assert (r.pick, r.tau, r.freq, r.conf) == (0, 0.0, 0.0, 0.0)
    assert any(m.tagged for r in refs for m in r.margins)

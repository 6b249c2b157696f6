"""SpeechSegmenter on the MI355X, end to end against what the reference recorded (tests/golden/U*.npz,
make_golden_segment.py): the choices are the reference's on every segment it keeps stable under a 1e-9 relative change of
the band energies (k_fbank.hip's contract), the continuous outputs within twice the change the reference itself shows
under that perturbation, element by element, and NaN sits where the reference has it.  SEGMENT.md has the numbers."""
import numpy as np
import pytest

from . import segment_refs as R

pytestmark = pytest.mark.gpu

CASES = R.golden_cases()
IDS = ["%s-%s" % (f, c["name"]) for f, _, c, _ in CASES]


def mirror(c, x):
    from pypevoc_amd.speech import SpeechSegmenter
    sg = SpeechSegmenter(sr=c["sr"], bands=list(c["bands"]), detect_thresh=c["detect_thresh"], rough_window=c["rough_window"],
                         fine_window=c["fine_window"])
    sg.set_signal(x, c["sr"])
    return sg


def close(got, want, sens, what, rows=None):
    """NaN and infinities where the reference has them, the rest within 2 x the recorded sensitivity, element by element."""
    got, want, sens = np.asarray(got, dtype=np.float64), np.asarray(want), np.asarray(sens)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if rows is not None:
        got, want, sens = got[rows], want[rows], sens[rows]
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), what
    err = np.abs(got[fin] - want[fin])
    print("%s: max err %.3e, bound 2 x %.3e" % (what, err.max() if err.size else 0.0, sens[fin].max() if err.size else 0.0))
    assert np.all(err <= 2 * sens[fin]), (what, float((err - 2 * sens[fin]).max()))


def check_case(g, c, x):
    """One fixture case through the class; returns what it computed (for the host / device comparison)."""
    from pypevoc_amd.speech import segmenter
    n = c["name"]
    sg = mirror(c, x)
    if n + "_raises" in g:
        with pytest.raises(ValueError):
            sg.process(x)
        return None
    seg = sg.process(x)
    rough, kern = sg.last_kernels()
    assert kern == ("k_seg_detect" if len(g[n + "_det"]) else "") and rough.startswith("k_fbank_fused<%d>" % c["rough_window"])
    got = {"det": sg.detection_func.copy(), "idx": sg.detection_func_indexes_int.copy(), "seg": np.array(seg)}
    assert bool(g[n + "_stable_det"])
    assert np.array_equal(sg.detection_func_indexes_int, g[n + "_idx"]) and np.array_equal(seg, g[n + "_seg"])
    assert sg.detection_func_indexes_int.dtype == np.intp
    close(sg.detection_func, g[n + "_det"], g[n + "_sens_det"], n + " det")
    hop = c["rough_window"] // 2
    assert np.array_equal(sg.detection_func_times, g[n + "_tfb"][:-1] + hop / 2 / float(c["sr"]))
    if n + "_par_raises" in g:
        with pytest.raises(ValueError):
            sg.refine_segments_parabolic()
    else:
        sg.refine_segments_parabolic()
        close(sg.segments, g[n + "_par_seg"], g[n + "_sens_par_seg"], n + " parabolic segments")
        got["par"] = np.array(sg.segments)
        for j, pk in enumerate(sg.detection_func_indexes_int[:3]):    # the one-peak method gives the kernel's position
            assert sg.refine_segment_parabolic_fit(pk)[0] == sg.detection_function_indexes_ref[j]
    if n + "_fine_spec" not in g:
        return got
    tsegs = g[n + "_refine_tsegs"]
    for thr in c["thrs"]:
        tag = "%s_t%s_" % (n, thr)
        stable = g[tag + "stable"]
        sg.segments = tsegs.copy()
        new = sg.refine_all_all_bands(thr=thr)
        assert isinstance(new, list) and sg.segments is new and len(new) == len(tsegs)
        fine, kern = sg.last_kernels()
        assert fine.startswith("k_fbank_fused") or c["fine_window"] < 512      # (64 .. 256 go k_frames + rocFFT + k_fbank_rows)
        assert kern == ("k_seg_refine" if len(tsegs) else "") and segmenter.last_kernels() == kern
        d = sg._refine_details()
        assert np.array_equal(d["cross"][stable], g[tag + "cross"][stable])
        close(d["valb"], g[tag + "valb"], g["%s_sens_t%s_valb" % (n, thr)], tag + "valb", stable)
        close(d["vala"], g[tag + "vala"], g["%s_sens_t%s_vala" % (n, thr)], tag + "vala", stable)
        close(new, g[tag + "refined"], g["%s_sens_t%s_refined" % (n, thr)], tag + "refined", stable)
        got[tag] = (np.array(new), d["cross"].copy(), d["valb"].copy())
        if len(tsegs):                                                # one segment alone: the same path, the same bits
            one = sg.refine_segment_all_bands(tsegs[0], thr=thr) / sg.sr
            assert one == new[0] or (np.isnan(one) and np.isnan(new[0]))
    assert np.array_equal(sg.fine_time, g[n + "_tfine"])
    fs = sg.fine_spec
    assert fs.shape == g[n + "_fine_spec"].shape
    with np.errstate(divide="ignore"):
        want = 10 * np.log10(g[n + "_fine_spec"])
    ok = np.isfinite(want)
    assert np.array_equal(np.isfinite(fs), ok) and np.abs(fs[ok] - want[ok]).max() < 1e-7      # 1e-9 relative in energy is 4.3e-9 dB
    return got


@pytest.mark.parametrize("f,g,c,x", CASES, ids=IDS)
def test_class_reproduces_the_reference_from_a_host_signal(f, g, c, x):
    check_case(g, c, x)


@pytest.mark.parametrize("k", [0, 8, 9, 14])                         # float32, int16 (Perlman), a silent gap, times at the end
def test_device_resident_signal_gives_the_host_signals_bits(k):
    import torch
    f, g, c, x = CASES[k]
    host = check_case(g, c, x)
    dev = check_case(g, c, torch.from_numpy(np.ascontiguousarray(x)).cuda())
    assert host.keys() == dev.keys()
    for key in host:
        for a, b in zip(host[key] if isinstance(host[key], tuple) else (host[key],), dev[key] if isinstance(dev[key], tuple) else (dev[key],)):
            assert R.same(a, b), key


@pytest.mark.parametrize("on_device", [False, True])
def test_refine_interval_all_modes(on_device):
    import torch
    from pypevoc_amd.speech import segmenter
    f, g, c, x = CASES[0]
    n = c["name"]
    sg = mirror(c, torch.from_numpy(x).cuda() if on_device else x)
    for k, (t0, t1) in enumerate(c["intervals"]):
        for mode in c["modes"]:
            key = "%s_iv%d_%s_" % (n, k, mode)
            tr = sg.refine_interval(t0, t1, mode=mode)
            assert sg.last_kernels()[1] == "k_seg_transitions" == segmenter.last_kernels()
            assert tr is sg.trans and np.array_equal(sg.tfine, g[key + "tfine"])
            close(tr, g[key + "trans"], g["%s_sens_iv%d_%s_trans" % (n, k, mode)], key + "trans")
            close(sg.bandtrans, g[key + "bandtrans"], g["%s_sens_iv%d_%s_bandtrans" % (n, k, mode)], key + "bandtrans")
            want = g[key + "finespec"]
            assert sg.finespec.shape == want.shape and np.abs(sg.finespec / want - 1).max() < 1e-9


def test_refine_interval_raises_where_the_reference_does():
    f, g, c, x = CASES[0]
    sg = mirror(c, x)
    with pytest.raises(ValueError) as e:                              # a level far outside the two values: nothing crosses it
        sg.refine_interval(1.0, 1.25, mode="mean", thr=-5.0)
    assert "band" in str(e.value) and ("start" in str(e.value) or "end" in str(e.value))
    with pytest.raises(NotImplementedError):                          # 5.1 s at hop 16: 5100 frames in a series
        from pypevoc_amd.speech import SpeechSegmenter
        s2 = SpeechSegmenter(sr=c["sr"], bands=list(c["bands"]), rough_window=2048, fine_window=32)
        s2.set_signal(x, c["sr"])
        s2.refine_interval(0.5, 5.5)
    with pytest.raises(ValueError):
        sg.refine_interval(1.0, 1.25, mode="nope")


def test_refine_refuses_sides_beyond_the_limit():
    f, g, c, x = CASES[0]
    from pypevoc_amd.speech import SpeechSegmenter
    sg = SpeechSegmenter(sr=c["sr"], bands=list(c["bands"]), rough_window=8192, fine_window=64)   # 2 * 8192 / 32 = 512 frames a side
    sg.set_signal(x, c["sr"])
    with pytest.raises(NotImplementedError):
        sg.refine_segment_all_bands(3.0)


def test_transition_points_one_row_and_rows_agree_with_the_restatement():
    from pypevoc_amd.speech import refine_transition_points, transition_points_rows
    rng = np.random.default_rng(3)
    n = 40
    step = np.concatenate([-40 + rng.uniform(-1, 1, 20), -20 + rng.uniform(-1, 1, 20)])
    perm = rng.permutation(n)
    order = np.argsort(perm)
    tx, xs = (np.arange(n) * 0.01)[perm], step[perm]                  # unsorted: the host sorts tx, the series with it
    assert np.array_equal(xs[order], step)
    for mode in ("minmax", "median", "mean", "pct10"):
        want = R.transitions_row(xs[order], tx[order], 0.195, mode, 0.5)
        got = refine_transition_points(xs, tx, 0.195, mode=mode, thr=0.5)
        assert got == want[:3], (mode, got, want)
        ttr, vb, va, st = transition_points_rows(np.vstack([xs, xs[::-1]]), tx, 0.195, mode=mode)
        assert st[0] == R.OK and (ttr[0], vb[0], va[0]) == want[:3]
    assert refine_transition_points(xs, tx, 5.0) == (5.0, 0, 0)
    with pytest.raises(ValueError):
        refine_transition_points(np.zeros(8), None, 3.5)

"""pypevoc_amd.speech.fricatives on the MI355X (k_fric.hip) against the reference's recorded values (tests/golden/Z*.npz,
make_golden_fricatives.py).

Bounds (FRICATIVES.md): the psd within 1e-9 relative per bin (the project's per-bin spectrum bound, FILTERBANK.md); imax
identical; each of the seven descriptors within 1e-9 x sum_k |d value / d ln S[k]|, computed with numpy from the fixture's own
psd row (tests/fricative_refs.py: closed forms, checked against long-double central differences in test_fricatives_cpu.py);
rms within 1e-9 (1 + |mean| / std) relative.  No row, bin or case is left out.  Run with -s for the worst measured values."""
import numpy as np
import pytest

from . import fricative_refs as R
from .test_fricatives_cpu import all_cases, check_hand_row, check_values, fixture, get_case, hand_rows

pytestmark = pytest.mark.gpu

FUSED = (512, 1024, 2048)
ROWS = "k_fric_frames+rocfft+k_fric_acc"
TAIL = "+k_fric_desc+k_fric_rms"
DTYPES = {"float32": np.float32, "float64": np.float64, "int16": np.int16}


def spectrum_kernels(nper):
    return "k_fric_fused<%d>" % nper if nper in FUSED else ROWS


def signal(g, case, dtype):
    return np.ascontiguousarray(g[case["x"]].astype(DTYPES[dtype]))


def runs(fname, cname):
    g, case = get_case(fname, cname)
    return [(g, case, dt) for dt in case["dtypes"]]


def psd_within(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float64
    err = float(np.max(np.abs(got - want) / want))
    print("%-34s psd worst relative error %.1e (bound %.0e)" % (what, err, R.PSD_BOUND))
    assert np.isfinite(got).all() and err <= R.PSD_BOUND, (what, err)


def same_rows(a, b, keys=None):
    keys = keys or sorted(set(a) & set(b))
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys)


@pytest.mark.parametrize("fname,cname", all_cases())
def test_welch_rows_against_the_fixture(fname, cname, monkeypatch):
    """Every case, in each of its sample types, on its documented route; the fused lengths once more down the rows route, and
    each route against the other."""
    from pypevoc_amd.speech import fricatives as fr
    for g, case, dt in runs(fname, cname):
        x = signal(g, case, dt)
        nper = fr.geometry(case["L"], case["nwind"])[0]
        want = g[cname + "_psd"]
        freq, psd = fr.welch_rows(x, case["starts"], case["L"], case["nwind"], case["sr"])
        assert fr.last_kernels() == spectrum_kernels(nper)
        assert freq.tobytes() == g[cname + "_freq"].tobytes()
        psd_within(psd, want, "%s %s" % (cname, dt))
        if nper in FUSED:
            monkeypatch.setenv("PVX_FRIC_ROWS", "1")
            _, rows = fr.welch_rows(x, case["starts"], case["L"], case["nwind"], case["sr"])
            assert fr.last_kernels() == ROWS
            monkeypatch.delenv("PVX_FRIC_ROWS")
            psd_within(rows, want, "%s %s rows route" % (cname, dt))
            psd_within(rows, psd, "%s %s rows against fused" % (cname, dt))


@pytest.mark.parametrize("fname,cname", all_cases())
def test_fricative_rows_against_the_reference(fname, cname, monkeypatch):
    from pypevoc_amd.speech import fricatives as fr
    for g, case, dt in runs(fname, cname):
        x = signal(g, case, dt)
        nper = fr.geometry(case["L"], case["nwind"])[0]
        got = fr.fricative_rows(x, case["starts"], case["L"], case["nwind"], case["sr"], return_psd=True)
        assert fr.last_kernels() == spectrum_kernels(nper) + TAIL
        assert not got["status"].any() and got["status"].dtype == np.int32 and got["imax"].dtype == np.int32
        for k in R.REFERENCE_KEYS:
            assert got[k].shape == (len(case["starts"]),) and got[k].dtype == np.float64
        psd_within(got["psd"], g[cname + "_psd"], "%s %s full call" % (cname, dt))
        check_values(g, case, got, dt)
        if nper in FUSED:
            monkeypatch.setenv("PVX_FRIC_ROWS", "1")
            rows = fr.fricative_rows(x, case["starts"], case["L"], case["nwind"], case["sr"])
            assert fr.last_kernels() == ROWS + TAIL
            monkeypatch.delenv("PVX_FRIC_ROWS")
            check_values(g, case, rows, dt + " rows route")
            assert same_rows(got, rows, ["rms"])                      # the samples' own sums do not depend on the route


def test_snip_is_row_zero():
    """FricativeDataFromSnip: the reference's keys, Python floats, row 0 of the batched call bit for bit; a snippet shorter than
    nwind uses nper = len(w)."""
    from pypevoc_amd.speech import fricatives as fr
    for fname, cname in (("Z1_rows", "w256"), ("Z1_rows", "w333_l300"), ("Z3_fused", "w1024_i16")):
        g, case = get_case(fname, cname)
        x = signal(g, case, case["dtypes"][0])
        s = case["starts"][1]
        w = x[s:s + case["L"]]
        d = fr.FricativeDataFromSnip(w, nwind=case["nwind"], sr=case["sr"])
        assert tuple(d) == R.REFERENCE_KEYS and all(type(v) is float for v in d.values())
        rows = fr.fricative_rows(x, case["starts"], case["L"], case["nwind"], case["sr"])
        for k in R.REFERENCE_KEYS:
            assert np.float64(d[k]).tobytes() == rows[k][1].tobytes(), (cname, k)
        check_values(g, case, rows, "the batched call")               # (and that call is the reference's, within the bounds)


@pytest.mark.parametrize("fname,cname", [("Z1_rows", "w256"), ("Z2_fused512", "w512_l768"), ("Z3_fused", "w1024_i16")])
def test_bit_identities(fname, cname, monkeypatch):
    """A device-resident signal against the host; a call under a small PVX_MAX_DEVICE_BYTES against the unchunked call; starts
    permuted against the rows permuted; the descriptor-only entry on the full call's psd rows against its descriptors."""
    import torch
    from pypevoc_amd.speech import fricatives as fr
    g, case = get_case(fname, cname)
    x = signal(g, case, case["dtypes"][0])
    args = (case["L"], case["nwind"], case["sr"])
    starts = np.array(case["starts"])
    full = fr.fricative_rows(x, starts, *args, return_psd=True)
    dev = fr.fricative_rows(torch.from_numpy(x).cuda(), starts, *args, return_psd=True)
    assert same_rows(full, dev) and len(set(full) & set(dev)) == 12
    _, wdev = fr.welch_rows(torch.from_numpy(x).cuda(), starts, *args)
    _, whost = fr.welch_rows(x, starts, *args)
    assert wdev.tobytes() == full["psd"].tobytes() == whost.tobytes()
    # chunks: a span of about a snippet and a half forces groups of one or two rows, each copying its own span
    monkeypatch.setenv("PVX_MAX_DEVICE_BYTES", str(int(1.5 * case["L"]) * x.dtype.itemsize))
    cut = fr.fricative_rows(x, starts, *args, return_psd=True)
    monkeypatch.delenv("PVX_MAX_DEVICE_BYTES")
    assert same_rows(full, cut)
    perm = np.random.default_rng(5).permutation(len(starts))
    shuf = fr.fricative_rows(x, starts[perm], *args, return_psd=True)
    for k in R.REFERENCE_KEYS + ("imax", "status", "psd"):
        assert shuf[k].tobytes() == full[k][perm].tobytes(), k
    twice = fr.fricative_rows(x, np.concatenate((starts, starts[:1])), *args)      # another grid, a repeated row
    assert all(twice[k][:-1].tobytes() == full[k].tobytes() and twice[k][-1] == full[k][0] for k in R.REFERENCE_KEYS)
    only = fr.fricative_desc_rows(full["psd"], full["freq"])
    assert fr.last_kernels() == "k_fric_desc"
    assert same_rows(full, only, list(R.KEYS) + ["imax", "status"])


def test_tail_on_hand_built_rows():
    """fricative_desc_rows: the peak at bin 0, at bin 1 and at the last bin, a plateau, a zero bin left of the peak, an all-zero
    row; nb = 2; nb = 129 and 1025 (the lane stride's remainders).  The regular rows against numpy and the package's
    DistribMoments within the bounds, every row against its status and nan pattern."""
    from pypevoc_amd.speech import fricatives as fr
    from pypevoc_amd.speech.SpeechAnalysis import DistribMoments
    f, rows = hand_rows()
    names = list(rows)
    got = fr.fricative_desc_rows(np.array([rows[n][0] for n in names]), f)
    for r, name in enumerate(names):
        S, status, nans = rows[name]
        d = dict((k, got[k][r]) for k in got)
        check_hand_row(name, f, S, d, status, nans)
        if not S.any():
            continue                                                  # (nan throughout: checked above)
        ref = R.descriptors(f, S)                                     # what a zero bin leaves finite is the restatement's value
        with np.errstate(divide="ignore", invalid="ignore"):
            bounds = R.value_bounds(f, S)
            y = 10 * np.log10(S)
        im = int(np.argmax(S))
        if S.all():
            if im >= 1:
                ref["slope_left"] = 1000 * np.polyfit(f[:im + 1], y[:im + 1], 1)[0]
            if im <= len(S) - 2:
                ref["slope_right"] = 1000 * np.polyfit(f[im:], y[im:], 1)[0]
        ref["cent"], ref["stdev"], ref["skew"], ref["kurt"] = DistribMoments(f, S)[:4]
        for k in R.KEYS:
            if k not in nans:
                assert abs(d[k] - ref[k]) <= bounds[k], (name, k, d[k], ref[k], bounds[k])
    assert got["f_max"][names.index("peak_last")] == f[-1] and got["f_max"][names.index("peak_bin0")] == f[1]
    assert got["imax"][names.index("plateau")] == 4 and got["f_max"][names.index("plateau")] == f[4]
    two = fr.fricative_desc_rows(np.array([[1.0, 3.0], [3.0, 1.0]]), f[:2])
    assert two["status"].tolist() == [1, 1] and two["imax"].tolist() == [1, 0] and two["f_max"].tolist() == [f[1], f[1]]
    assert np.isnan(two["slope_right"][0]) and np.isnan(two["slope_left"][1])
    assert abs(two["slope_left"][0] - 1000 * 10 * np.log10(3.0) / f[1]) <= 1e-9 * abs(two["slope_left"][0])
    for fname, cname in (("Z1_rows", "w256"), ("Z3_fused", "w2048_l4096")):           # nb = 129 and 1025
        g, case = get_case(fname, cname)
        psd, freq = g[cname + "_psd"], g[cname + "_freq"]
        assert psd.shape[1] in (129, 1025)
        d = fr.fricative_desc_rows(psd, freq)
        assert np.array_equal(d["imax"], g[cname + "_imax"]) and not d["status"].any()
        for r in range(len(psd)):
            bounds = R.value_bounds(freq, psd[r])
            want = R.descriptors(freq, psd[r], np.longdouble)
            for k in R.KEYS:
                assert abs(d[k][r] - float(want[k])) <= bounds[k], (cname, r, k)


def np_rows(x, starts, L, nwind, sr):
    return R.welch_rows(np.asarray(x, dtype=np.float64), starts, L, nwind, sr)[1]


@pytest.mark.parametrize("nwind", [512, 1024, 256])
def test_more_snippets_than_one_pass_holds(nwind):
    """5 000 overlapping snippets of one segment pair: more than the fused grid has waves (a wave then walks several snippets,
    prefetching across them) and, at nwind 256, more than one rocFFT batch of whole snippets (32 MB of frames: 5 461 snippets of
    3 segments).  The rows of the big call are those of small calls on the same snippets, bit for bit, and numpy's within 1e-9."""
    from pypevoc_amd.speech import fricatives as fr
    g = fixture("Z3_fused")
    x = np.ascontiguousarray(g["long16"])
    sr = 16000
    L = nwind + nwind // 2 if nwind != 256 else 512
    nrows = 5000 if nwind != 256 else 6000
    starts = (np.arange(nrows) * 7919) % (len(x) - L + 1)              # unsorted, overlapping, the last sample reached
    starts[-1] = len(x) - L
    big = fr.fricative_rows(x, starts, L, nwind, sr, return_psd=True)
    assert fr.last_kernels() == spectrum_kernels(nwind) + TAIL
    for lo, hi in ((0, 40), (nrows // 2 + 3, nrows // 2 + 70), (nrows - 25, nrows)):
        small = fr.fricative_rows(x, starts[lo:hi], L, nwind, sr, return_psd=True)
        for k in R.REFERENCE_KEYS + ("imax", "status", "psd"):
            assert small[k].tobytes() == big[k][lo:hi].tobytes(), (nwind, lo, k)
    pick = np.array([0, nrows // 2 + 5, nrows - 1])
    psd_within(big["psd"][pick], np_rows(x, starts[pick], L, nwind, sr), "nwind %d, %d snippets" % (nwind, nrows))


def test_snippet_longer_than_a_batch():
    """One snippet of 16 389 segments at nwind 256 -- five more than a rocFFT batch holds: it is cut between segments and carries
    its sums through its psd row.  Beside it in the call, a second snippet; both against numpy within the bounds."""
    from pypevoc_amd.speech import fricatives as fr
    nwind, sr = 256, 16000
    L = 16389 * 128 + 128
    rng = np.random.default_rng(77)
    x = (rng.standard_normal(L + 1000) + 0.25).astype(np.float32)
    starts = [1000, 0]
    assert fr.geometry(L, nwind)[2] == 16389
    got = fr.fricative_rows(x, starts, L, nwind, sr, return_psd=True)
    assert fr.last_kernels() == ROWS + TAIL and not got["status"].any()
    xd = x.astype(np.float64)
    for r, s in enumerate(starts):
        w = xd[s:s + L]
        seg = np.lib.stride_tricks.sliding_window_view(w, nwind)[::128][:16389]
        win = R.hann_periodic(nwind)
        X = np.fft.rfft((seg - seg.mean(axis=1, keepdims=True)) * win, axis=1)
        want = R.one_sided(nwind) * (np.abs(X) ** 2).mean(axis=0) / (sr * (win * win).sum())
        psd_within(got["psd"][r:r + 1], want[None, :], "16 389 segments, row %d" % r)
        ref = R.descriptors(got["freq"], want)
        bounds = R.value_bounds(got["freq"], want)
        assert got["imax"][r] == ref["imax"]
        for k in R.KEYS:
            assert abs(got[k][r] - ref[k]) <= bounds[k], (r, k, got[k][r], ref[k], bounds[k])
        assert abs(got["rms"][r] - w.std()) <= R.rms_bound(w) * w.std()


def test_intervals_through_one_call():
    from pypevoc_amd.speech import fricatives as fr
    g, case = get_case("Z3_fused", "w1024_i16")
    x = signal(g, case, "int16")
    sr = case["sr"]
    intervals = [(0.05, 0.25), (0.30, 0.34), (0.0, 0.01), (0.2, len(x) / sr)]
    out = fr.fricative_intervals(x, sr, intervals, pos=(0.25, 0.5), wsize=1024)
    assert fr.last_kernels() == "k_fric_fused<1024>" + TAIL and sorted(out) == [0.25, 0.5]
    imin = fr.interval_windows(intervals, sr, (0.25, 0.5), 1024)
    assert (imin[2] < 0).all()                                        # 10 ms at the start of the signal: the window starts before it
    inside = (imin >= 0) & (imin + 1024 <= len(x))
    rows = fr.fricative_rows(x, imin[inside], 1024, 1024, sr)
    for j, pp in enumerate((0.25, 0.5)):
        assert out[pp]["status"].tolist() == [0 if ok else 4 for ok in inside[:, j]]
        for k in R.REFERENCE_KEYS:
            full = np.full(imin.shape, np.nan)
            full[inside] = rows[k]                                    # the windows went through the call interval by interval
            assert np.isnan(out[pp][k][~inside[:, j]]).all() and not np.isnan(out[pp][k][inside[:, j]]).any()
            assert out[pp][k][inside[:, j]].tobytes() == full[inside[:, j], j].tobytes(), (pp, k)


def test_errors_and_no_rows():
    from pypevoc_amd import PvxError
    from pypevoc_amd.speech import fricatives as fr
    x = np.zeros(3000, dtype=np.float32)
    with pytest.raises(PvxError) as e:
        fr.fricative_rows(x, [0, 100, 3000 - 511, 7], 512, 256)
    assert "status -6" in str(e.value) and "row 2 " in str(e.value)
    with pytest.raises(PvxError) as e:
        fr.welch_rows(x, [0, -1], 512, 256)
    assert "status -6" in str(e.value) and "row 1 " in str(e.value)
    with pytest.raises(PvxError):
        fr.welch_rows(x, [0], 1, 256)
    fr.welch_rows(x + 1, [0], 512, 512)
    assert fr.last_kernels() != ""
    freq, psd = fr.welch_rows(x, [], 512, 256)
    assert psd.shape == (0, 129) and freq.shape == (129,) and fr.last_kernels() == ""
    d = fr.fricative_rows(x, [], 512, 256)
    assert all(d[k].shape == (0,) for k in R.REFERENCE_KEYS + ("imax", "status")) and fr.last_kernels() == ""
    d = fr.fricative_desc_rows(np.zeros((0, 129)), freq)
    assert d["f_max"].shape == (0,) and fr.last_kernels() == ""

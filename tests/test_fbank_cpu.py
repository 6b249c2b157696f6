"""FFT filter banks (pypevoc_amd.FFTFilters): what needs no GPU -- the namespace, filter construction against the F*
fixtures (pure numpy: exact equality), the reference's quirks, the not-mirrored stub, the fixtures' own consistency and
the loud failure without a device.  The GPU comparison is test_fbank_gpu.py."""
import glob
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ("DCT1", "DCT2", "DCT3", "DCT4", "IFFT")


def fbank_golden_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "F*.npz")))


def load_fbank_golden(name):
    """(fixture dict, list of cases)."""
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    if "x_from" in g:                                                # F7: G7's int16 Perlman samples
        g["x"] = np.load(os.path.join(GOLDEN, str(g["x_from"]) + ".npz"))["x"][:int(g["x_len"])]
    return g, json.loads(str(g["cases"]))


def all_cases():
    out = []
    for name in fbank_golden_names():
        _, cases = load_fbank_golden(name)
        out += [(name, c["name"]) for c in cases]
    return out


def get_case(name, cname):
    g, cases = load_fbank_golden(name)
    return g, [c for c in cases if c["name"] == cname][0]


def build_bank(ft, case):
    """The mirror's filter bank of a fixture case, as make_golden_fbank.py built the reference's."""
    kw = dict(case["ctor"])
    if case.get("fspecs") is not None:
        kw["fspec_list"] = [ft.PiecewiseFilterSpec(**{k: (np.array(v) if isinstance(v, list) else v) for k, v in s.items()})
                            for s in case["fspecs"]]
    bank = getattr(ft, case["cls"])(**kw)
    for r in case.get("zero_rows") or []:
        bank.fb[r, :] = 0.0
    return bank


def case_signal(ft, g, case):
    x = g[case["x"]]
    assert str(x.dtype) == ("float32" if case["dtype"] == "float64" else case["dtype"])
    if case["dtype"] == "float64":
        x = x.astype(np.float64)
    if case.get("slice"):
        x = x[case["slice"][0]:case["slice"][1]]
    if case.get("preemph"):
        x = ft.preemph(x, **case["preemph"])
    return x


def cep_matrix(mode, N):
    """[n][k] matrix of the cepstral transform from its defining sum (scipy.fftpack.dct norm=None; np.fft.ifft)."""
    n = np.arange(N)[:, None].astype(np.float64)
    k = np.arange(N)[None, :].astype(np.float64)
    if mode == "DCT1":
        m = 2 * np.cos(np.pi * k * n / (N - 1))
        m[0, :] = 1.0
        m[N - 1, :] = (-1.0) ** np.arange(N)
        return m
    if mode == "DCT2":
        return 2 * np.cos(np.pi * k * (2 * n + 1) / (2 * N))
    if mode == "DCT3":
        m = 2 * np.cos(np.pi * (2 * k + 1) * n / (2 * N))
        m[0, :] = 1.0
        return m
    if mode == "DCT4":
        return 2 * np.cos(np.pi * (2 * k + 1) * (2 * n + 1) / (4 * N))
    return np.exp(2j * np.pi * k * n / N) / N


def test_reference_import_lines_work():
    from pypevoc_amd import FFTFilters as ft
    from pypevoc_amd import FilterBank, TriangularFilterBank, MelFilterBank, PiecewiseFilterSpec
    from pypevoc_amd.FFTFilters import BandError, preemph, f_to_mel, mel_to_f, nextpow2, peaks, nearest, fft_filter  # noqa: F401
    assert ft.FilterBank is FilterBank and ft.PiecewiseFilterSpec is PiecewiseFilterSpec
    assert issubclass(MelFilterBank, TriangularFilterBank) and issubclass(TriangularFilterBank, FilterBank)
    assert issubclass(BandError, Exception)
    assert callable(MelFilterBank.mfcc) and callable(MelFilterBank.mfcc_and_mel) and callable(FilterBank.specout)


@pytest.mark.parametrize("name,cname", all_cases())
def test_construction_reproduces_the_reference_bit_for_bit(name, cname):
    from pypevoc_amd import FFTFilters as ft
    g, case = get_case(name, cname)
    bank = build_bank(ft, case)
    assert bank.fb.dtype == np.float64 and bank.fb.shape == g[cname + "_fb"].shape
    assert np.array_equal(bank.fb, g[cname + "_fb"])
    assert np.array_equal(bank.fvec, g[cname + "_fvec"])
    assert np.array_equal(bank.wind, g[cname + "_wind"])
    assert bank.hop == int(g[cname + "_hop"]) and bank.nwind == g[cname + "_fb"].shape[1]
    assert list(bank.label) == json.loads(str(g[cname + "_label"]))
    assert repr(bank).startswith("FilterBank with filters:\n")


def test_fixture_list_is_complete():
    names = fbank_golden_names()
    assert [n.split("_")[0] for n in names] == ["F%d" % i for i in range(1, 9)]
    for n in names:
        assert os.path.getsize(os.path.join(GOLDEN, n + ".npz")) < 1 << 20
    cases = dict((c, n) for n, c in all_cases())
    nwinds = {c: get_case(n, c)[0][c + "_fb"].shape[1] for c, n in cases.items()}
    assert nwinds["mel44k"] == 1024 and nwinds["mel16k"] == 512 and nwinds["mel96k"] == 2048 and nwinds["mel8k"] == 256
    assert nwinds["chunk_bp"] == 4096 and nwinds["n1000_exact"] == 1000 and nwinds["n999_odd"] == 999
    # F3: the top mel band at 8 kHz lives in the upper half of the spectrum
    fb = get_case("F3_mel8k", "mel8k")[0]["mel8k_fb"]
    assert (fb[-1, :128] == 0).all() and (fb[-1, 129:] != 0).any()


def test_piecewise_spec_modes_and_vertex_form():
    from pypevoc_amd.FFTFilters import PiecewiseFilterSpec, BandError
    lp = PiecewiseFilterSpec(mode='lp', freq=1000, sr=8000.)
    assert lp.label == 'Lowpass filter, fc=1000.0'
    assert np.array_equal(lp.bandf, [[0.0, 0.125], [0.125, 0.5]]) and np.array_equal(lp.bandg, [[1, 1], [0, 0]])
    assert PiecewiseFilterSpec(mode='HiPass', freq=1000, sr=8000.).label == 'Hipass filter, fc=1000.0'
    bs = PiecewiseFilterSpec(mode='bandstop', freq=[1000, 2000], sr=8000.)
    assert bs.label == 'Bandstop filter, fc=1500.0' and np.array_equal(bs.bandg, [[1, 1], [0, 0], [1, 1]])
    f, gn = bs.get_frequency_gains()
    assert np.array_equal(f, [[0, 1000], [1000, 2000], [2000, 4000]]) and gn.shape == (3, 2)
    assert np.array_equal(bs.get_frequency_edges(), [0, 1000, 2000, 4000])
    v = PiecewiseFilterSpec(freq=np.array([2000., 0., 1000.]), gain=np.array([0., 0., 1.]), sr=8000.)
    assert v.label == 'Piecewise filter with 1 bands'                 # (len(bandf) - 1, as the reference counts)
    assert np.array_equal(v.bandf * 8000., [[0, 1000], [1000, 2000]])
    assert np.array_equal(v.apply_to_freq_vector([0., 500., 1000., 1500., 2000., 3000.]), [0, .5, 1, .5, 0, 0])
    assert repr(v) == ('Piecewise filter with 1 bands:\n  Freq = [0.0,1000.0]: gain = [0.0,1.0]\n'
                       '  Freq = [1000.0,2000.0]: gain = [1.0,0.0]\n')
    assert repr(lp).splitlines()[1] == '  Freq = [0.0,1000.0]: gain = 1.0'
    # two edges that fall on the same element of the frequency vector: the band has no width
    narrow = PiecewiseFilterSpec(mode='bp', freq=[1000, 1001], sr=8000.)
    with pytest.raises(BandError) as e:
        narrow.apply_to_freq_vector(np.linspace(0, 8000., 64), align_edges=True)
    assert "too narrow" in str(e.value) and e.value.message == str(e.value)
    assert narrow.apply_to_freq_vector(np.linspace(0, 8000., 64), align_edges=False).shape == (64,)


def test_quirks_that_decide_numbers():
    from pypevoc_amd import FFTFilters as ft
    assert float(ft.f_to_mel(700.)) == 1125. + np.log(2.)             # a sum, not the mel formula's product
    assert abs(float(ft.mel_to_f(ft.f_to_mel(3000.))) - 3000.) < 1e-6
    assert ft.f_to_mel(np.array([0., 700.])).shape == (2,)
    x = np.arange(8, dtype=np.float64) ** 2
    y = ft.preemph(x, hpFreq=50., Fs=8000.)
    a = np.exp(-2. * np.pi * 50. / 8000.)
    assert y.dtype == np.float32 and y[-1] == 49.0
    assert np.array_equal(y[:-1], (x[:-1].astype('f') - x[1:].astype('f') * a).astype('f'))   # the NEXT sample
    assert ft.preemph(x) is x
    b = ft.TriangularFilterBank(flim=[0.1, 0.2, 0.30000001, 0.4], nwind=64)
    f32 = np.float32
    assert b.fb.shape == (2, 64) and b.hop == 32                      # the limits are rounded to float32
    assert b.label[0] == '{} band ({}-{})'.format(f32(0.2), f32(0.1), f32(0.30000001)) and float(f32(0.30000001)) != 0.30000001
    assert ft.TriangularFilterBank(flim=[100., 200., 400.], nwind=64, sr=8000.).label == ['200.0Hz band (100.0-400.0Hz)']
    m = ft.MelFilterBank(sr=22050.)
    assert m.nwind == 512 and m.hop == 220 and m.fb.shape == (26, 512) and m.fvec[1] == 22050. / 511
    assert ft.nextpow2(1000) == 1024.0
    assert np.array_equal(ft.peaks(np.array([0, 2, 1, 3, 3, 1, 5, 0])), [1, 6])
    assert np.array_equal(ft.nearest([0.9, 5.2], np.array([0., 1., 5.])), [1., 5.])


def test_fft_filter_stub_names_the_reference_lines():
    from pypevoc_amd import FFTFilters as ft
    with pytest.raises(NotImplementedError) as e:
        ft.fft_filter(np.zeros(16), [(0, 0.1)], [(1., 1.)])
    assert "FFTFilters.py:376-405" in str(e.value)


@pytest.mark.parametrize("mode", ["DCT5", "dct2", "FFT", ""])
def test_unknown_mfcc_mode_is_not_implemented(mode):
    from pypevoc_amd import MelFilterBank
    with pytest.raises(NotImplementedError):
        MelFilterBank(sr=16000.).mfcc(np.zeros(2000), mode=mode)


def test_too_many_bands_names_the_cap():
    from pypevoc_amd import FFTFilters as ft
    bank = ft.FilterBank(nwind=512)
    bank.fb = np.ones((ft.MAX_NBAND + 1, 512))
    with pytest.raises(NotImplementedError) as e:
        bank.specout(np.zeros(2000))
    assert str(ft.MAX_NBAND) in str(e.value)
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "pvx.h")).read()
    assert "#define PVX_FBANK_MAX_NBAND %d" % ft.MAX_NBAND in hdr and ft.MAX_NBAND >= 128


def specout_numpy(x, wind, hop, fb):
    """float64 restatement of FilterBank.specout (FFTFilters.py:274-292) on the half spectrum."""
    nwind = len(wind)
    half = nwind // 2 + 1
    fold = fb[:, :half].copy()
    k = np.arange(1, (nwind - 1) // 2 + 1)
    fold[:, k] += fb[:, nwind - k]
    rows = []
    n = 0
    x = np.asarray(x, dtype=np.float64)
    while n < len(x) - nwind:
        p = np.abs(np.fft.rfft(x[n:n + nwind] * wind)) ** 2
        rows.append(fold @ p)
        n += hop
    return np.array(rows)


@pytest.mark.parametrize("name,cname", all_cases())
def test_fixtures_are_self_consistent(name, cname):
    from pypevoc_amd import FFTFilters as ft
    g, case = get_case(name, cname)
    x = case_signal(ft, g, case)
    fb, wind, hop = g[cname + "_fb"], g[cname + "_wind"], int(g[cname + "_hop"])
    spec, t = g[cname + "_spec"], g[cname + "_t"]
    assert case["raises"]["specout"] is None
    mine = specout_numpy(x, wind, hop, fb)
    if mine.size == 0:
        assert spec.shape == (0,) and t.shape == (0,) and len(x) <= len(wind)
        assert case["raises"]["mfcc"] == ("ValueError" if case["modes"] else None)
        return
    assert case["raises"]["mfcc"] is None
    assert spec.shape == mine.shape == (len(t), fb.shape[0])
    assert np.array_equal(spec == 0, mine == 0)
    nz = spec != 0
    assert np.max(np.abs(mine[nz] - spec[nz]) / spec[nz]) < 1e-11
    assert np.array_equal(t, (np.arange(len(t)) * hop + len(wind) / 2.) / float(case["ctor"].get("sr", 1.0)))
    # the cepstra are the defining sums of the transforms applied to log(spec), wherever every log is finite
    fin = nz.all(axis=1)
    for mode in case["modes"]:
        cep = g[cname + "_cep_" + mode]
        assert cep.dtype == (np.complex128 if mode == "IFFT" else np.float64) and cep.shape == spec.shape
        want = np.log(spec[fin]) @ cep_matrix(mode, spec.shape[1])
        assert np.max(np.abs(cep[fin] - want), initial=0.0) < 1e-10
        assert not np.isfinite(cep[~fin]).any()


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import pypevoc_amd
    x = np.sin(2 * np.pi * 440 / 16000 * np.arange(16000))
    with pytest.raises(pypevoc_amd.PvxError) as e:
        pypevoc_amd.MelFilterBank(sr=16000.).mfcc(x)
    assert "no CPU fallback" in str(e.value)
    with pytest.raises(pypevoc_amd.PvxError):
        pypevoc_amd.FilterBank().specout(x)

"""Buffer reuse in the host layer (pypevoc_amd/csrc/pvx_mem.h and its users): a plan's grow-only buffers across calls of
different sizes, and the process-wide workspaces of pvx_periodicity / pvx_filterbank across window lengths.  Reused memory
must never show in a result: everything is compared bit for bit."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR, NFFT, HOP, NPKS = 44100, 512, 128, 8
SIZES = (4096, 65536, 8192)
LIMIT = 200000                              # PVX_MAX_DEVICE_BYTES of the chunked runs


def signal(n, seed, freq=440.0, sr=SR):
    t = np.arange(n) / float(sr)
    return 0.5 * np.sin(2 * np.pi * freq * t) + 0.01 * np.random.default_rng(seed).standard_normal(n)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()      # (NaN == NaN, -0.0 != 0.0)


def new_plan(precision):
    from pypevoc_amd.PVAnalysis import _Plan
    return _Plan(SR, NFFT, HOP, NPKS, 0.0, np.hanning(NFFT), precision)


def analyze(plan, x):
    """pvx_analyze of the float64 host signal x on `plan`: the seven output arrays and the last spectrum."""
    from pypevoc_amd import _lib
    lib = _lib.load()
    F = int(lib.pvx_nframes(len(x), NFFT, HOP))
    out = {k: np.empty(F * NPKS) for k in ("f", "mag", "ph", "realph", "binno")}
    out["t"], out["totalmag"], out["last_spec"] = np.empty(F), np.empty(F), np.empty(NFFT)
    got = lib.pvx_analyze(plan.handle, ctypes.c_void_p(x.ctypes.data), _lib.PVX_F64, len(x), 1, len(x),
                          *[_lib.dptr(out[k]) for k in ("f", "mag", "ph", "realph", "binno", "t", "totalmag")], None, _lib.dptr(out["last_spec"]))
    _lib.check(got, "pvx_analyze")
    assert got == F
    return out


def chunks(nsamp, limit, es=8):
    """analyze_host's chunk count for one signal of float64 samples under PVX_MAX_DEVICE_BYTES = limit."""
    F = -(-(nsamp - NFFT) // HOP)
    per_chunk = max(1, (limit - NFFT * es) // (HOP * es + (5 * NPKS + 2) * 8))
    return -(-F // min(per_chunk, F))


@pytest.mark.parametrize("limit", (None, LIMIT), ids=("one_chunk", "chunked"))
@pytest.mark.parametrize("precision", (32, 64))
def test_one_plan_reused_across_sizes(precision, limit, monkeypatch):
    if limit is None:
        monkeypatch.delenv("PVX_MAX_DEVICE_BYTES", raising=False)
    else:
        monkeypatch.setenv("PVX_MAX_DEVICE_BYTES", str(limit))
        assert chunks(65536, limit) >= 3
    xs = [signal(n, seed) for seed, n in enumerate(SIZES)]
    plan = new_plan(precision)
    for n, x in zip(SIZES, xs):
        got = analyze(plan, x)                  # the buffers of the earlier, larger or smaller, calls
        want = analyze(new_plan(precision), x)  # a fresh plan, the same single call
        for k in want:
            assert same_bits(got[k], want[k]), (precision, limit, n, k)
        assert np.isfinite(got["f"]).any() and got["mag"].max() > 0


def periodicity(x, nwind, method, cand):
    from pypevoc_amd import _lib
    lib = _lib.load()
    _lib.init()
    wind = np.ones(nwind)                       # (the reference's default window)
    idx = np.arange(nwind // 2, len(x) - nwind + nwind // 2, nwind // 2, dtype=np.int64)
    nf, ncand = len(idx), 8
    per, st = np.empty(nf * ncand), np.empty(nf * ncand)
    cnt, pref = np.empty(nf, np.int32), np.empty(nf, np.int32)
    got = lib.pvx_periodicity(_lib.dptr(x), len(x), _lib.dptr(wind), nwind, idx.ctypes.data_as(_lib.c_int64_p), nf, method, cand, 2, nwind // 3,
                              0.5, 0.2, ncand, 0.1, _lib.dptr(per), _lib.dptr(st), cnt.ctypes.data_as(_lib.c_int32_p),
                              pref.ctypes.data_as(_lib.c_int32_p))
    _lib.check(got, "pvx_periodicity")
    assert got == nf
    return {"period": per, "strength": st, "count": cnt, "preferred": pref}


def filterbank(x, nwind, cep_mode):
    from pypevoc_amd import _lib
    lib = _lib.load()
    _lib.init()
    nband, hop = 8, nwind // 2
    k = np.arange(nwind)
    centres = (np.arange(nband) + 1.0) * (nwind / 2.0) / (nband + 1)
    fb = np.ascontiguousarray(np.maximum(0.0, 1.0 - np.abs(k[None, :] - centres[:, None]) / (nwind / 16.0)))
    wind = np.hanning(nwind)
    nfr = int(lib.pvx_nframes(len(x), nwind, hop))
    spec, cep = np.empty(nfr * nband), np.empty(nfr * nband)
    got = lib.pvx_filterbank(ctypes.c_void_p(x.ctypes.data), _lib.PVX_F64, len(x), _lib.dptr(wind), nwind, hop, _lib.dptr(fb), nband, cep_mode,
                             _lib.dptr(spec), _lib.dptr(cep) if cep_mode else None)
    _lib.check(got, "pvx_filterbank")
    assert got == nfr
    return {"spec": spec, "cep": cep} if cep_mode else {"spec": spec}


def first_equals_third(run):
    """window lengths 64, 1024, 64 on one 16384-sample signal through a process-wide workspace: the larger call in between
    must not show in the third result."""
    x = signal(16384, 7, freq=1000.0, sr=16000)     # a period of 16 samples: inside the lag range of the 64-sample windows
    first, mid, third = run(x, 64), run(x, 1024), run(x, 64)
    for k in first:
        assert same_bits(first[k], third[k]), k
    assert all(len(mid[k]) for k in mid)
    return first


@pytest.mark.parametrize("method,cand", ((0, 0), (1, 1)), ids=("xcorr_fft", "amdf"))
def test_periodicity_workspace_reused_across_windows(method, cand):
    r = first_equals_third(lambda x, n: periodicity(x, n, method, cand))
    assert (r["count"] > 0).any()


@pytest.mark.parametrize("rows_route", (False, True), ids=("default_routes", "rocfft_rows"))
@pytest.mark.parametrize("cep_mode", (0, 2), ids=("spec", "dct2"))
def test_filterbank_workspace_reused_across_windows(cep_mode, rows_route, monkeypatch):
    # rocfft_rows: window 1024 takes k_frames + rocFFT + k_fbank_rows too (PVX_FBANK_ROWS), a second plan on the shared work buffer
    if rows_route:
        monkeypatch.setenv("PVX_FBANK_ROWS", "1")
    else:
        monkeypatch.delenv("PVX_FBANK_ROWS", raising=False)
    r = first_equals_third(lambda x, n: filterbank(x, n, cep_mode))
    assert np.isfinite(r["spec"]).all() and r["spec"].max() > 0

"""k_fused_rev's instantiations with npks as a compile-time constant (KC = 8) and with the hop taken from the H template
parameter: the same arithmetic on the same values as the generic kernel, so every result array is bit-identical to what
PVX_REV_NO_SPEC=1 (the generic kernel of the same geometry) computes, and pvx_plan_last_kernels says which of the two ran.
npks 20 (the dense staging) stays among the cases: its instantiations were measured and not kept (0 % on a tone, +1 % on noise:
profiles/rev_spec_ab.jsonl), so the dispatcher must name the generic kernel both times there, as for npks 7 and 9.
Shapes: the smallest at which each specialised path can go wrong -- three signals of ~40 frames in one call (zero rows between
them): the bench's harmonic tone (one candidate per lane), white noise (> 64 candidates: radix select, thinning) and silence
followed by a tone (zero spectra, the x/0 rule); grids of 1 and 3 workgroups (several rows per wave: hand-over through the stash,
full per-peak passes of 8 frames and a partial tail pass) and the default grid; float32 aligned, float32 one sample into the
buffer (4-byte loads) and int16."""
import ctypes

import numpy as np
import pytest

from .parity import compare_analysis

pytestmark = pytest.mark.gpu

SR = 44100.0
NFRAMES = 40
FIELDS = ("f", "mag", "ph", "realph", "binno", "t", "totalmag")


@pytest.fixture(scope="module")
def lib():
    from pypevoc_amd import _lib
    _lib.init()          # raises if the HIP extension or the GPU is missing: no silent fallback
    return _lib.load()


def bench_tone(n, seed=1234, f0=220.0):
    """bench.py's c2 generator: 8 harmonics, 1 % / 5 Hz vibrato, amplitudes 0.3 / h, noise"""
    t = np.arange(n, dtype=np.float64) / SR
    ph = 2 * np.pi * f0 * (t - 0.01 / (2 * np.pi * 5.0) * np.cos(2 * np.pi * 5.0 * t))
    x = sum(0.3 / h * np.sin(h * ph) for h in range(1, 9)) + 0.001 * np.random.default_rng(seed).standard_normal(n)
    return x.astype(np.float32)


_signals = {}


def signals(nfft, hop):
    """[3, nsamp] float32, computed once per geometry and left unchanged: tone | white noise | silence, then the tone"""
    if (nfft, hop) not in _signals:
        n = nfft + hop * (NFRAMES - 1) + 3
        tone = bench_tone(n)
        noise = (0.1 * np.random.default_rng(99).standard_normal(n)).astype(np.float32)
        late = tone.copy()
        late[: nfft + hop * 17 + 5] = 0.0
        xb = np.stack([tone, noise, late])
        xb.setflags(write=False)
        _signals[(nfft, hop)] = xb
    return _signals[(nfft, hop)]


def device_input(xb, kind):
    """the batch on the device as `kind`: (tensor kept alive, pointer, x_dtype, signal stride)"""
    import torch
    from pypevoc_amd import _lib
    dev = torch.device("cuda", 0)
    nsig, n = xb.shape
    if kind == "i16":
        d = torch.from_numpy(np.round(xb * 20000).astype(np.int16)).to(dev)
        return d, d.data_ptr(), _lib.PVX_I16, n
    stride = n + (n & 1)                                            # even: only the start address decides the 8-byte loads
    d = torch.zeros(nsig * stride + 3, dtype=torch.float32, device=dev)
    off = 1 if kind == "f32_odd" else 0                             # (the allocation itself is 8-byte aligned: asserted below)
    for b in range(nsig):
        d[off + b * stride: off + b * stride + n] = torch.from_numpy(np.array(xb[b])).to(dev)
    ptr = d.data_ptr() + 4 * off
    assert (ptr % 8 == 0) == (kind == "f32")
    return d, ptr, _lib.PVX_F32, stride


def analyze(lib, nfft, hop, K, ptr, x_dtype, n, nsig, stride, wire_format=0):
    """One pvx_analyze_dev (wire_format 0) or pvx_analyze_dev_wire call on a fresh plan -> (arrays or bytes, kernels)"""
    import torch
    from pypevoc_amd import _lib
    from pypevoc_amd.batch import ResultWire
    dev = torch.device("cuda", 0)
    plan = ctypes.c_void_p()
    _lib.check(lib.pvx_plan_create(ctypes.byref(plan), SR, nfft, hop, K, 0.005, _lib.dptr(np.hanning(nfft)), 32, 0), "pvx_plan_create")
    try:
        assert lib.pvx_plan_get_fft_mode(plan) == 4
        F = int(lib.pvx_nframes(n, nfft, hop))
        assert F == NFRAMES
        rows = nsig * F
        if wire_format:
            wire = ResultWire(plan, rows, K, wire_format=wire_format)
            w = torch.full((wire.nbytes,), 0xAB, dtype=torch.uint8, device=dev)
            r = lib.pvx_analyze_dev_wire(plan, ptr, x_dtype, n, nsig, stride, w.data_ptr(), None)
            assert r == F, (r, lib.pvx_last_error())
            torch.cuda.synchronize()
            out = w.cpu().numpy()
        else:
            nk = rows * K
            res = torch.full((5 * nk + 2 * rows,), np.nan, dtype=torch.float64, device=dev)
            a = [res.data_ptr() + 8 * i * nk for i in range(5)] + [res.data_ptr() + 8 * (5 * nk), res.data_ptr() + 8 * (5 * nk + rows)]
            r = lib.pvx_analyze_dev(plan, ptr, x_dtype, n, nsig, stride, a[0], a[1], a[2], a[3], a[4], a[5], a[6], None, None)
            assert r == F, (r, lib.pvx_last_error())
            torch.cuda.synchronize()
            h = res.cpu().numpy()
            out = {k: h[i * nk:(i + 1) * nk].reshape(rows, K) for i, k in enumerate(FIELDS[:5])}
            out["t"] = h[5 * nk: 5 * nk + rows]
            out["totalmag"] = h[5 * nk + rows:]
        return out, lib.pvx_plan_last_kernels(plan).decode()
    finally:
        lib.pvx_plan_destroy(plan)


def pair(lib, monkeypatch, *args, **kw):
    a = analyze(lib, *args, **kw)
    monkeypatch.setenv("PVX_REV_NO_SPEC", "1")
    try:
        b = analyze(lib, *args, **kw)
    finally:
        monkeypatch.delenv("PVX_REV_NO_SPEC")
    return a, b


def kernel_name(kc):
    return "analysis=k_fused_rev" + ("<kc%d>" % kc if kc else "")


# (nfft, hop, npks, the KC the dispatcher must pick)
CASES = [(2048, 512, 8, 8), (2048, 1024, 8, 8), (2048, 300, 8, 8), (1024, 256, 8, 8), (512, 128, 8, 8),
         (2048, 512, 20, 0), (2048, 1024, 20, 0), (1024, 256, 20, 0), (512, 128, 20, 0),
         (2048, 512, 7, 0), (2048, 512, 9, 0)]


@pytest.mark.parametrize("nfft,hop,K,kc", CASES)
def test_specialised_kernel_is_bit_identical_to_generic(lib, monkeypatch, nfft, hop, K, kc):
    xb = signals(nfft, hop)
    nsig, n = xb.shape
    for kind in ("f32", "f32_odd", "i16"):
        keep, ptr, x_dtype, stride = device_input(xb, kind)
        for nb in (None, "1", "3"):
            if nb:
                monkeypatch.setenv("PVX_FUSED_BLOCKS", nb)
            try:
                (a, ka), (b, kb) = pair(lib, monkeypatch, nfft, hop, K, ptr, x_dtype, n, nsig, stride)
            finally:
                if nb:
                    monkeypatch.delenv("PVX_FUSED_BLOCKS")
            assert ka == kernel_name(kc) and kb == kernel_name(0), (kind, nb, ka, kb)
            for k in FIELDS:
                assert not np.isnan(a[k]).any(), (kind, nb, k)
                assert np.array_equal(a[k].view(np.int64), b[k].view(np.int64)), (kind, nb, k)
            # the shapes do what they are here for: peaks on every signal, full rows on the noise, empty rows in the silence
            F = NFRAMES
            assert (a["f"][:F] > 0).sum() >= F and (a["f"][F:2 * F] > 0).sum() >= F and (a["f"][2 * F:2 * F + 10] > 0).sum() == 0
        del keep


@pytest.mark.parametrize("wire_format", [1, 2])
def test_specialised_kernel_writes_the_same_wire_block(lib, monkeypatch, wire_format):
    nfft, hop, K = 2048, 512, 8
    xb = signals(nfft, hop)
    nsig, n = xb.shape
    keep, ptr, x_dtype, stride = device_input(xb, "f32")
    for nb in (None, "1"):
        if nb:
            monkeypatch.setenv("PVX_FUSED_BLOCKS", nb)
        try:
            (a, ka), (b, kb) = pair(lib, monkeypatch, nfft, hop, K, ptr, x_dtype, n, nsig, stride, wire_format=wire_format)
        finally:
            if nb:
                monkeypatch.delenv("PVX_FUSED_BLOCKS")
        assert ka == kernel_name(8) and kb == kernel_name(0), (nb, ka, kb)
        assert a.tobytes() == b.tobytes(), nb
        assert (a != 0xAB).sum() > a.size // 2
    del keep


def test_specialised_kernel_against_the_oracle(lib, oracle):
    """... so that the check does not rest on the generic kernel alone: the dispatched nfft 2048 / hop 512 / npks 8 result on the
    tone against the oracle, at the float32 tolerances of tests/test_hip_parity.py (assert_f32)."""
    nfft, hop, K = 2048, 512, 8
    xb = signals(nfft, hop)[:1]
    n = xb.shape[1]
    keep, ptr, x_dtype, stride = device_input(xb, "f32")
    got, kern = analyze(lib, nfft, hop, K, ptr, x_dtype, n, 1, stride)
    assert kern == kernel_name(8)
    o = oracle.analyze(xb[0].astype(np.float64), SR, nfft, hop, K)
    c = compare_analysis(got, o, nfft, hop, SR)
    print(c)
    assert c["bad_peaks"] <= 1e-3 * max(c["ref_peaks"], 1), c
    assert c["ph_norm"] <= 2e-6 and c["realph_norm"] <= 2e-5 and c["f_norm"] <= 2e-5 and c["mag_norm"] <= 1e-6, c
    assert c["totalmag_rel"] <= 1e-6, c
    assert c["f_abs"] <= 1e-3 and c["mag_rel"] <= 1e-5 and c["ph_abs"] <= 2e-5, c
    del keep

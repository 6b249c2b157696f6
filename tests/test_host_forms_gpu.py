"""The host forms of the whole-signal operations (pvx_heterodyne, pvx_rms_frames, pvx_funcwind, pvx_hetharm,
pvx_hetharm_resynth, pvx_periodicity, pvx_yin, pvx_marks_corr, pvx_marks_peak) stage the caller's arrays and delegate to
their `_dev` forms: what the other GPU tests leave out of that.  Host arrays against the same arrays on the GPU, optional
outputs omitted against present, an input just above the size up to which a host array is copied directly, and calls
without a frame.  Every comparison is bit for bit."""
import ctypes

import numpy as np
import pytest

from pypevoc_amd import _lib

pytestmark = pytest.mark.gpu

WLEN, HOP = 64, 16
N = 3 * WLEN + 1                                                      # 9 frames, the last one ends a sample before the signal does
WIND = np.blackman(WLEN)
SR = 8000.0
FW_MEAN, FW_STD = 1, 4                                                # pvx_funcwind_op of include/pvx.h
NHARM = 3


class In(object):
    """an input array: the caller's (host form) or a copy on the GPU (`_dev` form); complex values as pairs of float64"""
    def __init__(self, a):
        a = np.ascontiguousarray(a)
        self.a = a.view(np.float64) if np.iscomplexobj(a) else a


class Out(object):
    """an output array of `count` elements, every byte 0x5a before the call; present=False: the caller passes NULL"""
    def __init__(self, dtype, count, present=True):
        self.a = np.frombuffer(b"\x5a" * (count * np.dtype(dtype).itemsize), dtype=dtype).copy() if present else None


def untouched(a):
    return a.tobytes() == b"\x5a" * a.nbytes


def call(name, dev, *args):
    """pvx_<name> on host arrays, or pvx_<name>_dev on the In / Out arrays on the GPU and torch's current stream (other numpy
    arrays stay on the host in both forms): the returned count and the Out arrays, None for an omitted one."""
    import torch
    lib = _lib.load()
    tdev = torch.device("cuda", _lib.init())
    full = name + "_dev" if dev else name
    types = _lib.SIGNATURES[full][1]
    cargs, outs, alive = [], [], []
    for i, a in enumerate(args):
        if isinstance(a, (In, Out)):
            h = a.a
            if dev and h is not None:
                assert h.size > 0
                h = torch.from_numpy(h).to(tdev)
            alive.append(h)                                           # (a device copy lives until the call has returned)
            if isinstance(a, Out):
                outs.append(h)
            a = None if h is None else ctypes.c_void_p(h.data_ptr()) if dev else h.ctypes.data_as(types[i])
        elif isinstance(a, np.ndarray):
            a = a.ctypes.data_as(types[i])
        cargs.append(a)
    if dev:
        cargs.append(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert len(cargs) == len(types)
    got = _lib.check(getattr(lib, full)(*cargs), full)
    return got, [o.cpu().numpy() if dev and o is not None else o for o in outs]


def nframes(n):
    return int(_lib.load().pvx_nframes(n, WLEN, HOP))


def signal(n=N, seed=1):
    t = np.arange(n)
    return np.cos(2 * np.pi * 0.031 * t + 0.3) + 0.1 * np.random.default_rng(seed).standard_normal(n)


def hetsig(n=N):
    return np.exp(-2j * np.pi * 0.031 * np.arange(n))


def fvec(n=N):
    return 0.031 * (1 + 0.05 * np.sin(2 * np.pi * np.arange(n) / 150.0))


def heterodyne(dev, n=N, icent=True):
    nfr = max(nframes(n), 1)
    return call("pvx_heterodyne", dev, In(signal(n)), In(hetsig(n)), n, WIND, WLEN, HOP, Out(np.float64, 2 * nfr), Out(np.int64, nfr, icent))


def rms_frames(dev, n=N):
    return call("pvx_rms_frames", dev, In(signal(n)), n, WIND, WLEN, HOP, Out(np.float64, max(nframes(n), 1)))


def funcwind(dev, func, cpx, n=N):
    x = signal(n) * hetsig(n) if cpx else signal(n)
    nout = max(nframes(n), 1) * (2 if cpx and func == FW_MEAN else 1)
    return call("pvx_funcwind", dev, In(x), int(cpx), n, WIND, WLEN, HOP, func, float(WIND.sum()), Out(np.float64, nout))


def hetharm(dev, n=N, icent=True):
    nfr = max(nframes(n), 1)
    return call("pvx_hetharm", dev, In(signal(n)), n, In(fvec(n)), WIND, WLEN, HOP, 0, NHARM, 1, Out(np.float64, 2 * nfr * NHARM),
                Out(np.int64, nfr, icent))


def resynth(dev, ah, first, count, filt, hf, n=N):
    return call("pvx_hetharm_resynth", dev, In(fvec(n)), n, In(ah), nframes(n), NHARM, WLEN, HOP, first, count, filt, SR, 100.0, 1000.0, 0.1,
                Out(np.float64, n), Out(np.float64, 2 * n, hf))


def yin(dev, x, starts, optional=True):
    nfr = len(starts)
    return call("pvx_yin", dev, In(x), len(x), starts, nfr, WLEN, 2, WLEN // 2 - 2, 0.15, SR, Out(np.float64, max(nfr, 1)), Out(np.float64, max(nfr, 1)),
                Out(np.float64, max(nfr, 1), optional), Out(np.int32, max(nfr, 1), optional), Out(np.int32, max(nfr, 1), optional))


def same(a, b):
    assert len(a) == len(b)
    return all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


HOST_AND_DEVICE = {
    "heterodyne": heterodyne,
    "rms_frames": rms_frames,
    "funcwind_std_real": lambda dev: funcwind(dev, FW_STD, False),
    "funcwind_mean_complex": lambda dev: funcwind(dev, FW_MEAN, True),
}


@pytest.mark.parametrize("name", sorted(HOST_AND_DEVICE))
def test_host_arrays_give_the_bits_of_device_arrays(name):
    nh, host = HOST_AND_DEVICE[name](False)
    nd, dev = HOST_AND_DEVICE[name](True)
    assert nh == nd == nframes(N) == 9
    assert same(host, dev)
    assert not any(untouched(a) for a in host) and np.isfinite(host[0]).all() and np.abs(host[0]).max() > 0


@pytest.mark.parametrize("hf", [True, False])
def test_resynthesis_from_host_arrays_gives_the_bits_of_device_arrays(hf):
    ah = hetharm(False)[1][0]
    for first, count, filt in ((1, 1, 0), (1, 1, 1)) + (() if hf else ((0, NHARM, 0),)):   # (the interpolated amplitude is one harmonic's)
        nh, host = resynth(False, ah, first, count, filt, hf)
        nd, dev = resynth(True, ah, first, count, filt, hf)
        assert nh == nd == N
        assert same(host[:1], dev[:1]) and np.isfinite(host[0]).all()
        assert (host[1] is None and dev[1] is None) if not hf else same(host[1:], dev[1:])
    assert np.abs(host[0]).max() > 0


def test_omitted_optional_outputs_leave_the_others_as_they_are():
    assert same(heterodyne(False)[1][:1], heterodyne(False, icent=False)[1][:1])
    assert same(hetharm(False)[1][:1], hetharm(False, icent=False)[1][:1])
    ah = hetharm(False)[1][0]
    assert same(resynth(False, ah, 1, 1, 1, True)[1][:1], resynth(False, ah, 1, 1, 1, False)[1][:1])
    x = signal(20 * WLEN)
    starts = np.arange(0, len(x) - WLEN + 1, 3 * HOP, dtype=np.int64)
    full, bare = yin(False, x, starts)[1], yin(False, x, starts, optional=False)[1]
    assert bare[2:] == [None, None, None] and same(full[:2], bare[:2])
    assert not any(untouched(a) for a in full)


def test_an_input_that_bounces_through_the_ring_gives_the_bits_of_device_input():
    """70 000 float64 samples are 560 000 bytes: above the 512 KiB up to which a pageable host array is copied directly, so
    the signal goes through the process-wide ring's memory; the last frame ends with the signal."""
    x = signal(70000, seed=2)
    assert x.nbytes > 512 << 10
    starts = np.append(np.arange(0, len(x) - WLEN, 997, dtype=np.int64), len(x) - WLEN)
    nh, host = yin(False, x, starts)
    nd, dev = yin(True, x, starts)
    assert nh == nd == len(starts)
    assert same(host, dev) and np.isfinite(host[1]).all()


def test_calls_without_a_frame_return_0_and_write_nothing():
    from pypevoc_amd.SoundUtils import yin_last_kernels
    from pypevoc_amd.marks import marks_last_kernels, period_marks_peak
    assert nframes(WLEN) == 0
    ah = np.zeros((1, NHARM), dtype=np.complex128)
    none = np.zeros(0, dtype=np.int64)
    for got, outs in (heterodyne(False, WLEN), rms_frames(False, WLEN), funcwind(False, FW_STD, False, WLEN), funcwind(False, FW_MEAN, True, WLEN),
                      hetharm(False, WLEN), resynth(False, ah, 1, 1, 0, True, WLEN)):
        assert got == 0 and all(untouched(a) for a in outs)
    x = signal(20 * WLEN)
    yin(False, x, np.zeros(1, dtype=np.int64))
    assert yin_last_kernels() != ""
    got, outs = yin(False, x, none)
    assert got == 0 and all(untouched(a) for a in outs) and yin_last_kernels() == ""
    cand, cnt = [Out(np.float64, 1), Out(np.float64, 1)], [Out(np.int32, 1), Out(np.int32, 1)]
    got, outs = call("pvx_periodicity", False, In(x), len(x), WIND, WLEN, none, 0, 0, 0, 2, WLEN // 3, 0.5, 0.2, 8, 0.1, *(cand + cnt))
    assert got == 0 and all(untouched(a) for a in outs)
    period_marks_peak(np.cos(2 * np.pi * 100.0 * np.arange(2000) / SR), sr=SR, f=100.0)
    assert marks_last_kernels() != ""
    marks, rest = Out(np.float64, 1), [Out(np.float64, 1), Out(np.int32, 1), Out(np.int32, 1)]
    got, outs = call("pvx_marks_peak", False, In(x), len(x), none, none, None, 0, None, np.full(1, 100.0), 0, 1, SR, 3, 4, 16, marks, *rest)
    assert got == 0 and all(untouched(a) for a in outs) and marks_last_kernels() == ""
    period_marks_peak(np.cos(2 * np.pi * 100.0 * np.arange(2000) / SR), sr=SR, f=100.0)
    got, outs = call("pvx_marks_corr", False, In(x), len(x), none, none, None, None, 0, np.zeros(1), np.full(1, 100.0), 1, 100.0, SR, 32, 0.001, 4, 16,
                     marks, *rest[1:])
    assert got == 0 and all(untouched(a) for a in outs) and marks_last_kernels() == ""

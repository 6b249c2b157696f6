"""The host side of SoundUtils.f0yin / aubio_f0yin, without a GPU: framing, argument errors, the tolerance message."""

import numpy as np
import pytest


def reference_loop(nsamp, nwind, hop, sr):
    """The framing loop of the reference's aubio_f0yin (SoundUtils.py:255, 258)."""
    starts, time = [], []
    for ii in range(0, nsamp - nwind, hop):
        starts.append(ii)
        time.append(float(ii + nwind / 2) / sr)
    return np.array(starts, dtype=np.int64), np.array(time)


@pytest.mark.parametrize("nwind", [8, 255, 256, 1024])
@pytest.mark.parametrize("hop", [1, 64, 100, 512])
def test_frame_starts_and_times(nwind, hop):
    from pypevoc_amd.SoundUtils import yin_frames
    sr = 16000
    for nsamp in (0, nwind - 1, nwind, nwind + 1, nwind + hop, nwind + hop + 1, nwind + 3 * hop, nwind + 3 * hop + hop // 2, nwind + 7 * hop - 1):
        starts, time = yin_frames(nsamp, sr, nwind, hop)
        rs, rt = reference_loop(nsamp, nwind, hop, sr)
        assert np.array_equal(starts, rs) and starts.dtype == np.int64, (nsamp, nwind, hop)
        assert np.array_equal(time, rt), (nsamp, nwind, hop)
        if len(starts):
            assert starts[-1] + nwind < nsamp                        # the strict upper end


def test_no_frame_gives_three_empty_arrays():
    from pypevoc_amd.SoundUtils import aubio_f0yin, f0yin
    for y in (np.zeros(1024), np.zeros(100), np.zeros(0)):
        for out in (f0yin(y, 44100), aubio_f0yin(y, 44100, 1024, 512)):
            assert len(out) == 3 and all(isinstance(a, np.ndarray) and a.shape == (0,) for a in out)
    full = f0yin(np.zeros(1024), 44100, full=True)
    assert sorted(full) == ["conf", "flag", "freq", "pick", "starts", "tau", "time"] and all(len(v) == 0 for v in full.values())


def test_lag_range():
    from pypevoc_amd.SoundUtils import yin_lags
    assert yin_lags(1024, 44100) == (2, 510)
    assert yin_lags(255, 16000) == (2, 125)
    assert yin_lags(8, 16000) == (2, 2)
    assert yin_lags(1024, 16000, fmin=150.0, fmax=400.0) == (40, 107)
    assert yin_lags(1024, 16000, fmin=10.0) == (2, 510)              # ceil(sr / fmin) beyond the window: L - 2
    assert yin_lags(1024, 16000, fmax=1e6) == (2, 510)
    assert yin_lags(256, 16000, fmax=219.0) == (73, 126) and yin_lags(256, 16000, fmin=223.0) == (2, 72)
    assert yin_lags(1024, 16000, fmin=100.0, fmax=100.0) == (160, 160)


def test_argument_errors():
    from pypevoc_amd.SoundUtils import f0yin, f0yin_rows
    y = np.zeros(4096)
    with pytest.raises(ValueError):
        f0yin(y, 16000, nwind=7)
    with pytest.raises(ValueError):
        f0yin(y, 16000, hop=0)
    with pytest.raises(ValueError):
        f0yin(y, 16000, nwind=1024, fmin=200.0, fmax=100.0)          # lo = 160 > hi = 80
    with pytest.raises(ValueError):
        f0yin(y, 16000, nwind=64, fmax=400.0)                        # lo = 40 > L - 2 = 30
    with pytest.raises(ValueError):
        f0yin_rows(y, [4000], 1024, 16000)                           # the frame leaves the signal
    with pytest.raises(ValueError):
        f0yin_rows(y, [-1], 1024, 16000)
    with pytest.raises(ValueError):
        f0yin(np.zeros((4, 4096)), 16000, nwind=8, hop=1)


@pytest.mark.parametrize("tolerance", [0.0, 1.0, 1.5, -0.2])
def test_tolerance_out_of_bounds_is_reported(tolerance, capsys):
    from pypevoc_amd.SoundUtils import aubio_f0yin
    aubio_f0yin(np.zeros(100), 44100, tolerance=tolerance)           # (no frame: nothing runs)
    assert capsys.readouterr().err == "Tolerance not set: Out of bounds\n"


def test_tolerance_in_bounds_is_silent(capsys):
    from pypevoc_amd.SoundUtils import aubio_f0yin
    aubio_f0yin(np.zeros(100), 44100, tolerance=0.3)
    aubio_f0yin(np.zeros(100), 44100)
    assert capsys.readouterr().err == ""


def test_other_aubio_methods_raise():
    from pypevoc_amd.SoundUtils import aubio_f0yin
    with pytest.raises(NotImplementedError):
        aubio_f0yin(np.zeros(4096), 44100, method="yinfft")


def test_without_a_gpu_the_failure_is_loud():
    """No CPU fallback: with frames to analyse the call reaches the library, which refuses without a device."""
    import torch
    import pypevoc_amd
    from pypevoc_amd.SoundUtils import f0yin
    if torch.cuda.is_available():
        assert len(f0yin(np.zeros(4096), 16000)) == 3
    else:
        with pytest.raises(pypevoc_amd.PvxError):
            f0yin(np.zeros(4096), 16000)

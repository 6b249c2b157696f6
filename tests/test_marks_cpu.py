"""pypevoc_amd.marks without a GPU: what the host layer refuses before anything reaches the library, the step bound it derives,
and the entry points the library exports."""
import numpy as np
import pytest


def test_arguments_are_refused_on_the_host():
    from pypevoc_amd.marks import period_marks_corr, period_marks_peak, period_marks_rows
    x = np.zeros(100)
    with pytest.raises(ValueError, match="fit_points"):
        period_marks_peak(x, sr=8000, f=150.0, fit_points=2)
    with pytest.raises(ValueError, match="strictly increasing"):
        period_marks_corr(x, sr=8000, tf=[0.0, 0.0], f=[150.0, 150.0])
    with pytest.raises(ValueError, match="same, non-zero"):
        period_marks_corr(x, sr=8000)
    with pytest.raises(ValueError, match="window_size"):
        period_marks_corr(x, sr=8000, tf=[0.0, 1.0], f=[150.0, 150.0], window_size=1)
    with pytest.raises(ValueError, match="1-D"):
        period_marks_corr(np.zeros((2, 50)), sr=8000, tf=[0.0, 1.0], f=[150.0, 150.0])
    with pytest.raises(ValueError, match="inside"):
        period_marks_rows(x, [0], [101], sr=8000, tf=[0.0, 1.0], f=[150.0, 150.0])
    with pytest.raises(ValueError, match="one value per sample"):
        period_marks_peak(x, sr=8000, f=np.ones(99))
    with pytest.raises(ValueError, match="'corr' or 'peak'"):
        period_marks_rows(x, [0], [100], sr=8000, tf=[0.0, 1.0], f=[150.0, 150.0], method="amdf")


def test_step_bound_and_messages():
    from pypevoc_amd import marks
    f = np.array([100.0, np.nan, 200.0])
    assert marks.corr_max_steps(8000, 8000.0, 0.001, f) == 1002       # 1 s in steps of min(0.001, 1 / 200) s, + 2
    assert marks.corr_max_steps(8000, 8000.0, 0.01, f) == 202
    assert marks.corr_max_steps(8000, 8000.0, 0.0, f) == 4 * 8000 + 16
    assert marks.corr_max_steps(100, 8000.0, 1e-9, f) == 416
    assert "no local maximum" in marks.status_message(marks.NO_PEAK) and ";" in marks.status_message(marks.NO_PEAK | marks.STEPS)
    assert marks.status_message(marks.SHORT_FIT) == ""


def test_library_exports_the_entry_points():
    from pypevoc_amd import _lib
    lib = _lib.load()
    for name in ("pvx_marks_corr", "pvx_marks_corr_dev", "pvx_marks_peak", "pvx_marks_peak_dev", "pvx_marks_last_kernels"):
        assert hasattr(lib, name), name
    assert lib.pvx_marks_last_kernels() == b""

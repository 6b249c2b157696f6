#!/usr/bin/env python3
"""Generate the K*.npz golden vectors of pypevoc_amd.marks by IMPORTING the reference (pypevoc/Periodicity.py:
period_marks_corr :573-618, period_marks_peak :621-709) and running the two functions unchanged.

Run in the build container only (the reference never travels to the GPU box):

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_marks.py

(PYPEVOC_REFERENCE names the reference's checkout.)  Under numpy >= 2 the reference's `except (ValueError, np.RankWarning)`
needs the name: np.RankWarning = np.exceptions.RankWarning is set before the call, a shim of the kind of the xrange one.

  K1_marks_corr  sig_<key>: float32 signals; cases: the JSON list tests/marks_refs.py: CORR_FIXTURES; <name>_marks
  K2_marks_peak  sig_<key>; cases: PEAK_FIXTURES; <name>_marks, <name>_vals
The fixtures are float32-exact synthetic vowels of at most 0.5 s at 8 / 16 kHz.

The guards (conditions, not measurements): on every fixture the restatement of tests/marks_refs.py reaches none of the
status cases, every decision of it has a relative margin of at least 1e-6, and the reference's marks lie inside the
restatement's bounds.  Data only."""
import os
import sys
import warnings

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.environ.get("PYPEVOC_REFERENCE", "/root/reference"))

import numpy as np  # noqa: E402

warnings.simplefilter("ignore")
if not hasattr(np, "RankWarning"):
    np.RankWarning = np.exceptions.RankWarning

from pypevoc import Periodicity as per  # noqa: E402

import marks_refs as R  # noqa: E402

CAP = 300000


def save(fname, out):
    path = os.path.join(HERE, fname + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= CAP, (fname, size)
    print("%s: %d bytes" % (fname, size))


def main():
    out = {"sig_" + k: R.make_signal(k) for k in R.SIGNALS}
    out["cases"] = R.cases_json(R.CORR_FIXTURES)
    for c in R.CORR_FIXTURES:
        x = out["sig_" + c["sig"]].astype(np.float64)
        marks = per.period_marks_corr(x, sr=c["sr"], t0=c["t0"], tf=np.array(c["tf"]), f=np.array(c["f"]), window_size=c["W"],
                                      min_per=c["min_per"])
        r = R.corr_walk(x, c["sr"], c["t0"], c["tf"], c["f"], c["W"], c["min_per"])
        assert r.status == 0, (c["name"], r.status)
        worst = min((m for m in r.margins if not m.tagged), key=lambda m: m.value)
        assert worst.value >= R.MARGIN_FLOOR, (c["name"], worst)
        assert len(marks) == len(r.marks) and len(marks) >= 4, (c["name"], len(marks), len(r.marks))
        err = np.abs(marks - r.marks)
        assert np.all(err <= r.bounds), (c["name"], err.max(), r.bounds.max())
        out[c["name"] + "_marks"] = np.asarray(marks, dtype=np.float64)
        branch = sum(1 for s in r.steps if not s["delay_t"] > c["min_per"])
        print("%-10s %3d marks  %3d steps (%d by 1 / f0)  margin %.1e (%s)  reference against the restatement %.1e, bound %.1e"
              % (c["name"], len(marks), len(r.steps), branch, worst.value, worst.kind, err.max(), r.bounds.max()))
    save("K1_marks_corr", out)

    keys = sorted(set(c["sig"] for c in R.PEAK_FIXTURES))
    out = {"sig_" + k: R.make_signal(k) for k in keys}
    out["cases"] = R.cases_json(R.PEAK_FIXTURES)
    for c in R.PEAK_FIXTURES:
        x = out["sig_" + c["sig"]].astype(np.float64)
        f = R.peak_f(c, len(x))
        tf = None if c["tf"] is None else np.array(c["tf"])
        marks, vals = per.period_marks_peak(x, sr=c["sr"], tf=tf, f=np.array(f) if np.ndim(f) else f, fit_points=c["fit_points"])
        r = R.peak_walk(x, c["sr"], c["tf"], f, c["fit_points"], exact=False)
        assert r.status & ~R.SHORT_FIT == 0, (c["name"], r.status)
        assert len(marks) == len(r.marks) >= 4, (c["name"], len(marks), len(r.marks))
        keep = ~((r.idx >= len(x) - 2))                              # fewer than 3 fit points: the stated deviation
        assert np.array_equal(marks[keep], r.marks[keep]) and np.array_equal(np.asarray(vals)[keep], r.vals[keep]), c["name"]
        worst = min((m.value for m in r.margins), default=np.inf)
        assert worst >= R.MARGIN_FLOOR, (c["name"], worst)
        out[c["name"] + "_marks"], out[c["name"] + "_vals"] = np.asarray(marks, dtype=np.float64), np.asarray(vals, dtype=np.float64)
        print("%-12s %3d marks (%d fitted)  margin %.1e" % (c["name"], len(marks), int(r.fitted.sum()), worst))
    save("K2_marks_peak", out)


if __name__ == "__main__":
    main()

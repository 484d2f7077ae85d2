#!/usr/bin/env python
"""Measure the bar of tests/test_weights_gpu.py on the CPU: on the inputs of its comparison against the restatement (every
shape, length and target; weights and intercepts) the largest difference between the float64 and the extended-precision run of
tests/weights_ref.py, relative to max(1, max |w|) of the target.  The test's bar is 16 times that (the kernel's tree-order sums
differ from numpy's left-to-right order), floored at 1e-13; the figure printed here is the one in its docstring.

    python scripts/measure_weights_bar.py
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_weights_gpu as tw  # noqa: E402


def main():
    worst, where = 0.0, None
    cases = [(c, si) for si, c in enumerate(tw.CASES)] + [(tw.UNSPECIALISED + ("unspecialised",), len(tw.CASES))]
    for (N, K, family), si in cases:
        for ti, T in enumerate(tw.LENGTHS):
            _, full = tw._plan(si, ti)
            p = tw._data(N, K, T, 100 * N + T, full)
            t0 = time.perf_counter()
            for b in tw._compared(N, K):
                g64 = gld = None
                for what in ("series", "states"):
                    tg = tw._targets(p, what)
                    (w64, i64), g64 = tw._reference(p, b, tg, what, g64, dtype=np.float64)
                    (wld, ild), gld = tw._reference(p, b, tg, what, gld, dtype=np.longdouble)
                    for m in range(tg.shape[1]):
                        if np.isnan(ild[m]) or not np.isfinite(wld[m]).any():
                            continue
                        scale = max(1.0, float(np.nanmax(np.abs(wld[m]))))
                        diff = max(float(np.nanmax(np.abs(w64[m] - wld[m]))), abs(float(i64[m] - ild[m]))) / scale
                        if diff > worst:
                            worst, where = diff, (N, K, family, T, b, what, m)
            print("(%d,%d) %s T=%d: %.1f s, worst so far %.3g" % (N, K, family, T, time.perf_counter() - t0, worst), flush=True)
    print("MEASURED = %.3g at %s;  16 x = %.3g;  BAR = max(that, 1e-13) = %.3g" % (worst, where, 16 * worst, max(16 * worst, 1e-13)))


if __name__ == "__main__":
    main()

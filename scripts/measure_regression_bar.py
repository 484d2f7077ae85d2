#!/usr/bin/env python
"""Measure the bars of tests/test_regression_gpu.py on the CPU: on the inputs of its comparison against the restatement (every
shape, length, instance and effect list) the largest difference between the float64 and the extended-precision run of
tests/regress_ref.py -- the normal matrix A entrywise relative to sqrt(A_pp A_qq), and separately beta, cov and gain (which carry
the conditioning of S) relative to max(1, |value|).  The test's bars are 16 times these (the kernel's tree-order sums differ from
numpy's left-to-right order), floored at 1e-13; the figures printed here are the ones in its docstring, with the largest
condition number of the unit-diagonal S of the effects kept.

    python scripts/measure_regression_bar.py
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import regress_ref  # noqa: E402
import test_regression_gpu as tr  # noqa: E402


def main():
    worst_a, worst_s, worst_c = (0.0, None), (0.0, None), (0.0, None)
    cases = [(c, si) for si, c in enumerate(tr.CASES)] + [(tr.UNSPECIALISED + ("unspecialised",), len(tr.CASES))]
    for (N, K, family), si in cases:
        for ti, T in enumerate(tr.LENGTHS):
            _, full = tr._plan(si, ti)
            t_first = tr._t_first(si, ti)
            p = tr._data(N, K, T, 100 * N + T, full)
            t0 = time.perf_counter()
            for b in range(tr.B_):
                g64 = gld = None
                for M in (16, 3, 1):
                    ef = tr._effects(N, T, M)
                    r64, g64 = tr._reference(p, b, ef, t_first, g64, dtype=np.float64)
                    rld, gld = tr._reference(p, b, ef, t_first, gld, dtype=np.longdouble)
                    assert np.array_equal(r64["dropped"], rld["dropped"]) and np.array_equal(r64["support"], rld["support"])
                    da, ds = tr.differences(r64, rld)
                    cond = regress_ref.unit_condition(rld["normal"], rld["dropped"])
                    where = (N, K, family, T, b, M)
                    worst_a, worst_s, worst_c = max(worst_a, (da, where)), max(worst_s, (ds, where)), max(worst_c, (cond, where))
            print("(%d,%d) %s T=%d t_first=%d: %.1f s, worst so far A %.3g, solve %.3g, condition %.3g"
                  % (N, K, family, T, t_first, time.perf_counter() - t0, worst_a[0], worst_s[0], worst_c[0]), flush=True)
    for name, (worst, where) in (("MEASURED_A", worst_a), ("MEASURED_S", worst_s)):
        print("%s = %.3g at %s;  16 x = %.3g;  BAR = max(that, 1e-13) = %.3g" % (name, worst, where, 16 * worst, max(16 * worst, 1e-13)))
    print("largest condition number of the unit-diagonal S: %.3g at %s" % worst_c)


if __name__ == "__main__":
    main()

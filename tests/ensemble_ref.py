"""Test infrastructure: the numpy restatement of the WINDOW STATISTICS of posterior draws (metran_amd/csrc/ensemble_kernels.hip,
include/metran_hip.h "WINDOW STATISTICS") -- the contract every kernel, entry point and accessor of the feature is tested
against.  The order of every sum is part of the definition (increasing t, increasing s), so the path functionals of a kernel
are expected to be bit-identical to these and the ensemble summary to differ by fused multiply-adds only.

``wrong=`` names one deliberate mistake (tests/test_window_stats_host.py shows that the tests can see each of them):
``long_start`` / ``long_stop`` a window one step long at either end, ``le`` ``<=`` for ``<``, ``carry`` a spell carried across a
window's edge, ``nan_counted`` a NaN path counted (its NaN steps skipped), ``m_divisor`` m for m - 1, ``ceil`` ceil for floor."""
import numpy as np

NF = 5
FUNCTIONALS = ("mean", "min", "max", "fraction_below", "longest_spell")
STATISTICS = ("count", "mean", "sd", "min", "max")


def path_functionals(paths, windows, thresholds=None, wrong=None):
    """``paths [S,B,T,Wd]``, ``windows`` int ``[R,W,2]`` half-open step ranges per record ``r = i % R`` (sorted, not overlapping,
    ``0 <= a <= b <= T``), ``thresholds [R,Wd]`` or None -> ``[S,B,Wd,W,5]``: mean (adds in increasing t, one division), min,
    max, fraction of steps below the level, longest spell below it.  An empty window, or one holding a NaN, is NaN in all
    five; a NaN or absent level makes the last two NaN."""
    paths = np.asarray(paths, dtype=np.float64)
    windows = np.asarray(windows, dtype=np.int64)
    S, B, T, Wd = paths.shape
    R, W = windows.shape[:2]
    thr = np.full((R, Wd), np.nan) if thresholds is None else np.asarray(thresholds, dtype=np.float64).reshape(R, Wd)
    out = np.full((S, B, Wd, W, NF), np.nan)
    for r in range(R):
        c = thr[r]                                   # [Wd]
        run = np.zeros((S, len(range(r, B, R)), Wd))  # the spell the walk is in (reset at every window unless wrong="carry")
        for w in range(W):
            a, b = int(windows[r, w, 0]), int(windows[r, w, 1])
            if wrong == "long_start":
                a = max(a - 1, 0)
            if wrong == "long_stop":
                b = min(b + 1, T)
            if wrong != "carry":
                run = np.zeros_like(run)
            if b <= a:
                continue
            y = paths[:, r::R, a:b, :]               # [S,Bi,L,Wd]
            L = b - a
            holds_nan = np.isnan(y).any(axis=2)
            if wrong == "nan_counted":
                y = np.where(np.isnan(y), 0.0, y)
            total = y[:, :, 0, :].copy()
            for t in range(1, L):
                total = total + y[:, :, t, :]
            under = (y <= c) if wrong == "le" else (y < c)
            longest = np.zeros_like(run)
            for t in range(L):
                run = np.where(under[:, :, t, :], run + 1.0, 0.0)
                longest = np.maximum(longest, run)
            level = np.broadcast_to(~np.isnan(c), total.shape)
            five = np.stack([total / float(L), y.min(axis=2), y.max(axis=2),
                             np.where(level, under.sum(axis=2) / float(L), np.nan), np.where(level, longest, np.nan)], axis=-1)
            if wrong != "nan_counted":
                five = np.where(holds_nan[..., None], np.nan, five)
            out[:, r::R, :, w, :] = five
    return out


def ensemble_summary(values, probs, wrong=None):
    """``values [S,cells]`` -> ``[cells, 5 + P]``: over the FINITE values of a cell in increasing s -- count m, mean
    (sequential sum / m), sd (two-pass, divisor m - 1, NaN if m < 2), min, max -- then the "linear" quantile of every
    probability: h = (m - 1) p, lo = floor(h), q = z_lo + (h - lo) (z_min(lo+1, m-1) - z_lo) on the sorted finite values."""
    values = np.asarray(values, dtype=np.float64)
    probs = np.asarray(probs, dtype=np.float64).reshape(-1)
    S, cells = values.shape
    out = np.full((cells, 5 + probs.size), np.nan)
    for cell in range(cells):
        x = values[:, cell]
        x = x[np.isfinite(x)]
        m = x.size
        out[cell, 0] = m
        if m == 0:
            continue
        mean = np.cumsum(x)[-1] / float(m)           # cumsum adds one after the other (np.sum adds pairwise)
        out[cell, 1] = mean
        if m > 1:
            d = x - mean
            out[cell, 2] = np.sqrt(np.cumsum(d * d)[-1] / float(m if wrong == "m_divisor" else m - 1))
        out[cell, 3], out[cell, 4] = x.min(), x.max()
        z = np.sort(x)
        h = float(m - 1) * probs
        lo = (np.ceil(h) if wrong == "ceil" else np.floor(h))
        hi = np.minimum(lo + 1, m - 1).astype(np.int64)
        lo = np.minimum(lo, m - 1).astype(np.int64)
        out[cell, 5:] = z[lo] + (h - np.floor(h)) * (z[hi] - z[lo])
    return out


def same_bits(a, b):
    """True when two float64 arrays agree bit for bit, every NaN taken for the same one."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64)))


# ---- the synthetic inputs shared by the CPU tier (host emulation) and the GPU tier (raw ABI) ----
def window_sets(T, R=3):
    """Three window sets ``[R,W,2]`` for ``T`` steps: W = 1 (``[0,T)`` for every record), W = 5, and W = 1 again with one late
    window (the last quarter: the walk has nothing to read before it).  In the set of five record 0 has the window
    ``[0,T)`` and trailing ``(T,T)`` pads, record 1 an empty window, a one-step window, gaps and a window ending at T, and the
    other records five windows that tile ``[0,T)`` (some of them empty when T < 5)."""
    one = np.tile(np.array([[0, T]], dtype=np.int64), (R, 1, 1))
    five = np.full((R, 5, 2), T, dtype=np.int64)
    five[0, 0] = (0, T)
    c1 = min(3, T)
    c2 = max(c1, T // 2)
    c3 = max(c2, T - max(1, T // 3))
    five[1] = [(0, 0), (0, 1), (c1, c2), (c3, T), (T, T)]
    edges = np.rint(np.linspace(0, T, 6)).astype(np.int64)
    for r in range(2, R):
        five[r] = np.stack([edges[:-1], edges[1:]], axis=1)
    late = np.tile(np.array([[T - T // 4, T]], dtype=np.int64), (R, 1, 1))
    return [one, five, late]


def synthetic_paths(S, B, T, Wd, R=3, seed=0):
    """``(paths [S,B,T,Wd], thresholds [R,Wd])``: random paths with one planted NaN (last draw, instance 5, step T // 2, last
    column: inside a window of either set); levels near the paths' median with a NaN in one column of record 1 and, in record 0's last column, a level that
    EQUALS a path value (draw 0, instance 0, step 0) exactly."""
    rng = np.random.default_rng(seed + 1000 * T + Wd)
    paths = rng.standard_normal((S, B, T, Wd))
    thr = 0.3 * rng.standard_normal((R, Wd))
    thr[1, 0] = np.nan
    thr[0, Wd - 1] = paths[0, 0, 0, Wd - 1]
    paths[S - 1, min(5, B - 1), T // 2, Wd - 1] = np.nan
    return paths, thr


PROBS = (0.0, 0.025, 0.5, 0.975, 1.0)


def summary_values(S, seed=0):
    """``values [S,cells]`` with the cells that matter: random, all equal, ties, NaNs (and an infinity) among the values, all
    NaN, exactly one finite value, and values of very different magnitude."""
    rng = np.random.default_rng(seed + S)
    cols = [rng.standard_normal(S), np.full(S, 1.25), np.round(rng.standard_normal(S) * 2.0) / 2.0, rng.standard_normal(S),
            np.full(S, np.nan), np.full(S, np.nan), rng.standard_normal(S) * 10.0 ** rng.integers(-3, 4, S), rng.standard_normal(S)]
    cols[3][rng.random(S) < 0.4] = np.nan
    cols[3][S // 2] = np.inf
    cols[5][S - 1] = -0.75
    cols[7][0] = np.nan
    return np.stack(cols, axis=1)


def summary_bar(values):
    """Per cell ``m * 2^-52 * max|x|`` over its finite values: one rounding per summand of the sd's and the quantile's sums, a
    fused multiply-add allowed.  0 for a cell without finite values."""
    x = np.where(np.isfinite(values), np.abs(values), 0.0)
    return np.isfinite(values).sum(axis=0) * 2.0 ** -52 * x.max(axis=0)

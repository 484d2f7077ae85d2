"""The residual diagnostics WITHOUT a GPU: the longdouble restatement and its bars (tests/resid_ref.py) against float64
restatements in the two summation orders a kernel may use, deliberately wrong variants shown to be far outside the bars, the
facade's formulas against scipy and a hand-built case, the calibration of the p-values on simulated white noise, the facade
over a stand-in engine (tests/resid_engine.py) and the binding of the two entry points."""
import functools
import itertools
import os
import re

import numpy as np
import pytest

import resid_ref as R
from batch_standin import stand_in, two_models
from metran_amd import residuals  # noqa: F401  (the feature under test: without it nothing here means anything)
from resid_engine import ResidEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = np.float64


@functools.lru_cache(maxsize=None)
def _series_cases():
    return R.check_decisive(R.series_cases())


@functools.lru_cache(maxsize=None)
def _cross_cases():
    return R.cross_cases()


# ---------------------------------------------------------------------------------- float64 restatements in two orders
def _tree(x):
    """The xor-butterfly sum over the 64 lanes of a tile: halves added onto each other."""
    x = np.array(x, dtype=F64)
    while len(x) > 1:
        x = x[: len(x) // 2] + x[len(x) // 2:]
    return x[0]


def _scan(x):
    """Hillis-Steele inclusive prefix sum over 64 lanes."""
    x = np.array(x, dtype=F64)
    off = 1
    while off < 64:
        y = np.concatenate([np.zeros(off), x[:-off]])
        x = np.where(np.arange(64) >= off, x + y, x)
        off *= 2
    return x


def _series64(v, f, t_first, tiles):
    """[N,12] in float64: ``tiles=False`` one accumulator in ascending time; ``tiles=True`` a tree per 64-step tile and the
    tiles in sequence, prefix scans per tile plus a carry; ``tiles="lanes"`` the kernel's own order of the totals: one
    accumulator per lane over its steps of all tiles, then one tree."""
    T, N = v.shape
    ok = R.valid_cells(v, f, t_first)
    out = np.full((N, 12), np.nan)
    Tp = -(-T // 64) * 64
    for j in range(N):
        o = np.zeros(Tp, dtype=bool)
        o[:T] = ok[:, j]
        e = np.zeros(Tp)
        e[:T][ok[:, j]] = v[ok[:, j], j] / np.sqrt(f[ok[:, j], j])
        m = int(o.sum())
        out[j, 0], out[j, 5] = m, 0
        if m == 0:
            continue
        pos = np.cumsum(o)                       # 1-based position among the valid cells
        h = (m + 1) // 3

        def total(x):
            if tiles == "lanes":                 # a lane per step of a tile adds its own steps, then one tree over the lanes
                acc = np.zeros(64)
                for t0 in range(0, Tp, 64):
                    acc = acc + x[t0:t0 + 64]
                return _tree(acc)
            if tiles:
                s = F64(0)
                for t0 in range(0, Tp, 64):
                    s = s + _tree(x[t0:t0 + 64])
                return s
            s = F64(0)
            for val in x[o]:
                s = s + val
            return s

        def running(x):
            if tiles:
                c, carry = np.zeros(Tp), F64(0)
                for t0 in range(0, Tp, 64):
                    c[t0:t0 + 64] = carry + _scan(x[t0:t0 + 64])
                    carry = c[t0 + 63]
                return c
            c = np.zeros(Tp)
            c[o] = np.cumsum(x[o])               # numpy's cumsum is sequential
            return c

        mean = total(e) / F64(m)
        d = np.where(o, e - mean, 0.0)
        S2 = total(d * d)
        C, Q = running(d), running(d * d)
        xc = np.where(o, np.abs(C), -1.0)
        xq = np.where(o, np.abs(Q - (pos.astype(F64) / F64(m)) * S2), -1.0)
        out[j] = [m, mean, S2, total(d * d * d), total((d * d) * (d * d)), h, total(np.where(o & (pos <= h), e * e, 0.0)),
                  total(np.where(o & (pos > m - h), e * e, 0.0)), xc.max(), int(np.argmax(xc)), xq.max(), int(np.argmax(xq))]
    return out


def _cross64(v, f, L, t_first, stats):
    """(counts, sums) in float64 from the float64 statistics rows: ascending time, one accumulator per (lag, i, j)."""
    T, N = v.shape
    ok = R.valid_cells(v, f, t_first)
    live = (stats[:, 0] > 0) & (stats[:, 2] > 0)
    ok &= live[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        sd = np.sqrt(stats[:, 2] / stats[:, 0])
        Z = np.where(ok, (v / np.sqrt(np.where(ok, f, 1.0)) - stats[None, :, 1]) / sd[None, :], 0.0)
    counts, sums = np.zeros((L + 1, N, N), dtype=np.int64), np.zeros((L + 1, N, N))
    for l in range(L + 1):
        for t in range(l, T):
            sums[l] = sums[l] + np.outer(Z[t], Z[t - l])
            counts[l] += np.outer(ok[t], ok[t - l])
    pair = live[:, None] & live[None, :]
    return np.where(pair, counts, 0), np.where(pair, sums, np.nan)


_inside, check_series, TIMES = R.inside, R.check_series, R.TIMES


@pytest.mark.parametrize("tiles", [False, True, "lanes"], ids=["sequential", "tile_tree", "lane_accumulators"])
def test_float64_series_in_both_orders_is_inside_the_bars(tiles):
    for name, v, f in _series_cases():
        for b in range(v.shape[0]):
            for t_first in R.t_firsts(v.shape[1]):
                check_series(_series64(v[b], f[b], t_first, tiles), v[b], f[b], t_first, (name, b, t_first))


def test_float64_cross_is_inside_the_bars():
    for name, v, f, L in _cross_cases():
        for b in range(v.shape[0]):
            for t_first in (0, 1):
                st = _series64(v[b], f[b], t_first, True)
                counts, sums = _cross64(v[b], f[b], L, t_first, st)
                wc, ws, bars = R.cross(v[b], f[b], L, t_first, detail=True)
                assert np.array_equal(counts, wc), (name, b, t_first)
                _inside(sums, ws, bars, (name, b, t_first))


# ------------------------------------------------------------------------------------------------ the tests can fail
def _series_wrong_cases():
    """The cases a wrong series variant is shown on: records with gaps and more than a tile."""
    return [(n, v, f) for n, v, f in _series_cases() if n.endswith("miss50") and v.shape[1] >= 63]


@pytest.mark.parametrize("variant,cols", [("uncentred", [R.S2, R.S3, R.S4, R.CUSUM, R.CUSQ]), ("calendar_thirds", [R.SS_FIRST, R.SS_LAST]),
                                          ("h_floor", [R.H, R.SS_FIRST, R.SS_LAST])])
def test_wrong_series_variants_are_far_outside_the_bars(variant, cols):
    cases = _series_wrong_cases()
    assert len(cases) >= 4
    for name, v, f in cases:
        far = 0.0
        for b, t_first in itertools.product(range(v.shape[0]), range(6)):   # some t_first leaves m = 2 mod 3, where h differs
            want, bars, _ = R.series(v[b], f[b], t_first, detail=True)
            bad = R.series(v[b], f[b], t_first, variant=variant)
            for c in cols:
                diff = np.abs(bad[:, c] - want[:, c])
                bar = np.where(bars[:, c] > 0, bars[:, c], R.LD(1e-300))   # an exact column: any difference is beyond every bar
                far = max(far, float(np.nanmax(diff / bar)))
        assert far >= 1000, (variant, name, far)


def test_last_step_on_a_tie_is_a_different_answer():
    v, f = R.tie_model()
    want, bad = R.series(v[0], f[0], 0), R.series(v[0], f[0], 0, variant="last_tie")
    assert list(want[:, R.CUSUM_T]) == [2, 3] and list(want[:, R.CUSQ_T]) == [2, 9]
    assert list(bad[:, R.CUSUM_T]) == [30, 64] and list(bad[:, R.CUSQ_T]) == [32, 65]
    for tiles in (False, True, "lanes"):   # the float64 restatements keep the first
        got = _series64(v[0], f[0], 0, tiles)
        assert np.array_equal(got[:, TIMES], want[:, TIMES].astype(F64))


@pytest.mark.parametrize("variant", ["lag_sign", "compacted", "m_minus_1", "no_t_first"])
def test_wrong_cross_variants_are_far_outside_the_bars(variant):
    cases = [c for c in _cross_cases() if c[3] >= 1 and c[1].shape[1] >= 33 and c[1].shape[2] >= 2]
    assert len(cases) >= 8
    for name, v, f, L in cases:
        far = 0.0
        for b in range(v.shape[0]):
            wc, ws, bars = R.cross(v[b], f[b], L, 2, detail=True)
            bc, bs = R.cross(v[b], f[b], L, 2, variant=variant)
            if variant == "no_t_first":      # the counts are compared exactly: any difference is a failure
                far = max(far, 1e300 if not np.array_equal(bc, wc) else 0.0)
                continue
            fin = np.isfinite(ws.astype(F64)) & (bars > 0)
            far = max(far, float(np.max(np.abs(bs - ws)[fin] / bars[fin])))
        assert far >= 1000, (variant, name, far)


# ------------------------------------------------------------------------------------------------------ formula pins
def test_normality_is_scipys_jarque_bera():
    from scipy import stats as sps

    from metran_amd.residuals import normality

    rng = np.random.default_rng(3)
    e = rng.standard_t(5, size=(400, 3))
    st = R.series(e, np.ones_like(e)).astype(F64)
    got = normality(st)
    for j in range(3):
        jb = sps.jarque_bera(e[:, j])
        assert got["nobs"][j] == 400
        np.testing.assert_allclose(got["skew"][j], sps.skew(e[:, j]), rtol=1e-12)
        np.testing.assert_allclose(got["kurtosis"][j], sps.kurtosis(e[:, j], fisher=False), rtol=1e-12)
        np.testing.assert_allclose(got["JB"][j], jb.statistic, rtol=1e-11)
        np.testing.assert_allclose(got["pvalue"][j], jb.pvalue, rtol=1e-9, atol=1e-300)
        ref = R.normality(R.series(e, np.ones_like(e))[j])
        np.testing.assert_allclose([got[k][j] for k in ("skew", "kurtosis", "JB", "pvalue")], ref[1:], rtol=1e-11)


def test_heteroskedasticity_formulas():
    from scipy.special import kolmogorov
    from scipy.stats import f as fdist

    from metran_amd.residuals import heteroskedasticity

    rng = np.random.default_rng(4)
    e = rng.normal(size=(100, 2))
    e[60:, 1] *= 2.0
    e[rng.random((100, 2)) < 0.2] = np.nan
    st = R.series(e, np.ones_like(e)).astype(F64)
    got = heteroskedasticity(st)
    for j in range(2):
        x = e[np.isfinite(e[:, j]), j]
        m = len(x)
        h = (m + 1) // 3
        H = np.sum(x[m - h:] ** 2) / np.sum(x[:h] ** 2)
        assert got["nobs"][j] == m and got["h"][j] == h
        np.testing.assert_allclose(got["H"][j], H, rtol=1e-12)
        np.testing.assert_allclose(got["pvalue"][j], 2 * min(fdist.cdf(H, h, h), fdist.sf(H, h, h)), rtol=1e-10)
        d = x - x.mean()
        s = np.sqrt(np.mean(d * d))
        # the scaling of the two bridges: partial sums over sigma sqrt(m), and of squares over sqrt(2 m) sigma^2
        cs = np.max(np.abs(np.cumsum(d))) / (s * np.sqrt(m))
        cq = np.max(np.abs(np.cumsum(d * d) - np.arange(1, m + 1) / m * np.sum(d * d))) / (np.sqrt(2.0 * m) * s * s)
        np.testing.assert_allclose([got["cusum"][j], got["cusumsq"][j]], [cs, cq], rtol=1e-11)
        np.testing.assert_allclose([got["cusum_pvalue"][j], got["cusumsq_pvalue"][j]], [kolmogorov(cs), kolmogorov(cq)], rtol=1e-9)
        steps = np.nonzero(np.isfinite(e[:, j]))[0]
        assert got["cusum_step"][j] == steps[np.argmax(np.abs(np.cumsum(d)))]
        ref = R.heteroskedasticity(R.series(e, np.ones_like(e))[j])
        keys = ("nobs", "h", "H", "pvalue", "cusum", "cusum_step", "cusum_pvalue", "cusumsq", "cusumsq_step", "cusumsq_pvalue")
        np.testing.assert_allclose([got[k][j] for k in keys], ref, rtol=1e-10)
    assert got["pvalue"][1] < 0.01 < got["pvalue"][0]
    # kolmogorov is the law of sup |Brownian bridge|: its 5 % point is 1.358
    assert abs(kolmogorov(1.3581) - 0.05) < 1e-4


def test_cross_correlation_bookkeeping_on_three_series():
    """A observed on even steps only, B on odd steps only, C always: n_AB(0) = 0 is no term of Q, n_AB(1) > 0 is."""
    from scipy.stats import chi2

    from metran_amd.residuals import correlations, cross_correlation

    T = 60
    rng = np.random.default_rng(8)
    e = rng.normal(size=(T, 3))
    e[1::2, 0] = np.nan
    e[0::2, 1] = np.nan
    counts, sums = R.cross(e, np.ones_like(e), 1)
    assert counts[0, 0, 1] == 0 == counts[0, 1, 0] and counts[1, 0, 1] == 29 and counts[1, 1, 0] == 30
    assert counts[0, 0, 2] == 30 and counts[0, 2, 2] == 60 and counts[1, 2, 2] == 59 and counts[1, 0, 0] == 0
    got = cross_correlation(counts, sums.astype(F64), min_pairs=20)
    # lag 0: AC, BC (AB never overlaps); lag 1: AB, BA, AC, CA, BC, CB
    assert got["df"] == 8
    z = {}
    ok = np.isfinite(e)
    Z = np.where(ok, (e - np.nanmean(e, axis=0)) / np.nanstd(e, axis=0), 0.0)
    Q = 0.0
    for l, a, b in [(0, 0, 2), (0, 1, 2), (1, 0, 1), (1, 1, 0), (1, 0, 2), (1, 2, 0), (1, 1, 2), (1, 2, 1)]:
        n = np.sum(ok[l:, a] & ok[:T - l, b])
        r = np.sum(Z[l:, a] * Z[:T - l, b]) / n
        z[(a, b, l)] = r * np.sqrt(n)
        Q += n * r * r
    np.testing.assert_allclose(got["Q"], Q, rtol=1e-12)
    np.testing.assert_allclose(got["pvalue"], chi2.sf(Q, 8), rtol=1e-10)
    worst = max(z, key=lambda k: abs(z[k]))
    assert got["worst"][:3] == worst and abs(got["worst"][4] - z[worst]) < 1e-12
    ref = R.cross_test(counts, sums, 20)
    np.testing.assert_allclose([got["Q"], got["df"], got["pvalue"]], ref[:3], rtol=1e-11)
    assert got["worst"][:3] == ref[3][:3]
    assert cross_correlation(counts, sums.astype(F64), min_pairs=30)["df"] == 5     # AC(0), BC(0), BA(1), CA(1), BC(1) have 30 steps
    none = cross_correlation(counts, sums.astype(F64), min_pairs=31)
    assert none["df"] == 0 and np.isnan(none["Q"]) and np.isnan(none["pvalue"]) and none["worst"] is None
    r0 = correlations(counts, sums.astype(F64))
    assert np.isnan(r0[0, 0, 1]) and abs(r0[0, 2, 2] - 1.0) < 1e-12


# ----------------------------------------------------------------------------------------- calibration of the p-values
def _white(seed, n, T=300, missing=0.3):
    rng = np.random.default_rng(seed)
    e = rng.normal(size=(T, n))
    gap = rng.random((T, n)) < missing
    return e, gap


def _share(p, level=0.05):
    p = np.asarray(p)
    assert np.isfinite(p).all()
    return float(np.mean(p < level)), 4.0 * np.sqrt(level * (1 - level) / len(p))


@functools.lru_cache(maxsize=None)
def _white_stats():
    e, gap = _white(2024, 2000)
    return R.series(np.where(gap, np.nan, e), np.ones_like(e)).astype(F64)


def test_calibration_of_the_per_series_tests():
    from metran_amd.residuals import heteroskedasticity, normality

    st = _white_stats()
    het = heteroskedasticity(st)
    for name, p in (("JB", normality(st)["pvalue"]), ("H", het["pvalue"])):
        share, band = _share(p)
        print("share of %s pvalue < 0.05: %.4f (0.05 +- %.4f)" % (name, share, band))
        assert abs(share - 0.05) <= band, name
    for name in ("cusum_pvalue", "cusumsq_pvalue"):   # conservative on finite records: the upper side alone is a condition
        share, band = _share(het[name])
        print("share of %s < 0.05: %.4f (<= 0.05 + %.4f)" % (name, share, band))
        assert share <= 0.05 + band, name


def test_power_against_a_variance_doubling_and_a_level_shift():
    from metran_amd.residuals import heteroskedasticity

    e, gap = _white(77, 400)
    e2 = e.copy()
    e2[150:] *= np.sqrt(2.0)
    het = heteroskedasticity(R.series(np.where(gap, np.nan, e2), np.ones_like(e)).astype(F64))
    assert np.mean(het["pvalue"] < 0.05) > 0.5
    assert np.mean(het["cusumsq_pvalue"] < 0.05) > 0.5
    e3 = e.copy()
    e3[150:] += 0.5
    het = heteroskedasticity(R.series(np.where(gap, np.nan, e3), np.ones_like(e)).astype(F64))
    assert np.mean(het["cusum_pvalue"] < 0.05) > 0.5


def test_calibration_and_power_of_the_cross_correlation_test():
    from metran_amd.residuals import cross_correlation

    e, gap = _white(99, 4 * 500)
    rng = np.random.default_rng(100)
    common = rng.normal(size=(300, 500))
    p0, p1 = [], []
    for k in range(500):
        cols = slice(4 * k, 4 * k + 4)
        for p, x in ((p0, e[:, cols]), (p1, np.sqrt(0.7) * e[:, cols] + np.sqrt(0.3) * common[:, [k]])):
            v = np.where(gap[:, cols], np.nan, x)
            counts, sums = R.cross(v, np.ones_like(v), 5)
            p.append(cross_correlation(counts, sums.astype(F64), min_pairs=20)["pvalue"])
    share, band = _share(p0)
    print("share of Q pvalue < 0.05: %.4f (0.05 +- %.4f)" % (share, band))
    assert abs(share - 0.05) <= band
    assert np.mean(np.array(p1) < 0.05) > 0.9


# ---------------------------------------------------------------------------------------------------------- the facade
def _facade(cells=None):
    models, G = two_models()
    log = []
    mb = stand_in(lambda obs, loadings: ResidEngine(obs, loadings, log=log, cells=cells), models, G)
    alpha = np.full((2, 4), 8.0)
    return mb, alpha, log


def test_facade_frames_time_stamps_and_cache():
    import pandas as pd

    mb, alpha, log = _facade()
    norm, het, cross = mb.test_normality(alpha), mb.test_heteroskedasticity(alpha), mb.test_cross_correlation(alpha, nlags=2, min_pairs=5)
    assert [c for c, _ in log] == ["innovations", "residual_series", "residual_cross"]
    assert list(norm.columns) == ["nobs", "skew", "kurtosis", "JB", "pvalue"]
    assert list(het.columns) == ["nobs", "h", "H", "pvalue", "cusum", "cusum_time", "cusum_pvalue", "cusumsq", "cusumsq_time", "cusumsq_pvalue"]
    assert list(cross.columns) == ["Q", "df", "pvalue", "series_a", "series_b", "lag", "r", "z"]
    white = mb.test_whiteness(alpha, nlags=3)
    assert norm.index.equals(white.index) and het.index.equals(white.index)
    assert cross.index.name == "model" and list(cross.index) == [0, 1]
    v, f = (t.numpy() for t in mb.get_innovations(alpha, standardized=False))
    for r in range(2):
        st = R.series(v[r], f[r], 1)
        cc, cs = R.cross(v[r], f[r], 2, 1)
        q = R.cross_test(cc, cs, 5)
        np.testing.assert_allclose(cross.loc[r, ["Q", "df", "pvalue"]].values.astype(F64), q[:3], rtol=1e-10)
        names = mb.batch.names[r]
        assert (cross.loc[r, "series_a"], cross.loc[r, "series_b"], cross.loc[r, "lag"]) == (names[q[3][0]], names[q[3][1]], q[3][2])
        for j, name in enumerate(names):
            np.testing.assert_allclose(norm.loc[(r, name)].values.astype(F64), R.normality(st[j]), rtol=1e-10)
            ref = R.heteroskedasticity(st[j])
            row = het.loc[(r, name)]
            np.testing.assert_allclose(row[["nobs", "h", "H", "pvalue", "cusum", "cusum_pvalue", "cusumsq", "cusumsq_pvalue"]].values.astype(F64),
                                       [ref[i] for i in (0, 1, 2, 3, 4, 6, 7, 9)], rtol=1e-10)
            # the time stamps: the model's own index at the step of the excursion
            assert row["cusum_time"] == mb.batch.index[r][ref[5]] and row["cusumsq_time"] == mb.batch.index[r][ref[8]]
            assert isinstance(row["cusum_time"], pd.Timestamp)
        corr = mb.get_residual_correlations(r, lag=1, nlags=2, alpha=alpha)
        assert list(corr.index) == list(names) == list(corr.columns)
        np.testing.assert_allclose(corr.values, (cs[1] / cc[1]).astype(F64), rtol=1e-12)
    # a second call with the same parameters runs nothing again; other lags run the cross sums alone
    n = len(log)
    mb.test_normality(alpha), mb.test_heteroskedasticity(alpha), mb.test_cross_correlation(alpha, nlags=2, min_pairs=9)
    mb.get_residual_correlations(0, lag=0, nlags=2, alpha=alpha)
    assert len(log) == n
    mb.get_residual_correlations(0, lag=0, alpha=alpha)
    assert [c for c, _ in log[n:]] == ["residual_cross"]
    with pytest.raises(ValueError):
        mb.get_residual_correlations(0, lag=3, nlags=2, alpha=alpha)


def test_facade_honours_t_first():
    mb, alpha, log = _facade()
    v, f = (t.numpy() for t in mb.get_innovations(alpha, standardized=False))
    a, b = mb.test_normality(alpha, t_first=1), mb.test_normality(alpha, t_first=9)
    for r in range(2):
        for j, name in enumerate(mb.batch.names[r]):
            for frame, t_first in ((a, 1), (b, 9)):
                np.testing.assert_allclose(frame.loc[(r, name)].values.astype(F64), R.normality(R.series(v[r], f[r], t_first)[j]), rtol=1e-10)
    assert (a["nobs"].values > b["nobs"].values).all()
    c9 = mb.test_cross_correlation(alpha, nlags=1, min_pairs=5, t_first=9)
    q = R.cross_test(*R.cross(v[0], f[0], 1, 9), 5)
    np.testing.assert_allclose(c9.loc[0, ["Q", "df", "pvalue"]].values.astype(F64), q[:3], rtol=1e-10)


def test_facade_nan_rules_and_screen():
    """Known residuals behind the facade: model 0 = white noise but series s2 with a tenfold variance from mid-record; model 1 =
    s0 empty, s1 three cells, s2 constant."""
    rng = np.random.default_rng(12)
    T = 40
    v = rng.normal(size=(2, T, 3))
    v[0, 20:, 2] *= 10.0
    v[1, :, 0] = np.nan
    v[1, :, 1] = np.nan
    v[1, [3, 8, 20], 1] = [0.3, -1.0, 0.5]
    v[1, :, 2] = 0.5
    mb, alpha, log = _facade(cells=(v, np.ones_like(v)))
    norm, het = mb.test_normality(alpha), mb.test_heteroskedasticity(alpha)
    assert list(norm.loc[1]["nobs"]) == [0, 3, T - 1]
    assert norm.loc[1][["skew", "kurtosis", "JB", "pvalue"]].isna().all().all() and norm.loc[0].notna().all().all()
    dead = het.loc[1].loc[["s0", "s2"]]                       # three cells are enough for h = 1: s1 has its statistics
    assert dead[["H", "pvalue", "cusum", "cusum_pvalue", "cusumsq", "cusumsq_pvalue"]].isna().all().all()
    assert dead[["cusum_time", "cusumsq_time"]].isna().all().all() and het.loc[0].notna().all().all() and het.loc[(1, "s1")].notna().all()
    assert list(het.loc[1]["h"]) == [0, 1, (T - 1 + 1) // 3]
    cross = mb.test_cross_correlation(alpha, nlags=2, min_pairs=20)
    assert cross.loc[0, "df"] == 3 + 2 * 6 and cross.loc[1, "df"] == 0 and np.isnan(cross.loc[1, "Q"]) and np.isnan(cross.loc[1, "pvalue"])
    assert cross.loc[1, "series_a"] is None
    assert mb.test_cross_correlation(alpha, nlags=2, min_pairs=T).loc[0, "df"] == 0          # no pair has T common steps (t_first = 1)
    corr = mb.get_residual_correlations(1, alpha=alpha)           # s1 alone is live: its own lag-0 entry is 1
    assert abs(corr.loc["s1", "s1"] - 1.0) < 1e-12 and corr.isna().values.sum() == 8
    screen = mb.screen_residuals(alpha, nlags=3, level=0.01)
    assert list(screen.columns) == ["whiteness", "normality", "heteroskedasticity", "cross_correlation", "flag"]
    assert screen.index.equals(norm.index)
    assert screen.loc[(0, "s2"), "heteroskedasticity"] < 1e-4 and bool(screen.loc[(0, "s2"), "flag"])
    assert screen.loc[0]["cross_correlation"].nunique() == 1
    np.testing.assert_array_equal(screen["normality"].values, norm["pvalue"].values)
    assert not screen.loc[1]["flag"].any()                                                    # NaN p-values do not flag
    manual = (screen[["whiteness", "normality", "heteroskedasticity", "cross_correlation"]] < 0.01).any(axis=1)
    assert (screen["flag"] == manual).all()


# ---------------------------------------------------------------------------------------------------------- the binding
def test_the_two_entry_points_are_bound_as_the_header_declares_them():
    from metran_amd import _lib

    src = open(os.path.join(ROOT, "include", "metran_hip.h")).read()
    for name, nargs in (("mk_residual_series", 9), ("mk_residual_cross", 12)):
        proto = re.search(r"MK_API\s+[\w\s\*]+?\b%s\s*\((.*?)\);" % name, src, re.S)
        assert proto, "%s is not declared in the header" % name
        assert len(proto.group(1).split(",")) == len(_lib.API[name][1]) == nargs, name
    assert re.search(r"#define MK_ABI_VERSION 7\b", src) and _lib.ABI_VERSION == 7
    mk = open(os.path.join(ROOT, "metran_amd", "csrc", "Makefile")).read()
    assert "resid_kernels.hip" in mk and "resid_kernels.h" in mk

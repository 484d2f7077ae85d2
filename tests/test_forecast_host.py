"""The numpy restatement of the multi-step-ahead forecasts and the forecast skill (tests/forecast_ref.py), pinned WITHOUT a
GPU: to the oracle (the C restatement of seqkalmanfilter) run on records truncated after the origin, its three deliberately
wrong variants shown to be far outside every bar, the bars of the skill sums derived and shown to be ten times what float64
arithmetic uses, and the MetranBatch accessors over a stand-in engine that answers from the restatement."""
import os
import re

import numpy as np
import pytest

import forecast_ref
import oracle
from metran_amd.synthetic import make_dfm_batch

F64 = np.float64
ATOL_MEAN, RTOL_VAR = 1e-12, 1e-12   # the per-cell bars of tests/test_innovations_host.py: atol 1e-12 max(1, max |y|) on a mean, rtol on a variance
Z95 = 1.959963984540054
CHUNK = 32                            # kForecastChunk of forecast_kernels.h (tests/test_forecast_gpu.py runs T around it)


def _models():
    """(y, phi, q, G, R, x0, P0, H): shapes (3,1), (8,2), (13,4), with and without R / x0 / P0; an empty first step, an empty
    run, a never-observed series; the first has H >= T."""
    out = []
    for (N, K, T, seed, extra, H) in ((3, 1, 6, 21, False, 8), (8, 2, 24, 22, True, 9), (13, 4, 19, 23, True, 5)):
        d = make_dfm_batch(1, N, K, T, seed=seed, missing=0.3)
        y = d["obs"][0].copy()
        y[0] = np.nan                          # an empty first step
        if T > 8:
            y[4:8] = np.nan                    # an empty run
            y[:, N - 1] = np.nan               # a series that is never observed
            y[9] = np.where(np.isfinite(y[9]), y[9], 0.3)
            y[9, N - 1] = np.nan
        rng = np.random.default_rng(seed)
        n = N + K
        R = rng.uniform(0.05, 0.4, N) * (rng.random(N) < 0.6) if extra else None
        x0 = rng.normal(size=n) if extra else None
        A = rng.normal(size=(n, n))
        P0 = A @ A.T / n + 0.5 * np.eye(n) if extra else None
        out.append((y, d["phi"][0], d["q"][0], d["loadings"][0], R, x0, P0, H))
    return out


MODELS = _models()


def _oracle_prediction(y, phi, q, G, R, x0, P0, o, H):
    """The oracle's predicted moments at steps o + 1 .. o + H on the record whose steps after o are all missing (and which is
    long enough), projected: (m, s) [H,N]."""
    T, N = y.shape
    K = G.shape[1]
    n = N + K
    ym = np.full((max(T, o + 1 + H), N), np.nan)
    ym[: o + 1] = y[: o + 1]
    Z = np.concatenate([np.eye(N), G], axis=1)
    ob, oi, oc = oracle.set_observations(ym)
    Xp, Pp = oracle.seqkalmanfilter(ob, np.diag(phi), np.diag(q), Z, np.zeros(N) if R is None else R, oi, oc,
                                    np.zeros(n) if x0 is None else x0, np.eye(n) if P0 is None else P0)[5:7]
    rows = slice(o + 1, o + 1 + H)
    return (np.einsum("jn,tn->tj", Z, Xp[rows]),
            np.einsum("jn,tnm,jm->tj", Z, Pp[rows], Z) + (np.zeros(N) if R is None else R))


@pytest.mark.parametrize("m", range(len(MODELS)))
def test_reference_is_the_oracles_prediction_on_truncated_records(m):
    """For a set of origins o (-1, 0, inside and behind the empty run, T - 1): the oracle's filter on the record with every step
    after o missing gives, projected, the fan from o, the rows of the track whose origin is o and the (e, s) of every pair of o --
    at the per-cell bars of the innovations tier, for the float64 and the extended-precision restatement alike."""
    y, phi, q, G, R, x0, P0, H = MODELS[m]
    T, N = y.shape
    rng = np.random.default_rng(m)
    scale, offset = rng.uniform(0.5, 3.0, N), rng.normal(size=N)
    big = max(1.0, np.nanmax(np.abs(y)))
    th = min(3, T)
    for dtype in (F64, np.longdouble):
        for o in sorted({-1, 0, 1, 5, T // 2, T - 2, T - 1}):
            pm, pv = _oracle_prediction(y, phi, q, G, R, x0, P0, o, H)
            r = forecast_ref.forecast(y, phi, q, G, R, x0, P0, scale, offset, horizon=H, origin=o, track_horizon=th, t_first=0, dtype=dtype)
            # the table every output is read from: e = y - M and s = S of the pairs of this origin
            np.testing.assert_allclose(r["M"][o + 1, :H].astype(F64), pm, rtol=0, atol=ATOL_MEAN * big)
            np.testing.assert_allclose(r["S"][o + 1, :H].astype(F64), pv, rtol=RTOL_VAR, atol=0)
            fm, fv = pm * scale + offset, np.maximum(pv, 0.0) * scale ** 2
            np.testing.assert_allclose(r["fan_mean"].astype(F64), fm, rtol=0, atol=ATOL_MEAN * max(1.0, np.abs(fm).max()))
            np.testing.assert_allclose(r["fan_var"].astype(F64), fv, rtol=RTOL_VAR, atol=0)
            for t in range(T):
                if max(t - th, -1) == o:
                    np.testing.assert_allclose(r["track_mean"][t].astype(F64), fm[t - o - 1], rtol=0, atol=ATOL_MEAN * max(1.0, np.abs(fm).max()))
                    np.testing.assert_allclose(r["track_var"][t].astype(F64), fv[t - o - 1], rtol=RTOL_VAR, atol=0)
            for h in range(1, H + 1):
                t = o + h
                if 0 <= o and t <= T - 1:
                    for j in np.nonzero(np.isfinite(y[t]))[0]:
                        e, s = y[t, j] - pm[h - 1, j], pv[h - 1, j]
                        assert abs(float(r["ratio"][o, h - 1, j]) - e * e / s) <= (2 * abs(e) * ATOL_MEAN * big + e * e * RTOL_VAR) / s * 1.01 + 1e-24


@pytest.mark.parametrize("m", range(len(MODELS)))
def test_skill_counts_and_empty_rows(m):
    """The pair count is the number of finite y[t, j] with t_first + h <= t <= T - 1; a never-observed series and a horizon
    without pairs (h >= T - t_first) give six exact zeros."""
    y, phi, q, G, R, x0, P0, H = MODELS[m]
    T, N = y.shape
    for t_first in (0, 1, T - 1, T):
        r = forecast_ref.forecast(y, phi, q, G, R, x0, P0, horizon=H, t_first=t_first)
        for j in range(N):
            for h in range(1, H + 1):
                cnt = int(np.isfinite(y[t_first + h:, j]).sum())
                assert r["skill"][j, h - 1, 0] == cnt
                assert r["skill"][j, h - 1, 5] <= cnt
                if cnt == 0:
                    assert (r["skill"][j, h - 1] == 0).all()
    if T > 8:
        assert (forecast_ref.forecast(y, phi, q, G, R, x0, P0, horizon=H)["skill"][N - 1] == 0).all()


def test_track_of_horizon_one_is_the_one_step_ahead_forecast():
    import innov_ref

    y, phi, q, G, R, x0, P0, H = MODELS[1]
    r = forecast_ref.forecast(y, phi, q, G, R, x0, P0, track_horizon=1)
    i = innov_ref.innovations(y, phi, q, G, R, x0, P0)
    assert np.array_equal(r["track_mean"], i["pred_mean"]) and np.array_equal(r["track_var"], i["pred_var"])


# ------------------------------------------------------------------------------------------------ the tests can fail
@pytest.mark.parametrize("m", range(len(MODELS)))
def test_wrong_variants_are_far_outside_the_bars(m):
    """origin_shift and q_once move the fan, the track and the sums; target_shift moves what it touches, the errors of the
    pairs (the sums) -- each by at least 1000 bars."""
    y, phi, q, G, R, x0, P0, H = MODELS[m]
    T = y.shape[0]
    big = max(1.0, np.nanmax(np.abs(y)))
    kw = dict(horizon=H, origin=T // 2, track_horizon=min(3, T), t_first=0)
    good = forecast_ref.forecast(y, phi, q, G, R, x0, P0, **kw)
    bars = forecast_ref.sum_bars(y, good["M"], good["S"], H, 0, ATOL_MEAN * big, RTOL_VAR)
    far = 1e3

    def sums_far(bad, cols):
        d = np.abs((bad["skill"] - good["skill"]).astype(F64))
        return all((d[:, :, c] > far * bars[:, :, c]).any() for c in cols)

    bad = forecast_ref.forecast(y, phi, q, G, R, x0, P0, origin_shift=True, **kw)
    assert float(np.max(np.abs(bad["fan_mean"] - good["fan_mean"]))) > far * ATOL_MEAN * big
    assert float(np.max(np.abs(bad["fan_var"] / good["fan_var"] - 1))) > far * RTOL_VAR
    assert float(np.max(np.abs(bad["track_mean"] - good["track_mean"]))) > far * ATOL_MEAN * big
    assert float(np.max(np.abs(bad["track_var"] / good["track_var"] - 1))) > far * RTOL_VAR
    assert sums_far(bad, (1, 2, 3, 4))
    bad = forecast_ref.forecast(y, phi, q, G, R, x0, P0, q_once=True, **kw)   # the means do not depend on q
    assert float(np.max(np.abs(bad["fan_var"] / good["fan_var"] - 1))) > far * RTOL_VAR
    assert float(np.max(np.abs(bad["track_var"] / good["track_var"] - 1))) > far * RTOL_VAR
    assert sums_far(bad, (3, 4))
    bad = forecast_ref.forecast(y, phi, q, G, R, x0, P0, target_shift=True, **kw)
    assert sums_far(bad, (1, 2, 3))


# ------------------------------------------------------------------------------------------------ sums and hits
@pytest.mark.parametrize("m", range(len(MODELS)))
def test_sum_bars_and_exact_hits(m):
    """The bars of the six sums (forecast_ref.sum_bars).  The innovations tier holds a mean to a = 1e-12 max(1, max |y|) and a
    variance to a relative r = 1e-12.  With e = y - m and the sums over the mu pairs of a (series, horizon):
        count, hits   exact (hits: see below)
        sum e         |d| <= mu a
        sum e^2       |d| <= sum (2 |e| a + a^2)
        sum e^2 / s   |d| <= sum ((2 |e| a + a^2) / s + (e^2 / s) r)          (first order in r)
        sum log s     |d| <= mu r                                            (|d log s| = r to first order)
    -- each pair's bound added over the pairs; the rounding of the additions themselves (mu <= 150 terms of float64) is two
    orders below.  The float64 restatement against the extended-precision one on the same inputs must use at most a TENTH of
    these (observed maximum of |difference| / bar over the three models and the five sums' cells: 0.0006).
      hits is compared exactly, which is a condition on the inputs: no pair of these models has e^2 / s within 1e-6 z^2 of the
    threshold z^2 (asserted here on the reference; a model that fails it gets another seed, not a wider window)."""
    y, phi, q, G, R, x0, P0, H = MODELS[m]
    big = max(1.0, np.nanmax(np.abs(y)))
    worst = 0.0
    for t_first in (0, 1):
        ref = forecast_ref.forecast(y, phi, q, G, R, x0, P0, horizon=H, t_first=t_first, z=Z95)
        f64 = forecast_ref.forecast(y, phi, q, G, R, x0, P0, horizon=H, t_first=t_first, z=Z95, dtype=F64)
        bars = forecast_ref.sum_bars(y, ref["M"], ref["S"], H, t_first, ATOL_MEAN * big, RTOL_VAR)
        d = np.abs((f64["skill"] - ref["skill"]).astype(F64))
        assert (d[:, :, (0, 5)] == 0).all()
        assert (d <= 0.1 * bars).all()
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bars > 0, d / bars, 0.0))))
        ratio = ref["ratio"][np.isfinite(ref["ratio"])].astype(F64)
        assert ratio.size and np.min(np.abs(ratio - Z95 ** 2)) >= 1e-6 * Z95 ** 2
    print("float64 against extended precision: worst |difference| / bar = %.3g" % worst)


def test_chunk_is_what_the_kernel_source_says():
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metran_amd", "csrc")
    assert re.search(r"constexpr int kForecastChunk = %d;" % CHUNK, open(os.path.join(here, "forecast_kernels.h")).read())
    src = open(os.path.join(here, "forecast_kernels.hip")).read()
    assert "o = c * kForecastChunk" in src and "forecast_max_horizon = 32;" in open(os.path.join(here, "forecast_kernels.h")).read()


# ---- MetranBatch over a stand-in engine ----
def test_metran_batch_accessors_over_a_stand_in_engine():
    """The engine answers ``forecast`` from forecast_ref (tests/forecast_engine.py)."""
    import pandas as pd
    from scipy.stats import norm

    from batch_standin import stand_in, two_models
    from forecast_engine import ForecastEngine
    from metran_amd.params import phi_q_from_alpha

    models, G = two_models()
    mb = stand_in(ForecastEngine, models, G)
    alpha = np.array([[8.0, 6.0, 9.0, 12.0], [5.0, 7.0, 8.0, 10.0]])
    phi, q = phi_q_from_alpha(alpha, G, 1.0)
    L = [int(v) for v in mb.batch.lengths]
    assert L[1] < L[0] == mb.T
    std, mean, yst = mb._std.numpy(), mb._mean.numpy(), mb.kf.obs_np
    H = 5
    ref = [forecast_ref.forecast(yst[r], phi[r], q[r], G[r], None, None, None, std[r], mean[r], horizon=H, origin=L[r] - 1,
                                 track_horizon=3, t_first=1, z=norm.ppf(0.95), dtype=F64) for r in range(2)]

    # the fan: from every model's own last real step, the index continues the record's, original / standardised units
    fm, fv = mb.get_forecast_means(H, alpha).numpy(), mb.get_forecast_variances(H, alpha).numpy()
    assert fm.shape == fv.shape == (2, H, 3) and mb.kf.calls == 1
    for r in range(2):
        np.testing.assert_array_equal(fm[r], ref[r]["fan_mean"])
        np.testing.assert_array_equal(fv[r], ref[r]["fan_var"])
        frame = mb.get_forecast(r, "s1", steps=H, alpha=alpha)
        assert list(frame.columns) == ["mean", "lower", "upper"] and frame.shape[0] == H
        assert frame.index.equals(pd.date_range(mb.batch.index[r][-1] + pd.Timedelta(days=1), periods=H, freq="D"))
        assert frame.index[0] - mb.batch.index[r][-1] == pd.Timedelta(days=1)
        np.testing.assert_array_equal(frame["mean"].values, fm[r, :, 1])
        half = norm.ppf(0.975) * np.sqrt(fv[r, :, 1])
        np.testing.assert_allclose(frame["upper"].values - frame["mean"].values, half, rtol=0, atol=1e-13)
        np.testing.assert_allclose(frame["mean"].values - frame["lower"].values, half, rtol=0, atol=1e-13)
        st = mb.get_forecast(r, "s1", steps=H, alpha=alpha, standardized=True)
        np.testing.assert_allclose(st["mean"].values, (fm[r, :, 1] - mean[r, 1]) / std[r, 1], rtol=0, atol=1e-14)
        np.testing.assert_allclose((st["upper"] - st["mean"]).values, half / std[r, 1], rtol=1e-13, atol=0)
        assert isinstance(mb.get_forecast(r, "s1", steps=H, alpha=alpha, ci=None), pd.Series)
    assert not mb.batch.index[0][-1] == mb.batch.index[1][-1]
    assert mb.kf.calls == 1 and "forecast" in mb._cache           # same parameter set and request: one engine call

    # the track, on the model's own index
    tr = mb.get_prediction_at(1, "s2", 3, alpha=alpha)
    assert mb.kf.calls == 2 and tr.shape[0] == L[1] and tr.index.equals(mb.batch.index[1])
    np.testing.assert_array_equal(tr["mean"].values, ref[1]["track_mean"][:L[1], 2])
    half = norm.ppf(0.975) * np.sqrt(ref[1]["track_var"][:L[1], 2])
    np.testing.assert_allclose((tr["upper"] - tr["mean"]).values, half, rtol=0, atol=1e-13)
    mb.get_prediction_at(0, "s0", 3, alpha=alpha)
    assert mb.kf.calls == 2
    mb.get_prediction_at(0, "s0", 2, alpha=alpha)                 # another request: another call, the first stays cached
    mb.get_forecast_means(H, alpha)
    assert mb.kf.calls == 3

    # the skill table against a direct pandas computation from the per-pair table
    sk = mb.forecast_skill(horizon=H, alpha=alpha, t_first=1, coverage=0.9)
    assert mb.kf.calls == 4 and list(sk.index.names) == ["model", "series", "horizon"] and len(sk) == 2 * 3 * H
    assert list(sk.columns) == ["nobs", "bias", "rmse", "msse", "logscore", "coverage", "nominal", "skill"]
    z = norm.ppf(0.95)
    for r in range(2):
        for j in range(3):
            for h in range(1, H + 1):
                t = np.arange(1 + h, mb.T)
                t = t[np.isfinite(yst[r, t, j])]
                pairs = pd.DataFrame({"e": yst[r, t, j] - ref[r]["M"][t - h + 1, h - 1, j], "s": ref[r]["S"][t - h + 1, h - 1, j]})
                row = sk.loc[(r, "s%d" % j, h)]
                assert row["nobs"] == len(pairs) > 0
                var = np.nanvar(yst[r, :, j])
                want = [pairs.e.mean() * std[r, j], np.sqrt((pairs.e ** 2).mean()) * std[r, j], (pairs.e ** 2 / pairs.s).mean(),
                        -0.5 * (np.log(2 * np.pi) + np.log(pairs.s).mean() + (pairs.e ** 2 / pairs.s).mean()),
                        (pairs.e ** 2 <= z * z * pairs.s).mean(), 0.9, 1.0 - (pairs.e ** 2).mean() / var]
                np.testing.assert_allclose(row.values[1:].astype(float), want, rtol=1e-11, atol=1e-12)
    mb.forecast_skill(horizon=H, alpha=alpha, t_first=1, coverage=0.9)
    assert mb.kf.calls == 4
    mb.forecast_skill(horizon=H, alpha=alpha * 1.01, t_first=1, coverage=0.9)
    assert mb.kf.calls == 5                                       # another parameter set: another run

    # no pairs: NaN columns, zero count
    none = mb.forecast_skill(horizon=2, alpha=alpha, t_first=mb.T)
    assert (none["nobs"] == 0).all() and none.drop(columns="nobs").isna().all().all()

    # argument errors
    with pytest.raises(KeyError):
        mb.get_forecast(0, "nope", alpha=alpha)
    with pytest.raises(ValueError):
        mb.get_forecast_means(33, alpha)
    with pytest.raises(ValueError):
        mb.get_forecast_means(0, alpha)
    with pytest.raises(Exception, match="must be between 0 and 1") as err:   # MetranBatch._band raises the reference's bare Exception
        mb.get_forecast(0, "s0", steps=3, alpha=alpha, ci=1.5)
    assert type(err.value) is Exception
    with pytest.raises(ValueError):
        mb.get_forecast_means(3)                                  # no parameters

"""GPU tier: the FITTING kernels under the property sweep of tests/hard_models.py (persistence up to 1 - 1e-9, communality up to
0.999, records that are 95 % missing, hold one observation, start or end with empty steps, never-observed series, R > 0,
non-default x0 / P0) -- the three routes whose own tiers feed them mild models only:

  regression   regress_replay_kernel behind the gain tape: eight effects per record chosen by rule from the record (a duplicate,
               effects without support among them), t_first 0 and 1 in turn -- two launches, each model compared under its own
  functionals  functional_walk_kernel over the device's own filtered and smoothed records: nine windows and four contrasts per
               record, against the longdouble walk from the oracle's records and, up to T (N + K) = 600, the dense definition
  scores       score_tangent_kernel / score_stats_kernel with Metran's chain rule for (dphi, dq), t_first 0 and 1 in turn

each against its numpy restatement in np.longdouble.  The bars are tests/hard_models.py's (regression_tolerances,
functional_tolerances, score_tolerances): the tier's own flat bar plus a MEASURED multiple of the reference algorithm's
conditioning (scripts/measure_diagnostic_bars.py); tests/test_property_fits.py first shows on the CPU that they hold between the
float64 and the longdouble restatement, that the second definitions hold, that every deliberately wrong variant is outside them,
and that the dropped sets and the walk's pivots are decided by the models, not by rounding.  Compared: the models of
tests/diagnostic_sweep.py::compared; the scores, whose restatement holds [n,n,n] longdouble arrays per cell, on
``score_compared`` (all up to N + K = 16, at most six per group above).  All three also run under the size-generic kernel family."""
import numpy as np
import pytest

import diagnostic_sweep as ds
import hard_models
from test_gpu_property_diagnostics import GENERIC_GROUPS, GENERIC_IDS, _engine, _np, _what, _Worst, jit_cache  # noqa: F401

pytestmark = pytest.mark.gpu

GROUPS, IDS = ds.GROUPS, ds.IDS
SCORE_KEYS = ("score", "grad", "opg", "cusum")


def _clean(status, route):
    """No status bit at all: the filter's two, and the smoothers' MK_FLAG_RANK_DEFICIENT / MK_FLAG_NOT_SPD, which
    functional_walk_kernel sets for a pivot <= 0 of its own factorisation (tests/test_property_fits.py: a float64 evaluation meets
    none on these models)."""
    st = _np(status)
    assert not st.any(), "%s: status %s at models %s" % (route, sorted(set(st[st != 0].tolist())), np.nonzero(st)[0].tolist())


# ------------------------------------------------------------------------------------------------ intervention effects
def _check_regression(key, g, kf, worst):
    N, K, T, B = key
    ef = ds.group_effects(g)
    assert ef.shape == (B, ds.M_EFFECTS, 4) and len({ef[b].tobytes() for b in range(B)}) > 1   # the lists differ between the records
    M = ds.M_EFFECTS
    for tf in (0, 1):
        res = kf.regression(g["phi"], g["q"], ef, t_first=tf, x0=g["x0"], P0=g["P0"])
        _clean(res["status"], "regression")
        got = {k: _np(res[k]) for k in ("beta", "cov", "gain", "normal", "support", "dropped")}
        assert got["normal"].shape == (B, M + 1, M + 1) and got["cov"].shape == (B, M, M)
        for b in ds.compared(key, g):
            if ds.t_first(b) != tf:
                continue
            rl = ds.regression(g, b)
            mine = {k: got[k][b] for k in ("beta", "cov", "gain", "normal", "support")}
            mine["dropped"] = np.array([(int(got["dropped"][b]) >> m) & 1 for m in range(M)], dtype=bool)
            tol = hard_models.regression_tolerances(g, b, ds.oracle_ref(g, b), rl)
            for name, err, bar in ds.regression_checks(mine, rl, tol, ds.regression_usable(g, b)):
                worst.check(err, bar, _what(g, b, "t_first", tf, name))


@pytest.mark.parametrize("key,g", GROUPS, ids=IDS)
def test_regression(key, g, jit_cache):  # noqa: F811
    kf = _engine(key, g)
    assert kf.regression_supported
    worst = _Worst("regression", key)
    _check_regression(key, g, kf, worst)
    worst.report()
    kf.close()


# ---------------------------------------------------------------------------------------------------- window functionals
def _check_functionals(key, g, kf, worst):
    N, K, T, B = key
    wins, ct = ds.group_windows(key, g), ds.group_contrasts(g)
    res = kf.functionals(g["phi"], g["q"], wins, ct, x0=g["x0"], P0=g["P0"])
    _clean(res["status"], "functionals")
    mean, var = _np(res["mean"]), _np(res["var"])
    assert mean.shape == var.shape == (B, wins.shape[1], ds.N_CONTRASTS)
    for b in ds.compared(key, g):
        bars = hard_models.functional_tolerances(g, b, ds.oracle_ref(g, b), ds.functional_reach(key, g, b))
        for name, err, bar in ds.functional_checks((mean[b], var[b]), ds.functional_walk(key, g, b), bars):
            worst.check(err, bar, _what(g, b, name))
        assert (var[b][np.isfinite(var[b])] >= 0).all(), _what(g, b)
        if ds.has_definition(key):
            for name, err, bar in ds.functional_checks((mean[b], var[b]), ds.functional_definition(key, g, b), bars):
                worst.check(err, bar, _what(g, b, name, "against the definition"))


@pytest.mark.parametrize("key,g", GROUPS, ids=IDS)
def test_functionals(key, g, jit_cache):  # noqa: F811
    kf = _engine(key, g)
    assert kf.functionals_supported
    worst = _Worst("functionals", key)
    _check_functionals(key, g, kf, worst)
    worst.report()
    kf.close()


# --------------------------------------------------------------------------------------------------------------- scores
def _check_scores(key, g, kf, worst):
    N, K, T, B = key
    dphi, dq = ds.group_derivs(g)
    for tf in (0, 1):
        res = kf.scores(g["phi"], g["q"], dphi, dq, t_first=tf, x0=g["x0"], P0=g["P0"])
        _clean(res["status"], "scores")
        got = {k: _np(res[k]) for k in SCORE_KEYS + ("count",)}
        assert got["score"].shape == (B, T, N + K) and got["cusum"].shape == (B, N + K, N + K)
        for b in ds.score_compared(key, g):
            if ds.t_first(b) != tf:
                continue
            sl = ds.scores(g, b)
            mine = {k: got[k][b] for k in SCORE_KEYS + ("count",)}
            empty = ~np.isfinite(g["obs"][b]).any(axis=1)
            assert (mine["score"][empty] == 0).all(), _what(g, b)
            tol = hard_models.score_tolerances(g, b, ds.oracle_ref(g, b), T)
            for name, err, bar in ds.score_checks(mine, sl, tol):
                worst.check(err, bar, _what(g, b, "t_first", tf, name))


@pytest.mark.parametrize("key,g", GROUPS, ids=IDS)
def test_scores(key, g, jit_cache):  # noqa: F811
    kf = _engine(key, g)
    assert kf.scores_supported
    worst = _Worst("scores", key)
    _check_scores(key, g, kf, worst)
    worst.report()
    kf.close()


# ---------------------------------------------------------------------------------------------- the size-generic family
@pytest.mark.parametrize("route", ["regression", "functionals", "scores"])
@pytest.mark.parametrize("key,g", GENERIC_GROUPS, ids=GENERIC_IDS)
def test_generic_family(key, g, route, jit_cache):  # noqa: F811
    """The three routes behind ``set_variant("kernel_family", "generic")`` (the size-generic recording pass and smoother feed
    them): the same checks at the same bars."""
    kf = _engine(key, g, "generic")
    worst = _Worst(route + " (generic family)", key)
    {"regression": _check_regression, "functionals": _check_functionals, "scores": _check_scores}[route](key, g, kf, worst)
    worst.report()
    kf.close()

"""CPU tier of the diagnostic routes' property sweep (tests/test_gpu_property_diagnostics.py): on the models the GPU tier compares,
  1. the float64 restatement of every route is inside the route's bar WITHOUT its safety factor against the longdouble
     restatement -- the bars are above what a correct float64 code does;
  2. the longdouble restatements agree with a second definition from the oracle's moments at the smoother's bar;
  3. every deliberately wrong variant of a restatement is outside the bar on at least one compared model of EVERY group --
     the bars can fail."""
import numpy as np
import pytest

import diagnostic_sweep as ds
import disturbance_ref
import hard_models

GROUPS, IDS = ds.GROUPS, ds.IDS


def test_flat_bars_are_the_tiers_own():
    import test_disturbance_gpu
    import test_draws_gpu
    import test_forecast_gpu
    import test_weights_gpu

    assert hard_models.RAW_TOL == test_disturbance_gpu.RAW_TOL
    assert (hard_models.FORECAST_ATOL_MEAN, hard_models.FORECAST_RTOL_VAR) == (test_forecast_gpu.ATOL_MEAN, test_forecast_gpu.RTOL_VAR)
    assert hard_models.WEIGHTS_BAR == test_weights_gpu.BAR
    assert (hard_models.DRAW_TOL, hard_models.PERTURB_TOL) == (test_draws_gpu.TOL, test_draws_gpu.PERTURB_TOL)
    assert hard_models.MARGIN == 4.0 and all(v is not None and v > 0 for v in hard_models.MEASURED.values())


def test_compared_models_cover_the_patterns():
    seen = set()
    for key, g in GROUPS:
        cmp_ = ds.compared(key, g)
        seen |= {g["patterns"][b] for b in cmp_}
        if key[0] + key[1] <= 16:
            assert cmp_ == list(range(key[3]))
        assert {b for b in range(key[3]) if g["phi"][b].max() > 1.0 - 1e-6} <= set(cmp_)
    assert seen == set(hard_models.PATTERNS)


@pytest.mark.parametrize("key,g", GROUPS, ids=IDS)
def test_float64_restatements_are_inside_the_bars_without_the_margin(key, g):
    for b in ds.compared(key, g):
        ref = ds.oracle_ref(g, b)
        what = (key, b, g["patterns"][b])
        (r64, n64), (rl, nl) = ds.dist(g, b, np.float64), ds.dist(g, b)
        tr, tn = hard_models.disturbance_tolerances(g, b, ref, rl, nl, margin=1.0)
        assert np.abs(r64 - rl).max() <= tr and np.abs(n64 - nl).max() <= tn, what
        f64, fl = ds.forecast(key, g, b, np.float64), ds.forecast(key, g, b)
        atol, rtol = hard_models.forecast_tolerances(g, b, ref, fl["M"], margin=1.0)
        for k in ("fan_mean", "track_mean", "M"):
            assert np.abs(f64[k] - fl[k]).max() <= atol, what + (k,)
        for k in ("fan_var", "track_var", "S"):
            assert np.abs(f64[k] / fl[k] - 1).max() <= rtol, what + (k,)
        for kind in ("series", "states"):
            (w64, i64), (wl, il) = ds.weights(g, b, kind, np.float64), ds.weights(g, b, kind)
            for m in range(wl.shape[0]):
                if np.isnan(il[m]):
                    assert np.isnan(i64[m]) and np.isnan(w64[m]).all()
                    continue
                tol = hard_models.weights_tolerance(g, b, ref, wl[m], kind, margin=1.0)
                assert abs(i64[m] - il[m]) <= tol, what + (kind, m)
                assert not np.isfinite(wl[m]).any() or np.nanmax(np.abs(w64[m] - wl[m])) <= tol, what + (kind, m)


@pytest.mark.parametrize("key,g", GROUPS, ids=IDS)
def test_second_definitions(key, g):
    """The longdouble restatements against the oracle's moments, each at the smoother's bar (a projection: times the largest
    absolute row sum of Z; the predicted moments of the truncated record: the filter's bar of THAT record)."""
    N, K, T, B = key
    for b in ds.compared(key, g):
        ref = ds.oracle_ref(g, b)
        tol = hard_models.smoother_tolerance(g, b, ref)
        rows = float((1.0 + np.abs(g["loadings"][b]).sum(1)).max())
        what = (key, b, g["patterns"][b])
        # disturbances: q r and q - q^2 N of the pair against the definition from the smoothed moments, t >= 1
        if T > 1:
            rl, nl = ds.dist(g, b)
            mean, var = disturbance_ref.moments(g["q"][b], rl.astype(np.float64), nl.astype(np.float64))
            dm, dv = ds.dist_definition(g, b)
            assert np.abs(mean - dm)[1:].max() <= tol and np.abs(var - dv)[1:].max() <= tol, what
        # weights: sum w y + intercept against the smoothed projection at the target
        for kind in ("series", "states"):
            tg = ds.targets(g, b, kind)
            wl, il = ds.weights(g, b, kind)
            total, want = ds.reconstruct(g, b, wl, il).astype(np.float64), ds.smoothed_at(g, b, kind, tg)
            ok = tg[:, 0] >= 0
            assert np.array_equal(np.isnan(total), ~ok), what
            assert (np.abs(total - want)[ok] <= (rows if kind == "series" else 1.0) * tol).all(), what + (kind,)
        # forecasts: the fan from the record's origin against the predicted moments of the record truncated there
        o = ds.origin(key, b)
        if o < T - 1:
            pm, pv, cut = ds.truncated_prediction(g, b, o)
            f = ds.forecast(key, g, b)
            h = pm.shape[0]
            ftol = rows * rows * max(hard_models.filter_tolerances(g, b, cut)[1], hard_models.smoother_tolerance(g, b, cut))
            assert np.abs(f["fan_mean"][:h].astype(np.float64) - pm).max() <= ftol, what
            assert np.abs(f["fan_var"][:h].astype(np.float64) - pv).max() <= ftol, what
        # draws: the mean of the antithetic pair against the smoothed projection
        for kind in ("series", "states"):
            d = ds.draws(g, b, kind)
            want = ref["S"] @ ref["Z"].T if kind == "series" else ref["S"]
            assert np.abs(0.5 * (d["draws"][0] + d["draws"][1]) - want).max() <= d["tol"].max(), what + (kind,)


def _dist_caught(key, g, b, variant):
    rl, nl = ds.dist(g, b)
    rw, nw = disturbance_ref.dist_adjoint(*ds.args(g, b), variant=variant, dtype=np.longdouble)
    tr, tn = hard_models.disturbance_tolerances(g, b, ds.oracle_ref(g, b), rl, nl)
    return np.abs(rw - rl).max() > tr or np.abs(nw - nl).max() > tn


def _forecast_caught(key, g, b, variant):
    import forecast_ref

    fl = ds.forecast(key, g, b)
    tab = forecast_ref.table(*ds.args(g, b), hmax=ds.HORIZON, **{variant: True})
    fw = forecast_ref.forecast(*ds.args(g, b), horizon=ds.HORIZON, origin=ds.origin(key, b), track_horizon=ds.track_horizon(key),
                               t_first=ds.T_FIRST, z=ds.Z95, tab=tab)
    atol, rtol = hard_models.forecast_tolerances(g, b, ds.oracle_ref(g, b), fl["M"])
    return any(np.abs(fw[k] - fl[k]).max() > atol for k in ("fan_mean", "track_mean")) or \
        any(np.abs(fw[k] / fl[k] - 1).max() > rtol for k in ("fan_var", "track_var"))


def _weights_caught(key, g, b, variant):
    B = key[3]
    for kind in ("series", "states"):
        wl, il = ds.weights(g, b, kind)
        if variant == "other_record":      # the targets of the next record: a kernel that reads one list for everybody
            ww, iw = ds.weights(g, b, kind, record=(b + 1) % B)
        else:
            ww, iw = ds.weights(g, b, kind, variant=variant)
        for m in range(wl.shape[0]):
            if np.isnan(il[m]):
                if not np.isnan(iw[m]):
                    return True
                continue
            tol = hard_models.weights_tolerance(g, b, ds.oracle_ref(g, b), wl[m], kind)
            if np.isnan(iw[m]) or abs(iw[m] - il[m]) > tol or (np.isfinite(wl[m]).any() and np.nanmax(np.abs(ww[m] - wl[m])) > tol):
                return True
    return False


WRONG = [("disturbances", v, _dist_caught) for v in ds.DIST_VARIANTS] + [("forecast", v, _forecast_caught) for v in ds.FORECAST_VARIANTS] + \
        [("weights", v, _weights_caught) for v in ds.WEIGHTS_VARIANTS + ("other_record",)]


@pytest.mark.parametrize("route,variant,caught", WRONG, ids=["%s-%s" % w[:2] for w in WRONG])
def test_wrong_variants_are_outside_the_bars_in_every_group(route, variant, caught):
    """A model with a single observation cannot see most variants, hence per group: the first compared model that tells."""
    for key, g in GROUPS:
        assert any(caught(key, g, b, variant) for b in ds.compared(key, g)), (route, variant, key)

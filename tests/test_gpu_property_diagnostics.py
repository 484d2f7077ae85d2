"""GPU tier: the DIAGNOSTIC kernels under the property sweep of tests/hard_models.py (persistence up to 1 - 1e-9, communality up
to 0.999, records that are 95 % missing, hold one observation, start or end with empty steps, never-observed series, R > 0,
non-default x0 / P0) -- the routes a user runs on a calibrated batch, which their own tiers feed typical models only:

  disturbances         disturbance mode of adjoint_kernel / adjoint_wide_kernel, with and without an update tape on the context
  forecast             forecast_kernels.hip: fan from an origin per record (-1 .. T - 1), track, the six skill sums
  observation_weights  gain mode of innov_step_kernel + weights_walk_kernel, target lists that differ between the records
  draw_smoothed        draw_kernels.hip around one smoothing pass per draw, an antithetic pair of series and of state draws
  innovations          tests/test_innovations_gpu.py::test_hard_models' comparison on every shape of the sweep

each against its numpy restatement in np.longdouble (draws: draw_ref.draw_model, the oracle's smoother) and against a second
definition from the oracle's moments.  The bars are tests/hard_models.py's: the tier's own flat bar plus a MEASURED multiple of
the reference algorithm's conditioning (scripts/measure_diagnostic_bars.py); tests/test_property_diagnostics.py first shows on
the CPU that they hold between the float64 and the longdouble restatement, that the second definitions hold, and that every
deliberately wrong variant of a restatement is outside them in every group.  Compared: every model of a group up to N + K = 16;
above, every third plus every model with a persistence above 1 - 1e-6 (tests/diagnostic_sweep.py keeps a model's references
across the routes).  The record readers and the draws also run under the size-generic kernel family on three shapes."""
import math

import numpy as np
import pytest

import diagnostic_sweep as ds
import disturbance_ref
import forecast_ref
import hard_models
import time_axis

pytestmark = pytest.mark.gpu

GROUPS, IDS = ds.GROUPS, ds.IDS
GENERIC = [(i, kg) for i, kg in enumerate(GROUPS) if kg[0][:2] in ds.GENERIC_SHAPES]
GENERIC_GROUPS, GENERIC_IDS = [kg for _, kg in GENERIC], [IDS[i] for i, _ in GENERIC]
FAN, TRACK = ("fan_mean", "fan_var"), ("track_mean", "track_var")
INNOVATION_OUTPUTS = ("v", "f", "pred_mean", "pred_var")


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    import os

    old = os.environ.get("METRAN_HIP_CACHE")
    if old is None:
        os.environ["METRAN_HIP_CACHE"] = str(tmp_path_factory.getbasetemp() / "mkjit")
    yield
    if old is None:
        os.environ.pop("METRAN_HIP_CACHE", None)


def _engine(key, g, family="specialised"):
    from metran_amd.engine import BatchedKalman

    N, K, T, B = key
    kf = BatchedKalman(0, layout="time_major" if (N + T) % 2 else "model_major")
    kf.set_observations(g["obs"]).set_loadings(g["loadings"], g["obsvar"])
    if family != "specialised":
        kf.set_variant("kernel_family", family)
    return kf


def _no_flags(status, what):
    from metran_amd.engine import FLAG_NONPOSITIVE_F, FLAG_NOT_SPD

    assert not (int(np.bitwise_or.reduce(_np(status).ravel())) & (FLAG_NONPOSITIVE_F | FLAG_NOT_SPD)), what


class _Worst:
    """The largest error of a route in units of its bar, and where: printed per test (the figures of the pull request)."""

    def __init__(self, route, key):
        self.route, self.key, self.ratio, self.where = route, key, 0.0, None

    def check(self, err, bar, what):
        err = float(err)
        if bar > 0 and err / bar > self.ratio:
            self.ratio, self.where = err / bar, what
        assert err <= bar, "%s: %.3g exceeds %.3g (%.2f of the bar)" % (what, err, bar, err / bar if bar > 0 else float("inf"))

    def report(self):
        print("diagnostic sweep, %s %dx%d T=%d B=%d: largest error %.3g of its bar at %s" % ((self.route,) + self.key + (self.ratio, self.where)))


def _what(g, b, *more):
    return " ".join(["model %d (%s, min q %.2g)" % (b, g["patterns"][b], g["q"][b].min())] + [str(m) for m in more])


def test_sweep_coverage():
    """Every missingness pattern of the generator is among the compared models (the routes compare the same ones)."""
    seen = set()
    for key, g in GROUPS:
        seen |= {g["patterns"][b] for b in ds.compared(key, g)}
    assert seen == set(hard_models.PATTERNS)
    assert sum(len(ds.compared(key, g)) for key, g in GROUPS) >= 250
    assert {key[:2] for key, _ in GENERIC_GROUPS} == set(ds.GENERIC_SHAPES)


# ------------------------------------------------------------------------------------------------------- disturbances
@pytest.mark.parametrize("key,g", GROUPS, ids=IDS)
def test_disturbances(key, g, jit_cache):
    N, K, T, B = key
    kf = _engine(key, g)
    if not kf.disturbances_supported():
        pytest.skip("no disturbance walk for (%d,%d)" % (N, K))
    worst = _Worst("disturbances", key)
    has_tape = int(kf._L.mk_adjoint_update_stride(N, K)) > 0
    runs = {}
    for upd in ((True, False) if has_tape else (False,)):
        kf.adjoint_updates = upd
        kf._ensure_grad_updates(B)                 # the context holds (or drops) the gradient's update tape
        assert not upd or kf._grad_upd is not None
        out = kf.disturbances(g["phi"], g["q"], x0=g["x0"], P0=g["P0"])
        _no_flags(out["status"], "disturbances")
        runs[upd] = (_np(out["r"]).copy(), _np(out["ninfo"]).copy())
    for upd, (gr, gn) in runs.items():
        assert gr.shape == gn.shape == (B, T, N + K)
        for b in ds.compared(key, g):
            ref = ds.oracle_ref(g, b)
            rl, nl = ds.dist(g, b)
            tol_r, tol_n = hard_models.disturbance_tolerances(g, b, ref, rl, nl)
            what = _what(g, b, "update tape" if upd else "no tape")
            worst.check(np.abs(gr[b] - rl).max(), tol_r, what + " r")
            worst.check(np.abs(gn[b] - nl).max(), tol_n, what + " ninfo")
            assert (gn[b] >= 0).all(), what
            if T > 1:
                mean, var = disturbance_ref.moments(g["q"][b], gr[b], gn[b])
                dm, dv = ds.dist_definition(g, b)
                tol = hard_models.smoother_tolerance(g, b, ref)
                worst.check(np.abs(mean - dm)[1:].max(), tol, what + " q r against the definition")
                worst.check(np.abs(var - dv)[1:].max(), tol, what + " q - q^2 N against the definition")
    worst.report()
    kf.close()


# ---------------------------------------------------------------------------------------------------------- forecasts
def _near_threshold(y, f, atol, rtol):
    """[N,H]: the pairs whose e^2 / s is within twice the bar's reach of the coverage threshold (where a hit may flip)."""
    ratio = f["ratio"].astype(np.float64)
    T, H, N = ratio.shape
    e = np.full((T, H, N), np.nan)
    for h in range(1, H + 1):
        for o in range(ds.T_FIRST, T - h):
            e[o, h - 1] = y[o + h] - f["M"][o + 1, h - 1].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        reach = 2.0 * ratio * ((2.0 * atol * np.abs(e) + atol * atol) / (e * e) + rtol)
        near = np.isfinite(ratio) & (np.abs(ratio - ds.Z95 ** 2) <= reach)
    return near.sum(0).T


def _check_forecast(key, g, kf, worst):
    N, K, T, B = key
    H, th = ds.HORIZON, ds.track_horizon(key)
    origins = [ds.origin(key, b) for b in range(B)]
    assert len(set(origins)) == min(B, T + 1)
    r = kf.forecast(g["phi"], g["q"], g["x0"], g["P0"], horizon=H, outputs=("fan", "track", "skill"), origins=origins,
                    track_horizon=th, t_first=ds.T_FIRST, coverage=ds.COVERAGE)
    _no_flags(r["status"], "forecast")
    got = {k: _np(r[k]) for k in FAN + TRACK + ("skill",)}
    assert got["fan_mean"].shape == (B, H, N) and got["track_var"].shape == (B, T, N) and got["skill"].shape == (B, N, H, 6)
    for b in ds.compared(key, g):
        f = ds.forecast(key, g, b)
        atol, rtol = hard_models.forecast_tolerances(g, b, ds.oracle_ref(g, b), f["M"])
        what = _what(g, b, "origin", origins[b])
        for k in FAN + TRACK:
            w = f[k].astype(np.float64)
            if k.endswith("mean"):
                worst.check(np.abs(got[k][b] - w).max(), atol, what + " " + k)
            else:
                worst.check(np.abs(got[k][b] / w - 1.0).max(), rtol, what + " " + k)
        y = g["obs"][b]
        sk, w = got["skill"][b], f["skill"].astype(np.float64)
        assert np.isfinite(sk).all(), what
        assert np.array_equal(sk[:, :, 0], w[:, :, 0]), what
        assert (np.abs(sk[:, :, 5] - w[:, :, 5]) <= _near_threshold(y, f, atol, rtol)).all(), what
        bars = forecast_ref.sum_bars(y, f["M"], f["S"], H, ds.T_FIRST, atol, rtol)
        for c in (1, 2, 3, 4):
            diff, bar = np.abs(sk[:, :, c] - w[:, :, c]), bars[:, :, c]
            i = np.unravel_index(np.argmax(np.where(bar > 0, diff / np.where(bar > 0, bar, 1.0), np.where(diff > 0, np.inf, 0.0))), bar.shape)
            worst.check(diff[i], bar[i], what + " skill sum %d of series %d at horizon %d" % (c, i[0], i[1] + 1))
        assert (sk[w[:, :, 0] == 0] == 0).all(), what   # too short or too sparse for any pair: six exact zeros, not NaN


@pytest.mark.parametrize("key,g", GROUPS, ids=IDS)
def test_forecast(key, g, jit_cache):
    kf = _engine(key, g)
    assert kf.forecast_supported
    worst = _Worst("forecast", key)
    _check_forecast(key, g, kf, worst)
    worst.report()
    kf.close()


# ------------------------------------------------------------------------------------------------ observation weights
def _check_weights(key, g, kf, worst):
    N, K, T, B = key
    for what in ("series", "states"):
        tg = ds.group_targets(g, what)
        assert tg.shape == (B, ds.M_SERIES if what == "series" else ds.M_STATES, 2)
        assert len({tuple(map(tuple, tg[b])) for b in range(B)}) > 1   # the lists differ between the records
        res = kf.observation_weights(g["phi"], g["q"], tg, what, x0=g["x0"], P0=g["P0"])
        _no_flags(res["status"], "observation_weights")
        w, ic = _np(res["weights"]), _np(res["intercept"])
        assert w.shape == (B, tg.shape[1], T, N)
        for b in ds.compared(key, g):
            ref = ds.oracle_ref(g, b)
            wl, il = ds.weights(g, b, what)
            y = g["obs"][b]
            seen = np.isfinite(y)
            smoothed = ds.smoothed_at(g, b, what, tg[b])
            rows = float((1.0 + np.abs(g["loadings"][b]).sum(1)).max()) if what == "series" else 1.0
            stol = rows * hard_models.smoother_tolerance(g, b, ref)
            for m in range(tg.shape[1]):
                what_m = _what(g, b, what, "target", tuple(int(v) for v in tg[b, m]))
                if np.isnan(il[m]):                                   # an unused slot: the rule found no such cell
                    assert tg[b, m, 0] < 0 and np.isnan(w[b, m]).all() and np.isnan(ic[b, m]), what_m
                    continue
                assert np.array_equal(np.isnan(w[b, m]), ~seen), what_m   # NaN exactly at the cells that are not observed
                tol = hard_models.weights_tolerance(g, b, ref, wl[m], what)
                if seen.any():
                    worst.check(np.nanmax(np.abs(w[b, m] - wl[m].astype(np.float64))), tol, what_m + " weights")
                worst.check(abs(ic[b, m] - float(il[m])), tol, what_m + " intercept")
                # the reconstruction identity: sum w y + intercept is the oracle's smoothed projection at the target, at the
                # smoother's bar plus the weights' own bar carried through the sum
                terms = (w[b, m][seen] * y[seen]).tolist()
                total = math.fsum(terms + [ic[b, m]])
                worst.check(abs(total - smoothed[m]), stol + tol * (1.0 + float(np.abs(y[seen]).sum())), what_m + " identity")


@pytest.mark.parametrize("key,g", GROUPS, ids=IDS)
def test_observation_weights(key, g, jit_cache):
    kf = _engine(key, g)
    assert kf.observation_weights_supported
    worst = _Worst("observation_weights", key)
    _check_weights(key, g, kf, worst)
    worst.report()
    kf.close()


# -------------------------------------------------------------------------------------------------------------- draws
def _check_draws(key, g, kf, worst):
    N, K, T, B = key
    for what in ("series", "states"):
        out = kf.draw_smoothed(g["phi"], g["q"], 2, seed=time_axis.DRAW_SEED, what=what, x0=g["x0"], P0=g["P0"], antithetic=True)
        _no_flags(out["status"], "draw_smoothed")
        got = _np(out["draws"])
        assert got.shape == (2, B, T, N if what == "series" else N + K)
        for b in ds.compared(key, g):
            d = ds.draws(g, b, what)
            exact = np.isfinite(g["obs"][b]) & ((np.zeros(N) if g["obsvar"] is None else g["obsvar"][b]) == 0.0)[None, :]
            for s in range(2):
                what_s = _what(g, b, what, "draw", s)
                worst.check(np.abs(got[s, b] - d["draws"][s]).max(), d["tol"][s], what_s)
                if what == "series" and exact.any():   # an observed cell without observation variance: the observation
                    worst.check(np.abs(got[s, b] - g["obs"][b])[exact].max(), d["tol"][s], what_s + " at the observed cells")


@pytest.mark.parametrize("key,g", GROUPS, ids=IDS)
def test_draw_smoothed(key, g, jit_cache):
    kf = _engine(key, g)
    worst = _Worst("draw_smoothed", key)
    _check_draws(key, g, kf, worst)
    worst.report()
    kf.close()


# -------------------------------------------------------------------------------------------------------- innovations
def _check_innovations(key, g, kf, worst):
    r = kf.innovations(g["phi"], g["q"], g["x0"], g["P0"])
    _no_flags(r["status"], "innovations")
    got = {k: _np(r[k]) for k in INNOVATION_OUTPUTS}
    for b in ds.compared(key, g):
        _, tol = hard_models.filter_tolerances(g, b, ds.oracle_ref(g, b))
        want = ds.innovations(g, b)
        seen = np.isfinite(g["obs"][b])
        for k in INNOVATION_OUTPUTS:
            gk, wk = got[k][b], want[k].astype(np.float64)
            if k in ("v", "f"):
                assert np.array_equal(np.isnan(gk), ~seen), _what(g, b, k)
                gk, wk = gk[seen], wk[seen]
            if gk.size:
                worst.check(np.abs(gk - wk).max(), tol, _what(g, b, k))


@pytest.mark.parametrize("key,g", GROUPS, ids=IDS)
def test_innovations(key, g, jit_cache):
    kf = _engine(key, g)
    assert kf.innovations_supported
    worst = _Worst("innovations", key)
    _check_innovations(key, g, kf, worst)
    worst.report()
    kf.close()


# ---------------------------------------------------------------------------------------------- the size-generic family
@pytest.mark.parametrize("route", ["innovations", "forecast", "observation_weights", "draw_smoothed"])
@pytest.mark.parametrize("key,g", GENERIC_GROUPS, ids=GENERIC_IDS)
def test_generic_family(key, g, route, jit_cache):
    """The three record readers and the draws behind ``set_variant("kernel_family", "generic")`` (the size-generic recording
    pass and smoother feed them): the same checks at the same bars."""
    kf = _engine(key, g, "generic")
    assert not kf.disturbances_supported()
    worst = _Worst(route + " (generic family)", key)
    {"innovations": _check_innovations, "forecast": _check_forecast, "observation_weights": _check_weights,
     "draw_smoothed": _check_draws}[route](key, g, kf, worst)
    worst.report()
    kf.close()

"""CPU tier of the FITTING routes' property sweep (tests/test_gpu_property_fits.py: intervention effects, window functionals,
per-step scores under the hard models of tests/hard_models.py): on the models the GPU tier compares,
  1. the float64 restatement of every route is inside the route's bar WITHOUT its safety factor against the longdouble
     restatement -- the bars are above what a correct float64 code does;
  2. second definitions hold on hard models: the functional walk against the dense conditioning of the stacked states, ``grad``
     against the adjoint gradient contracted with (dphi, dq), the regression's ``gain`` against the drop of the oracle's -2 log L on
     the adjusted record;
  3. every deliberately wrong variant of a restatement is outside the bars in EVERY group in which it can differ from the right
     answer -- the test works that out from the inputs -- and each can differ in at least half of the groups;
  4. conditions on the INPUTS that the GPU tier relies on: the float64 and the longdouble restatement drop the same effects and no
     pivot sits within a factor 100 of the threshold (at most 2 % of the models may break this; they leave the beta / cov comparison
     only), and a float64 evaluation of the functional walk's unpivoted L D L' meets no pivot <= 0."""
import numpy as np
import pytest

import adjoint_ref
import diagnostic_sweep as ds
import functional_ref
import hard_models
import oracle
import regress_ref

GROUPS, IDS = ds.GROUPS, ds.IDS
F64 = np.float64
EXCLUDED_CAP = 0.02


def test_flat_bars_are_the_tiers_own():
    import call_forms
    import test_regression_gpu
    import test_scores_gpu

    assert (hard_models.REGRESS_BAR_A, hard_models.REGRESS_BAR_S) == (test_regression_gpu.BAR_A, test_regression_gpu.BAR_S)
    assert (hard_models.SCORE_BAR, hard_models.SCORE_BAR_SHORT) == (test_scores_gpu.BAR, test_scores_gpu.BAR_SHORT)
    assert hard_models.SCORE_SHORT == test_scores_gpu.SHORT and regress_ref.MIN_PIVOT == 1e-12
    assert hard_models.FUNCTIONAL_ATOL == call_forms.SMOOTH_ATOL == hard_models.DRAW_TOL
    g = GROUPS[0][1]
    ref = ds.oracle_ref(g, 0)   # the flat part of smoother_tolerance is FUNCTIONAL_ATOL on the scale of the moments
    big = max(1.0, float(np.abs(ref["Pp"]).max()), float(np.abs(ref["F"]).max()))
    assert hard_models.smoother_tolerance(g, 0, ref) >= hard_models.FUNCTIONAL_ATOL * big > 0
    assert ds.FUNCTIONAL_VARIANTS == functional_ref.WRONG and len(ds.REGRESS_VARIANTS) == len(ds.SCORE_VARIANTS) == 5


def test_score_subset_covers_every_pattern_and_shape():
    """The capped subset of the score route: the union over the groups holds every missingness pattern and every shape; every
    persistent model is in it (up to the cap), and up to N + K = 16 it is ``compared``."""
    seen, shapes = set(), set()
    for key, g in GROUPS:
        sc = ds.score_compared(key, g)
        seen |= {g["patterns"][b] for b in sc}
        shapes.add(key[:2])
        assert sc and len(set(sc)) == len(sc)
        if key[0] + key[1] <= ds.SCORE_ALL_UP_TO:
            assert sc == ds.compared(key, g)
        else:
            near = [b for b in range(key[3]) if g["phi"][b].max() > 1.0 - 1e-6]
            assert len(sc) <= ds.SCORE_CAP and set(near[:ds.SCORE_CAP]) <= set(sc)
    assert seen == set(hard_models.PATTERNS)
    assert shapes == set(hard_models.AOT_SHAPES + hard_models.JIT_SHAPES)


def _regression_bars(g, b, margin=hard_models.MARGIN):
    return hard_models.regression_tolerances(g, b, ds.oracle_ref(g, b), ds.regression(g, b), margin=margin)


def _functional_bars(key, g, b):
    return hard_models.functional_tolerances(g, b, ds.oracle_ref(g, b), ds.functional_reach(key, g, b))


def _score_bars(key, g, b, margin=hard_models.MARGIN):
    return hard_models.score_tolerances(g, b, ds.oracle_ref(g, b), key[2], margin=margin)


def _inside(checks, what):
    for name, err, bar in checks:
        assert err <= bar, what + (name, err, bar)


@pytest.mark.parametrize("key,g", GROUPS, ids=IDS)
def test_float64_restatements_are_inside_the_bars_without_the_margin(key, g):
    scored = set(ds.score_compared(key, g))
    for b in sorted(set(ds.compared(key, g)) | scored):
        what = (key, b, g["patterns"][b])
        r64 = ds.regression(g, b, F64)
        _inside(ds.regression_checks(r64, ds.regression(g, b), _regression_bars(g, b, 1.0), ds.regression_usable(g, b)), what)
        _inside(ds.functional_checks(ds.functional_walk(key, g, b, F64), ds.functional_walk(key, g, b), _functional_bars(key, g, b)), what)
        if b in scored:
            _inside(ds.score_checks(ds.scores(g, b, F64), ds.scores(g, b), _score_bars(key, g, b, 1.0)), what)


def test_regression_inputs_are_decided_by_the_model_not_by_rounding():
    """The condition of ``ds.regression_usable`` over every compared model; a model that breaks it is named here."""
    broken, total = [], 0
    for key, g in GROUPS:
        for b in ds.compared(key, g):
            total += 1
            if not ds.regression_usable(g, b):
                broken.append((key, b, g["patterns"][b]))
    assert len(broken) <= EXCLUDED_CAP * total, broken
    print("regression: %d of %d compared models excluded from the beta / cov comparison: %s" % (len(broken), total, broken))


@pytest.mark.parametrize("key,g", GROUPS, ids=IDS)
def test_the_walks_factorisation_meets_no_nonpositive_pivot(key, g):
    """A float64 restatement of functional_walk_kernel's unpivoted L D L' of Pp_{t+1} = Phi Pf_t Phi + Q: every pivot is positive on
    every compared model (q > 0 bounds them from below), so the GPU tier may demand a status without MK_FLAG_RANK_DEFICIENT."""
    for b in ds.compared(key, g):
        assert ds.ldl_pivots(g, b) > 0, (key, b, g["patterns"][b], ds.ldl_pivots(g, b))


def _warmup_of(obs, t_first):
    """The filter's warm-up that names the steps t >= t_first of a record: the non-empty steps before t_first."""
    return int(np.isfinite(obs[:t_first]).any(axis=1).sum())


def _objective(g, b, y, warmup):
    """(-2 log L of record ``y`` under model b's parameters at ``warmup``, the oracle's dict) by the C oracle."""
    other = dict(g, obs=g["obs"].copy())
    other.pop("_cache", None)
    other["obs"][b] = y
    ref = hard_models.oracle_model(oracle, other, b, smooth=False)
    sc = ref["sigmacount"]
    return oracle.get_mle(ref["sigmas"][:sc], ref["detfs"][:sc], oracle.set_observations(y)[2], warmup), ref


@pytest.mark.parametrize("key,g", GROUPS, ids=IDS)
def test_second_definitions(key, g):
    N, K, T, B = key
    scored = set(ds.score_compared(key, g))
    for b in sorted(set(ds.compared(key, g)) | scored):
        what = (key, b, g["patterns"][b])
        y, tf = g["obs"][b], ds.t_first(b)
        w = _warmup_of(y, tf)
        # functionals: the longdouble walk from the oracle's records against the dense conditioning of all T states
        if ds.has_definition(key):
            _inside(ds.functional_checks(ds.functional_walk(key, g, b), ds.functional_definition(key, g, b), _functional_bars(key, g, b)), what)
        # scores: grad is the adjoint gradient (float64, another algorithm) contracted with (dphi, dq); its bar on the larger of
        # grad's scale and the contraction's own |gphi dphi| + |gq dq|
        if b in scored:
            sl = ds.scores(g, b)
            dphi, dq = ds.derivs(g, b)
            yy, phi, q, G, R, x0, P0 = ds.args(g, b)
            _, gphi, gq = adjoint_ref.gradient(yy, phi, q, G, w, x0, P0, R)
            scale = np.maximum(sl["scale"]["grad"].astype(F64), np.abs(gphi * dphi) + np.abs(gq * dq))
            err = np.abs(gphi * dphi + gq * dq - sl["grad"].astype(F64))
            assert (err <= _score_bars(key, g, b)["grad"] * scale).all(), what + (float((err / np.where(scale > 0, scale, 1)).max()),)
            assert sl["count"] == int(np.isfinite(y[tf:]).any(axis=1).sum()), what
        # regression: the gain is the drop of the filter's objective on the record adjusted by the kept effects' beta
        rl = ds.regression(g, b)
        if (~rl["dropped"]).any():
            base, ref = _objective(g, b, y, w)
            after, ref_adj = _objective(g, b, regress_ref.adjusted(y, ds.effects(g, b), rl["beta"].astype(F64)), w)
            bar = (_regression_bars(g, b)["gain"] + hard_models.mle_tolerance(g, b, ref, base) + hard_models.mle_tolerance(g, b, ref_adj, after))
            assert abs((base - after) - float(rl["gain"])) <= bar, what + (base - after, float(rl["gain"]), bar)
        else:
            assert rl["gain"] == 0, what


# ------------------------------------------------------------------------------------------------------- wrong variants
def _observed_from(y, t):
    """True when a step >= t holds an observation."""
    return bool(np.isfinite(y[max(t, 0):]).any())


def _regression_applies(key, g, b, variant):
    """Can the variant change a counted sum of model b?  A regressor matters at OBSERVED cells only, and a change before t_first
    reaches the sums through the replayed state, which takes an observed step at or after it."""
    y, tf, ef = g["obs"][b], ds.t_first(b), ds.effects(g, b)
    T, N = y.shape
    seen = np.isfinite(y)
    if variant == "descending":
        return any(seen[t].sum() >= 2 and _observed_from(y, max(t, tf)) for t in range(T))
    if variant == "late_sums":
        return tf < T and bool(seen[tf].any())
    if variant == "skip_before":
        return tf >= 1 and (bool(seen[:tf].any()) or g["x0"] is not None) and _observed_from(y, tf)
    for j, kind, t0, t1 in ef:
        if j < 0:
            continue
        if variant == "inclusive" and kind == regress_ref.LEVEL and t1 < T and seen[t1, j] and _observed_from(y, max(t1, tf)):
            return True
        if variant == "ramp_from_zero" and kind == regress_ref.RAMP and any(seen[t, j] and _observed_from(y, max(t, tf)) for t in range(t0, T)):
            return True
    return False


def _regression_caught(key, g, b, variant):
    rw = ds.regression(g, b, variant=variant)
    return any(err > bar for _, err, bar in ds.regression_checks(rw, ds.regression(g, b), _regression_bars(g, b), ds.regression_usable(g, b)))


def _functional_applies(key, g, b, variant):
    """From the windows of record b: the lag terms need a hull of two steps (the whole record, T >= 2), so do the moved edges (a
    one-step record has nowhere to move them to) and the second range; the carry through a gap needs a difference window with a
    step between its ranges; the record has no scaling, so applying it once or twice is the same."""
    T = key[2]
    if variant == "scale_once":
        return False
    if variant == "no_gap_carry":
        for win in ds.windows(key, g, b):
            al, _ = functional_ref.alphas(win, T)
            on = np.nonzero(al)[0] if al is not None else []
            if len(on) and (al[on.min():on.max() + 1] == 0).any():
                return True
        return False
    return T >= 2


def _functional_caught(key, g, b, variant):
    got, want = ds.functional_walk(key, g, b, variant=variant), ds.functional_walk(key, g, b)
    return any(err > bar for _, err, bar in ds.functional_checks(got, want, _functional_bars(key, g, b)))


def _score_applies(key, g, b, variant):
    y, tf = g["obs"][b], ds.t_first(b)
    if variant == "count_before":
        return bool(np.isfinite(y[:tf]).any())
    if variant == "uncentred":
        return _observed_from(y, tf)
    return bool(np.isfinite(y).any())


def _score_caught(key, g, b, variant):
    return any(err > bar for _, err, bar in ds.score_checks(ds.scores(g, b, variant=variant), ds.scores(g, b), _score_bars(key, g, b)))


WRONG = [("regression", v, _regression_applies, _regression_caught, ds.compared) for v in ds.REGRESS_VARIANTS] + \
        [("functionals", v, _functional_applies, _functional_caught, ds.compared) for v in ds.FUNCTIONAL_VARIANTS] + \
        [("scores", v, _score_applies, _score_caught, ds.score_compared) for v in ds.SCORE_VARIANTS]
NEVER_APPLICABLE = {("functionals", "scale_once")}   # the hard generator draws no scaling: with scale = 1 the variant IS the right answer


@pytest.mark.parametrize("route,variant,applies,caught,models", WRONG, ids=["%s-%s" % w[:2] for w in WRONG])
def test_wrong_variants_are_outside_the_bars_in_every_applicable_group(route, variant, applies, caught, models):
    """Per group: where the variant can differ on some compared model, some compared model tells (tried in the order of
    ``applies``, the first that tells ends the group).  A variant that cannot differ must not be 'caught' either."""
    applicable = 0
    for key, g in GROUPS:
        can = [b for b in models(key, g) if applies(key, g, b, variant)]
        applicable += bool(can)
        if can:
            assert any(caught(key, g, b, variant) for b in can), (route, variant, key, can)
    if (route, variant) in NEVER_APPLICABLE:
        assert applicable == 0
        key, g = GROUPS[1]
        assert not any(caught(key, g, b, variant) for b in models(key, g)[:3])
    else:
        assert 2 * applicable >= len(GROUPS), (route, variant, applicable)

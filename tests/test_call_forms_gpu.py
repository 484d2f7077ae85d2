"""GPU tier, the call-form axis: every kernel that computes ``rec = inst % R`` for itself, run with more instances than
records (B = 15 parameter sets on R = 3 records; tests/call_forms.py) and at warm-ups other than 1, every instance against
the plain references of ``call_forms.reference``.

Shapes (all prebuilt), one per kernel that owns a ``rec``:
  (8,2)    narrow filter, both narrow smoothers, adjoint and leave-one-out walk; four models per wavefront
  (12,4)   n = 16, HOIST false
  (13,4)   split layout with H = 16, four models per wavefront; tape
  (32,4)   split layout with H = 32, two models per wavefront; adjoint_wide_kernel with and without the update tape;
           smoother_dk_kernel; both mk_wide.hip smoothers
  (33,4)   lane-per-state tape writer
  (60,4)   a full wavefront; no tape, no leave-one-out
  (8,2), (32,4), (70,3) with the size-generic family: 64, 256 and 1024 threads ((70,3): B = 6, T = 5)

Every wide variant is set explicitly, so that the 15-instance call and the 3-instance calls of the position-independence
check run the same kernels.  Bars: the tier's existing ones, listed in tests/call_forms.py; tests/test_call_forms.py shows on
the CPU that every wrong pairing of instance and record is at least 1000 of them away.  tests/test_draws_gpu.py runs
draw_smoothed with B == R only, so the draws are checked here too."""
import numpy as np
import pytest

import call_forms as cf

pytestmark = pytest.mark.gpu

SPECIALISED = [s for s in cf.SHAPES if s[0] + s[1] <= 64]
LAYOUTS = ("model_major", "time_major")
shapes = pytest.mark.parametrize("shape", SPECIALISED, ids=["%dx%d" % s for s in SPECIALISED])
layouts = pytest.mark.parametrize("layout", LAYOUTS)


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module", autouse=True)
def jit_cache(tmp_path_factory):
    import os

    old = os.environ.get("METRAN_HIP_CACHE")
    if old is None:
        os.environ["METRAN_HIP_CACHE"] = str(tmp_path_factory.getbasetemp() / "mkjit")
    yield
    if old is None:
        os.environ.pop("METRAN_HIP_CACHE", None)


def _engine(g, layout, family="specialised", **variants):
    """An engine on the group's records with every variant chosen here, none left to a rule on the batch size."""
    from metran_amd.engine import BatchedKalman

    kf = BatchedKalman(0, layout=layout)
    kf.set_observations(g["obs"]).set_loadings(g["loadings"], g["obsvar"])
    if g["scale"] is not None:
        kf.set_scaling(g["scale"], g["offset"])
    chosen = dict(kernel_family=family, smoother16="record", wide_smoother="mfma", tape_filter="observable",
                  wide_filter="split" if g["N"] <= 32 else "lane_per_state")
    chosen.update(variants)
    for which, name in chosen.items():
        kf.set_variant(which, name)
    kf.projection_path = "auto"
    assert kf.specialised() == (g["N"] + g["K"] <= 64)
    assert kf.get_variant("wide_filter") != "auto" and kf.resolved_wide_filter(g["B"]) == kf.resolved_wide_filter(g["R"])
    return kf


def _filter_variants(N, K):
    """The filter / smoother kernels that serve a shape, as set_variant keywords."""
    n = N + K
    if n <= 16:
        return [dict(smoother16="record")] + ([dict(smoother16="blk")] if n <= 15 else [])
    out = [dict(wide_smoother="mfma")]
    if N <= 32:
        out.append(dict(wide_filter="lane_per_state"))
    if n <= 51:
        out.append(dict(wide_smoother="v1"))
    return out


def _check_state(r, g, what, keys=("F", "Pf", "Xp", "Pp", "S", "Ps")):
    from metran_amd.engine import FLAG_NONPOSITIVE_F, FLAG_NOT_SPD

    assert not (int(np.bitwise_or.reduce(_np(r["status"]))) & (FLAG_NONPOSITIVE_F | FLAG_NOT_SPD)), what
    got = {k: _np(r[k]) for k in keys + ("mle", "sigmacount", "sigmas", "detfs")}
    for i in range(g["B"]):
        ref = cf.reference(g, i, 1, parts=("state",))
        w, rec, sc = "%s: %s" % (what, cf._what(g, i)), ref["rec"], ref["sigmacount"]
        cf.assert_close("mle", got["mle"][i], ref["mle"], g, rec, w)
        assert int(got["sigmacount"][i]) == sc, w
        cf.assert_close("sigmas", got["sigmas"][i, :sc], ref["sigmas"][:sc], g, rec, w)
        cf.assert_close("detfs", got["detfs"][i, :sc], ref["detfs"][:sc], g, rec, w)
        if "_rs" in r:   # packed records: the pads of the steps behind the last observed one are zero
            assert not got["sigmas"][i, sc:].any() and not got["detfs"][i, sc:].any(), w
        for k in keys:
            cf.assert_close(k, got[k][i], ref[k], g, rec, w)


@layouts
@shapes
def test_objective(shape, layout):
    """loglik at warm-up 0, 1, 2, 3 and T + 1, from given initial moments and from the defaults."""
    for g in (cf.group(*shape), cf.group_defaults(*shape)):
        kf = _engine(g, layout)
        cf.check_objective(kf, g, cf.loglik_warmups(g["T"]))
        kf.close()


@layouts
@shapes
def test_filter_and_smoother_records(shape, layout):
    """filter_smooth with full records behind every filter / smoother kernel of the shape, and with a dense subset."""
    g = cf.group(*shape)
    for variants in _filter_variants(*shape):
        kf = _engine(g, layout, **variants)
        _check_state(kf.filter_smooth(g["phi"], g["q"], **cf.init(g)), g, "%s %s" % (layout, variants))
        kf.close()
    kf = _engine(g, layout)
    r = kf.filter_smooth(g["phi"], g["q"], outputs=("F", "Pf", "S"), **cf.init(g))
    assert "_rs" not in r and "Ps" not in r
    _check_state(r, g, layout + " dense subset", keys=("F", "Pf", "S"))
    kf.close()
    d = cf.group_defaults(*shape)
    kf = _engine(d, layout)
    _check_state(kf.filter_smooth(d["phi"], d["q"]), d, layout + " default moments")
    kf.close()


@layouts
@shapes
def test_projection_and_state_variances(shape, layout):
    """simulate_smoothed on the tape (both tape writers where N <= 32) and on the filtered records, and
    smooth_state_variances (on the state tape too: the same group without observation variances), with a scale and an
    offset per record."""
    N, K = shape
    g = cf.group(N, K)
    served = 16 < N + K <= 63
    writers = ("observable", "state") if served and N <= 32 else ("observable",)
    for gg in (g, cf.group_without_obsvar(N, K)) if served else (g,):
        for writer in writers:
            kf = _engine(gg, layout, tape_filter=writer)
            assert kf.tape_path() == served
            for route in ("auto", "records") if served else ("auto",):
                kf.projection_path = route
                on_tape = served and route == "auto"
                out = []
                if gg is g:
                    out.append(kf.simulate_smoothed(gg["phi"], gg["q"], **cf.init(gg)))
                    assert bool(out[-1].get("_tape")) == on_tape
                if gg is g or on_tape:
                    out.append(kf.smooth_state_variances(gg["phi"], gg["q"], **cf.init(gg)))
                    assert bool(out[-1].get("_tape")) == (on_tape and gg["obsvar"] is None)
                got = [{k: _np(v) for k, v in o.items() if k in ("mle", "sim_means", "sim_vars", "S", "var")} for o in out]
                for i in range(gg["B"]):
                    ref = cf.reference(gg, i, 1, parts=("state",))
                    what = "%s, route %s, writer %s, R %s: %s" % (layout, route, writer, gg["obsvar"] is not None, cf._what(gg, i))
                    for o in got:
                        cf.assert_close("mle", o["mle"][i], ref["mle"], gg, ref["rec"], what)
                        for k, q in (("sim_means", "sim_means"), ("sim_vars", "sim_vars"), ("S", "S"), ("var", "state_vars")):
                            if k in o:
                                cf.assert_close(q, o[k][i], ref[q], gg, ref["rec"], what)
            kf.close()


@layouts
@shapes
def test_leave_one_out(shape, layout):
    g = cf.group(*shape)
    kf = _engine(g, layout)
    assert kf.loo_supported() == cf.has_loo(*shape)
    if not kf.loo_supported():
        kf.close()
        return
    r = kf.loo_predict(g["phi"], g["q"], **cf.init(g))
    assert int(r["status"].abs().sum().item()) == 0
    gm, gv = _np(r["loo_means"]), _np(r["loo_vars"])
    for i in range(g["B"]):
        ref = cf.reference(g, i, 0, parts=("loo",))
        seen = np.isfinite(g["obs"][ref["rec"]])
        assert np.array_equal(np.isnan(gm[i]), ~seen) and np.array_equal(np.isnan(gv[i]), ~seen), cf._what(g, i)
        cf.assert_close("loo_means", gm[i], ref["loo_means"], g, ref["rec"], cf._what(g, i))
        cf.assert_close("loo_vars", gv[i], ref["loo_vars"], g, ref["rec"], cf._what(g, i))
    kf.close()


def _gradient_engines(g, layout):
    """(adjoint_updates, wide filter) -> engine: for n > 16 the walk over the update tape and the recomputing walk behind the
    lane-per-state filter (the update tape's writer, whatever the variant says: mk_capi.hip), and where N <= 32 the recomputing
    walk behind the split-layout filter."""
    if g["N"] + g["K"] <= 16:
        return {(False, None): _engine(g, layout)}
    out = {}
    for upd, wf in ((True, "lane_per_state"), (False, "lane_per_state"), (False, "split")):
        if wf == "split" and g["N"] > 32:
            continue
        out[upd, wf] = _engine(g, layout, wide_filter=wf)
        out[upd, wf].adjoint_updates = upd
    return out


@layouts
@shapes
def test_gradient(shape, layout):
    """loglik_grad at warm-up 0, 2 and 3 (the "single" record's instances: exactly zero from warm-up 1 on); the objective
    bit for bit the same with and without the update tape; the two-phase form at warm-up 2 -- a forward pass at a decoy
    point, one at the point, one backward walk -- bit for bit the single call."""
    g = cf.group(*shape)
    engines = _gradient_engines(g, layout)
    res = {}
    for key, kf in engines.items():
        assert kf.has_adjoint()
        for w in cf.GRAD_WARMUPS:
            res[key, w] = tuple(_np(t) for t in kf.loglik_grad(g["phi"], g["q"], warmup=w, **cf.init(g)))
            cf.check_gradient(res[key, w], g, w, "%s %s" % (layout, key))
        if key[1] is not None:
            assert (getattr(kf, "_grad_upd", None) is not None) == key[0]
        single = [i for i in range(g["B"]) if g["patterns"][i % g["R"]] == "single"]
        assert len(single) == g["S"] and not res[key, 2][1][single].any() and not res[key, 2][2][single].any()
        cf.check_two_phase(lambda p: kf.loglik_forward(p[0], p[1], warmup=2, **cf.init(g)), kf.loglik_backward,
                           lambda p: kf.loglik_grad(p[0], p[1], warmup=2, **cf.init(g)),
                           (g["phi"], g["q"]), (g["phi"] * 0.9, g["q"] * 1.1), "%s %s two-phase" % (layout, key))
    for (upd, wf), w in res:
        if upd:   # the objective does not know about the tape
            assert np.array_equal(res[(True, wf), w][0], res[(False, wf), w][0]), (wf, w)
    for kf in engines.values():
        kf.close()


@layouts
@shapes
def test_gradient_in_alpha(shape, layout):
    """loglik_grad_alpha(alpha, dt=0.5, warmup=2): mk_params_from_alpha and mk_alpha_grad take (B, R) too."""
    g = cf.group(*shape)
    for kf in _gradient_engines(g, layout).values():
        cf.check_gradient_alpha(kf, g, dt=0.5, warmup=2)
        kf.close()


@layouts
@shapes
def test_results_do_not_depend_on_position(shape, layout):
    """The call on S * R instances equals, bit for bit, the S calls with B = R on the same models: objective, gradient,
    filter and smoother records, projection, state variances, leave-one-out predictions."""
    N, K = shape
    g = cf.group(N, K)
    take = lambda r, keys: {k: r[k] for k in keys}  # noqa: E731
    engines = _gradient_engines(g, layout)
    for key, kf in engines.items():
        cf.check_position_independent(lambda gg: dict(zip(("mle", "gphi", "gq"), kf.loglik_grad(gg["phi"], gg["q"], warmup=2, **cf.init(gg)))),
                                      g, "loglik_grad %s" % (key,))
    kf = next(iter(engines.values()))
    cf.check_position_independent(lambda gg: {"mle": kf.loglik(gg["phi"], gg["q"], warmup=3, **cf.init(gg))}, g, "loglik")
    for kf in engines.values():
        kf.close()
    for variants in _filter_variants(N, K):
        kf = _engine(g, layout, **variants)
        cf.check_position_independent(lambda gg: take(kf.filter_smooth(gg["phi"], gg["q"], **cf.init(gg)),
                                                      ("mle", "sigmacount", "sigmas", "detfs", "F", "Pf", "Xp", "Pp", "S", "Ps")),
                                      g, "filter_smooth %s" % variants)
        kf.close()
    served = 16 < N + K <= 63
    for writer in ("observable", "state") if served and N <= 32 else ("observable",):
        kf = _engine(g, layout, tape_filter=writer)
        for route in ("auto", "records") if served else ("auto",):
            kf.projection_path = route
            cf.check_position_independent(lambda gg: take(kf.simulate_smoothed(gg["phi"], gg["q"], **cf.init(gg)), ("mle", "sim_means", "sim_vars")),
                                          g, "simulate_smoothed %s %s" % (writer, route))
            cf.check_position_independent(lambda gg: take(kf.smooth_state_variances(gg["phi"], gg["q"], **cf.init(gg)), ("mle", "S", "var")),
                                          g, "smooth_state_variances %s %s" % (writer, route))
        kf.projection_path = "auto"
        if kf.loo_supported() and writer == "observable":
            cf.check_position_independent(lambda gg: take(kf.loo_predict(gg["phi"], gg["q"], **cf.init(gg)), ("loo_means", "loo_vars")),
                                          g, "loo_predict")
        kf.close()


@layouts
@pytest.mark.parametrize("shape", cf.SHAPES, ids=["%dx%d" % s for s in cf.SHAPES])
def test_draws(shape, layout):
    """draw_smoothed with B > R (tests/test_draws_gpu.py has B == R throughout): at an observed cell without observation
    variance a series draw is the observation of record i % R, in that record's units; an antithetic pair averages to the
    instance's own smoothed projection.  The draws tier's bar (tests/test_draws_gpu.py: TOL)."""
    g = cf.group(*shape)
    kf = _engine(g, layout)
    out = kf.draw_smoothed(g["phi"], g["q"], 2, seed=11, what="series", antithetic=True, **cf.init(g))
    assert int(out["status"].abs().sum().item()) == 0
    draws = _np(out["draws"])
    assert draws.shape == (2, g["B"], g["T"], g["N"])
    sim = _np(kf.simulate_smoothed(g["phi"], g["q"], **cf.init(g))["sim_means"])
    for i in range(g["B"]):
        r = i % g["R"]
        exact = np.isfinite(g["obs"][r]) & (g["obsvar"][r] == 0.0)[None, :]
        want = g["obs"][r] * g["scale"][r] + g["offset"][r]
        assert exact.any() or g["patterns"][r] == "single"
        for s in range(2):
            assert np.abs(draws[s, i][exact] - want[exact]).max(initial=0.0) <= cf.DRAW_TOL, cf._what(g, i)
        assert np.abs(0.5 * (draws[0, i] + draws[1, i]) - sim[i]).max() <= cf.DRAW_TOL, cf._what(g, i)
        cf.assert_close("sim_means", sim[i], cf.reference(g, i, 1, parts=("state",))["sim_means"], g, r, cf._what(g, i))
        assert np.abs(draws[0, i] - draws[1, i])[~np.isfinite(g["obs"][r])].max() > 1e-3
    kf.close()


@layouts
@pytest.mark.parametrize("shape", cf.GENERIC_SHAPES, ids=["%dx%d" % s for s in cf.GENERIC_SHAPES])
def test_generic_kernel_family(shape, layout):
    """The size-generic kernels (mk_generic.hip) on the same groups: objective, records, projection, state variances, and
    their independence of position."""
    g = cf.group(*shape)
    kf = _engine(g, layout, family="generic")
    assert not kf.has_adjoint() and not kf.tape_path() and not kf.loo_supported()
    cf.check_objective(kf, g, cf.loglik_warmups(g["T"]), "generic")
    _check_state(kf.filter_smooth(g["phi"], g["q"], **cf.init(g)), g, layout + " generic")
    p = kf.simulate_smoothed(g["phi"], g["q"], **cf.init(g))
    s = kf.smooth_state_variances(g["phi"], g["q"], **cf.init(g))
    got = {k: _np(v) for k, v in (("sim_means", p["sim_means"]), ("sim_vars", p["sim_vars"]), ("S", s["S"]), ("state_vars", s["var"]))}
    for i in range(g["B"]):
        ref = cf.reference(g, i, 1, parts=("state",))
        for o in (p, s):
            cf.assert_close("mle", _np(o["mle"])[i], ref["mle"], g, ref["rec"], cf._what(g, i, "generic"))
        for k, v in got.items():
            cf.assert_close(k, v[i], ref[k], g, ref["rec"], cf._what(g, i, "generic"))
    take = lambda r, keys: {k: r[k] for k in keys}  # noqa: E731
    cf.check_position_independent(lambda gg: {"mle": kf.loglik(gg["phi"], gg["q"], warmup=2, **cf.init(gg))}, g, "generic loglik")
    cf.check_position_independent(lambda gg: take(kf.filter_smooth(gg["phi"], gg["q"], **cf.init(gg)),
                                                  ("mle", "sigmacount", "sigmas", "detfs", "F", "Pf", "Xp", "Pp", "S", "Ps")), g, "generic filter_smooth")
    cf.check_position_independent(lambda gg: take(kf.simulate_smoothed(gg["phi"], gg["q"], **cf.init(gg)), ("mle", "sim_means", "sim_vars")),
                                  g, "generic simulate_smoothed")
    kf.close()

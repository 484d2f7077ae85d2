"""GPU tier, the time axis: every kernel that tiles or pipelines along t, at the record lengths where its tile and pipeline
boundaries lie (tests/time_axis.py: T = 1, 2, 3, 15, 16, 17, 32, 33; sparse records with 255 .. 513 observed steps), every
instance against the plain references of ``call_forms.reference``, both layouts, every kernel variant set explicitly.

Shapes (all prebuilt):
  (8,2)    narrow filter and smoothers, adjoint and leave-one-out walk; even N: 16-byte row pieces
  (5,1)    odd N: scalar row pieces; smoother_blk_kernel
  (13,4)   split layout with H = 16, odd N
  (32,4)   split layout with H = 32; both tape writers; smoother_dk_kernel; mfma and v1; adjoint_wide_kernel with and
           without the update tape; once with wide_filter left at the shipped "auto"
  (33,4)   lane-per-state tape writer: the WIDE tile path, odd N
  (60,4)   a full wavefront
  (8,2), (70,3) with the size-generic family at T = 1, 2, 17

One test function per route of time_axis.ROUTES, parametrised over (shape, layout) and looping over the lengths;
tests/test_time_axis.py asserts that coverage, shows on the CPU that a wrong row at a tile edge, a stale tile, a wrong clamp, a
short walk or a dropped list entry is at least 1000 bars away, and runs the check functions used here over a CPU engine.
Bars: the tier's existing ones (tests/call_forms.py; tests/test_sparse_objective.py for the sparse records)."""
import numpy as np
import pytest

import call_forms as cf
import time_axis as ta

pytestmark = pytest.mark.gpu


def _route(route):
    return pytest.mark.parametrize("shape,layout", ta.params(route), ids=ta.param_ids(route))


@pytest.fixture(scope="module", autouse=True)
def jit_cache(tmp_path_factory):
    import os

    old = os.environ.get("METRAN_HIP_CACHE")
    if old is None:
        os.environ["METRAN_HIP_CACHE"] = str(tmp_path_factory.getbasetemp() / "mkjit")
    yield
    if old is None:
        os.environ.pop("METRAN_HIP_CACHE", None)


def _engine(g, layout, family="specialised", packed_sym=False, **variants):
    """An engine on the group's records with every variant chosen here, none left to a rule on the batch size -- except where
    the caller asks for the shipped wide_filter "auto"."""
    from metran_amd.engine import BatchedKalman

    kf = BatchedKalman(0, layout=layout, packed_sym=packed_sym)
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
    assert kf.get_variant("wide_filter") == chosen["wide_filter"]
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
    if (N, K) == (32, 4):
        out.append(dict(wide_filter="auto"))
    return out


def _wide_filters(N, K):
    if N + K <= 16:
        return [{}]
    return [dict(wide_filter=w) for w in (("split", "lane_per_state") if N <= 32 else ("lane_per_state",)) + (("auto",) if (N, K) == (32, 4) else ())]


@_route("filter_smooth")
def test_filter_smooth(shape, layout):
    """All six records, sigmas, detfs and sigmacount behind every filter / smoother kernel of the shape; the packed-symmetric
    records once per shape and length."""
    for T in ta.lengths(shape, "filter_smooth"):
        g = ta.group(shape[0], shape[1], T)
        for variants in _filter_variants(*shape):
            kf = _engine(g, layout, **variants)
            ta.check_state(kf.filter_smooth(g["phi"], g["q"], **cf.init(g)), g, "%s %s" % (layout, variants))
            kf.close()
        if layout == "time_major":
            kf = _engine(g, layout, packed_sym=True)
            ta.check_state(kf.filter_smooth(g["phi"], g["q"], **cf.init(g)), g, layout + " packed_sym", unpack=kf.unpack_sym)
            kf.close()


@_route("loglik")
def test_loglik(shape, layout):
    """The objective at warm-up 0 and 1 behind every wide filter of the shape."""
    for T in ta.lengths(shape, "loglik"):
        g = ta.group(shape[0], shape[1], T)
        for variants in _wide_filters(*shape):
            kf = _engine(g, layout, **variants)
            ta.check_objective(kf, g, "%s %s" % (layout, variants))
            kf.close()


@_route("loglik_grad")
def test_loglik_grad(shape, layout):
    """loglik_grad against the numpy adjoint, the two-phase form bit for bit against it; for n > 16 the walk over the update
    tape and the recomputing walk behind either filter, the objective bit for bit the same with and without the tape."""
    N, K = shape
    for T in ta.lengths(shape, "loglik_grad"):
        g = ta.group(N, K, T)
        res = {}
        walks = [(False, None)] if N + K <= 16 else [(True, "lane_per_state"), (False, "lane_per_state")] + ([(False, "split")] if N <= 32 else [])
        for upd, wf in walks:
            kf = _engine(g, layout, **({} if wf is None else dict(wide_filter=wf)))
            assert kf.has_adjoint()
            kf.adjoint_updates = upd
            res[upd, wf] = [ta._np(t) for t in ta.check_gradient(kf, g, "%s %s" % (layout, (upd, wf)))]
            if wf is not None:
                assert (getattr(kf, "_grad_upd", None) is not None) == upd
            kf.close()
        if (True, "lane_per_state") in res:
            assert np.array_equal(res[True, "lane_per_state"][0], res[False, "lane_per_state"][0]), T


@_route("simulate_smoothed")
def test_simulate_smoothed(shape, layout):
    """simulate_smoothed on "auto" (the tape where it is served, both tape writers where N <= 32) and on "records", and the
    state variances (on the state tape too: the same group without observation variances)."""
    N, K = shape
    served = 16 < N + K <= 63
    writers = ("observable", "state") if served and N <= 32 else ("observable",)
    for T in ta.lengths(shape, "simulate_smoothed"):
        g = ta.group(N, K, T)
        for gg in (g, cf.variant(g, obsvar=None)) if served else (g,):
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
                    ta.check_projection(out, gg, "%s, route %s, writer %s, R %s" % (layout, route, writer, gg["obsvar"] is not None))
                kf.close()


@_route("loo_predict")
def test_loo_predict(shape, layout):
    for T in ta.lengths(shape, "loo_predict"):
        g = ta.group(shape[0], shape[1], T)
        kf = _engine(g, layout)
        assert kf.loo_supported()
        ta.check_loo(kf.loo_predict(g["phi"], g["q"], **cf.init(g)), g, layout)
        kf.close()


def test_no_leave_one_out_for_a_full_wavefront():
    g = ta.group(60, 4, 2)
    kf = _engine(g, "model_major")
    assert not kf.loo_supported()
    kf.close()


@_route("draw_smoothed")
def test_draw_smoothed(shape, layout):
    """Series and state draws, one antithetic pair, draw for draw against tests/draw_ref.py: T + 1 normals per path, step 0
    takes the initial draw (T = 1: nothing else)."""
    for T in ta.lengths(shape, "draw_smoothed"):
        g = ta.group(shape[0], shape[1], T)
        kf = _engine(g, layout)
        for kind in ("series", "states"):
            ta.check_draws(kf, g, kind, layout)
        kf.close()


@_route("generic_family")
def test_generic_family(shape, layout):
    """The size-generic kernels (mk_generic.hip: 64 and 1024 threads) at T = 1, 2 and 17: objective, records, projection and
    state variances."""
    for T in ta.lengths(shape, "generic_family"):
        g = ta.group(shape[0], shape[1], T)
        kf = _engine(g, layout, family="generic")
        assert not kf.has_adjoint() and not kf.tape_path() and not kf.loo_supported()
        ta.check_objective(kf, g, "generic")
        ta.check_state(kf.filter_smooth(g["phi"], g["q"], **cf.init(g)), g, layout + " generic")
        ta.check_projection([kf.simulate_smoothed(g["phi"], g["q"], **cf.init(g)), kf.smooth_state_variances(g["phi"], g["q"], **cf.init(g))],
                            g, layout + " generic")
        kf.close()


# ------------------------------------------------------------------------------------------------------------ the sparse
def _sparse_engine(rec, obsvar):
    from metran_amd.engine import BatchedKalman

    kf = BatchedKalman(0)
    kf.set_observations(rec["obs"][None]).set_loadings(rec["loadings"][None], rec["obsvar"][None] if obsvar else None)
    assert kf.get_variant("single_record") == "sparse" and kf.get_variant("kernel_family") == "specialised"
    return kf


@pytest.mark.parametrize("name", sorted(ta.SPARSE))
def test_sparse_objective(name):
    """loglik of one shared record walks the list of observed steps (observed_steps_kernel: passes of 256 time steps;
    loglik_sparse_kernel: tiles of 256 observed steps): 13 parameter sets against the oracle, and from given x0 / P0 with
    observation variances at warm-up 0, 1 and 3."""
    rec = ta.sparse_record(name)
    kf, full = _sparse_engine(rec, False), _sparse_engine(rec, True)
    ta.check_sparse_objective(kf, rec, full)
    kf.close()
    full.close()


@pytest.mark.parametrize("name", sorted(ta.SPARSE))
def test_sparse_record_filter(name):
    """The record-writing filter of one record (loglik_sparse_kernel<REC> and fill_gaps_kernel) against the oracle and against
    the step-by-step batched kernel: all four state arrays, the records of the empty steps included; sigmacount is the
    constructed count exactly; the pads behind it are zero."""
    rec = ta.sparse_record(name)
    S = ta.SPARSE_RECORD_SETS
    kf = _sparse_engine(rec, True)
    args = (rec["phi"][:S], rec["q"][:S])
    kw = dict(x0=rec["x0"][:S], P0=rec["P0"][:S])
    results = {"sparse": kf.filter(*args, **kw)}
    kf.set_variant("single_record", "stepwise")
    results["stepwise"] = kf.filter(*args, **kw)
    ta.check_sparse_records(results, rec)
    kf.close()

"""GPU tier, the status axis: invalid models in batches where they share a wavefront with valid ones (tests/status_cases.py),
behind every route that writes a status word or returns an objective without one, both layouts, every kernel variant set
explicitly.  Per route and case the same call runs on the BAD group and on its CLEAN TWIN:

  flags         the status of every instance is the expected bit set, bit for bit (from the longdouble restatement)
  containment   every output of every untouched instance is bit-identical to the twin's
  clean         ... and within the tier's existing bar of the oracle
  objective     a reference objective that is not finite is never answered with a finite number

and through the C ABI with d_status prefilled with 0xA5A5A5A5: mk_filter, mk_filter_smooth, mk_smooth, mk_smooth_dense,
mk_loglik_grad and mk_loo WRITE the word.  Every input is finite-or-NaN arithmetic inside kernels that already branch on it.
tests/test_status_cases.py runs the check functions on the CPU first and asserts this file's parametrisation."""
import ctypes

import numpy as np
import pytest

import call_forms as cf
import status_cases as sc
import time_axis as ta

pytestmark = pytest.mark.gpu

PREFILL = 0xA5A5A5A5
ROUTE_TESTS = {
    "test_filter": sc.SHAPES, "test_filter_smooth": sc.SHAPES, "test_projection": sc.SHAPES, "test_loglik": sc.SHAPES,
    "test_sparse_single_record": ((8, 2),), "test_loglik_grad": sc.SHAPES, "test_draw_smoothed": sc.SHAPES,
    "test_loo_predict": tuple(s for s in sc.SHAPES if cf.has_loo(*s)),   # not (60,4): a full wavefront has no leave-one-out walk
    "test_simulate_unconditional": sc.SHAPES,
    "test_generic_family": sc.GENERIC_SHAPES, "test_smoother_entry_points": sc.SHAPES, "test_prefilled_status": sc.SHAPES,
}


def _route(fn):
    shapes = ROUTE_TESTS[fn]
    params = [(s, lay) for s in shapes for lay in sc.LAYOUTS]
    return pytest.mark.parametrize("shape,layout", params, ids=["%dx%d-%s" % (s[0], s[1], lay) for s, lay in params])


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
    from metran_amd.engine import BatchedKalman

    kf = BatchedKalman(0, layout=layout, packed_sym=packed_sym)
    kf.set_observations(g["obs"]).set_loadings(g["loadings"], g["obsvar"])
    if g["scale"] is not None:
        kf.set_scaling(g["scale"], g["offset"])
    chosen = dict(kernel_family=family, smoother16="record", wide_smoother="mfma", tape_filter="observable", single_record="sparse",
                  wide_filter="split" if g["N"] <= 32 else "lane_per_state")
    chosen.update(variants)
    for which, name in chosen.items():
        kf.set_variant(which, name)
    kf.projection_path = "auto"
    assert kf.specialised() == (g["N"] + g["K"] <= 64)
    return kf


def _host(out):
    """A result as numpy arrays (copies: the engine is closed before they are compared); private flags kept."""
    if isinstance(out, (tuple, list)):
        return [sc._np(v).copy() for v in out]
    return {k: (sc._np(v).copy() if hasattr(v, "shape") else v) for k, v in out.items() if not k.startswith("_rec")}


def _pair(c, layout, call, **engine):
    """``call(kf, g)`` on the bad group and on the twin -> the two results on the host."""
    import torch

    outs = []
    for g in (c["bad"], c["twin"]):
        kf = _engine(g, layout, **engine)
        out = call(kf, g)
        torch.cuda.synchronize()
        outs.append(_host(out))
        kf.close()
    return outs


def _check(c, bad, twin, kind, what, warmup=1, clean=True, **kw):
    sc.check_flags(bad["status"], c, kind, what)
    sc.check_twin_flags(twin["status"], c, kind, what)
    sc.check_containment(bad, twin, c, what)
    if clean:
        sc.check_clean(bad, c, what, warmup, **kw)
    if "mle" in bad:
        sc.check_objective(bad["mle"], c, warmup, what)


def _filters(N, K):
    if N + K <= 16:
        return [{}]
    return [dict(wide_filter="lane_per_state")] + ([dict(wide_filter="split")] if N <= 32 else [])


def _smoothers(N, K):
    n = N + K
    if n <= 16:
        return [dict(smoother16="record")] + ([dict(smoother16="blk")] if n <= 15 else [])
    return [dict(wide_smoother="mfma"), dict(wide_smoother="mfma_unfolded")] + ([dict(wide_smoother="v1")] if n <= 51 else [])


def _prefill(status):
    status.fill_(PREFILL - (1 << 32))
    return status


@_route("test_filter")
def test_filter(shape, layout):
    """mk_filter: packed records, dense outputs and packed-symmetric records behind every filter kernel of the shape."""
    for name in sc.CASES:
        c = sc.case(shape[0], shape[1], name)
        for v in _filters(*shape):
            bad, twin = _pair(c, layout, lambda kf, g: kf.filter(g["phi"], g["q"], **cf.init(g)), **v)
            assert "_rs" in bad
            _check(c, bad, twin, "filter", "filter, records %s %s" % (layout, v))
            bad, twin = _pair(c, layout, lambda kf, g: kf.filter(g["phi"], g["q"], outputs=("F", "Pf"), **cf.init(g)), **v)
            assert "_rs" not in bad
            _check(c, bad, twin, "filter", "filter, dense %s %s" % (layout, v))
        def unpacked(kf, g):   # the packed upper triangles as full covariances: the same bits, in the shape the oracle's have
            r = kf.filter(g["phi"], g["q"], **cf.init(g))
            return dict(r, Pf=kf.unpack_sym(r["Pf"]), Pp=kf.unpack_sym(r["Pp"]))

        bad, twin = _pair(c, layout, unpacked, packed_sym=True)
        _check(c, bad, twin, "filter", "filter, packed_sym=True " + layout)


@_route("test_filter_smooth")
def test_filter_smooth(shape, layout):
    """mk_filter_smooth with all six records behind every RTS smoother of the shape: the filter's bit and the smoother's."""
    for name in sc.CASES:
        c = sc.case(shape[0], shape[1], name)
        for v in _smoothers(*shape):
            bad, twin = _pair(c, layout, lambda kf, g: kf.filter_smooth(g["phi"], g["q"], **cf.init(g)), **v)
            _check(c, bad, twin, "rts", "filter_smooth %s %s" % (layout, v))


@_route("test_projection")
def test_projection(shape, layout):
    """simulate_smoothed and smooth_state_variances on the record route and, where the shape has one, on the tape behind both
    tape writers and on the state tape (the group without observation variances; the record cases need them and stay away)."""
    N, K = shape
    served = 16 < N + K <= 63
    writers = ("observable", "state") if served and N <= 32 else ("observable",)
    for name in sc.CASES:
        c = sc.case(N, K, name)
        for writer in writers:
            for route in ("auto", "records") if served else ("auto",):
                def sim(kf, g):
                    kf.projection_path = route
                    return kf.simulate_smoothed(g["phi"], g["q"], **cf.init(g))

                def var(kf, g):
                    kf.projection_path = route
                    return kf.smooth_state_variances(g["phi"], g["q"], **cf.init(g))

                on_tape = served and route == "auto"
                what = "%s, route %s, writer %s" % (layout, route, writer)
                bad, twin = _pair(c, layout, sim, tape_filter=writer)
                assert bool(bad.get("_tape")) == on_tape
                _check(c, bad, twin, "tape" if on_tape else "rts", "simulate_smoothed " + what, keys=("mle", "sim_means", "sim_vars"))
                bad, twin = _pair(c, layout, var, tape_filter=writer)
                assert not bad.get("_tape")
                _check(c, bad, twin, "rts", "smooth_state_variances " + what, keys=("mle", "S", "var"))
                if on_tape and name in sc.INSTANCE_CASES:
                    cs = dict(c, bad=cf.variant(c["bad"], obsvar=None), twin=cf.variant(c["twin"], obsvar=None))
                    bad, twin = _pair(cs, layout, var, tape_filter=writer)
                    assert bad.get("_tape")
                    _check(cs, bad, twin, "tape", "state tape " + what, keys=("mle", "S", "var"))


@_route("test_loglik")
def test_loglik(shape, layout):
    """mk_loglik has no status: the objective alone tells, at warm-up 0 and 1, behind every filter kernel of the shape."""
    for name in sc.CASES:
        c = sc.case(shape[0], shape[1], name)
        for v in _filters(*shape):
            for w in sc.WARMUPS:
                bad, twin = _pair(c, layout, lambda kf, g: {"mle": kf.loglik(g["phi"], g["q"], warmup=w, **cf.init(g))}, **v)
                what = "loglik %s %s" % (layout, v)
                sc.check_containment(bad, twin, c, what)
                sc.check_clean(bad, c, what, w)
                sc.check_objective(bad["mle"], c, w, what)


@_route("test_sparse_single_record")
def test_sparse_single_record(shape, layout):
    """ONE record and B = 9 <= 16 instances: loglik_sparse_kernel, objective-only and record-writing (with fill_gaps_kernel)."""
    for name in sc.INSTANCE_CASES:
        c = sc.single_record(sc.case(shape[0], shape[1], name))
        assert c["bad"]["R"] == 1 and c["bad"]["B"] <= 16
        for w in sc.WARMUPS:
            bad, twin = _pair(c, layout, lambda kf, g: {"mle": kf.loglik(g["phi"], g["q"], warmup=w, **cf.init(g))})
            sc.check_containment(bad, twin, c, "sparse loglik")
            sc.check_clean(bad, c, "sparse loglik", w)
            sc.check_objective(bad["mle"], c, w, "sparse loglik")
        for single in ("sparse", "stepwise"):
            bad, twin = _pair(c, layout, lambda kf, g: kf.filter(g["phi"], g["q"], **cf.init(g)), single_record=single)
            _check(c, bad, twin, "filter", "single-record filter, " + single)


def _grad_raw(kf, g, warmup=0):
    """mk_loglik_grad through the C ABI with a prefilled d_status (the engine passes none)."""
    import torch

    prob, keep, B = kf._problem(g["phi"], g["q"], warmup, g["x0"], g["P0"])
    work = kf._take_grad_work(B * kf.T * kf.record_stride())
    kf._ensure_grad_updates(B)
    out = {"mle": torch.empty(B, dtype=torch.float64, device=kf.device), "gphi": torch.empty((B, kf.n), dtype=torch.float64, device=kf.device),
           "gq": torch.empty((B, kf.n), dtype=torch.float64, device=kf.device), "status": _prefill(torch.empty(B, dtype=torch.int32, device=kf.device))}
    sc_ = torch.empty(B, dtype=torch.int64, device=kf.device)
    kf._bind_stream()
    from metran_amd._lib import check
    check(kf._L.mk_loglik_grad(kf._ctx, ctypes.byref(prob), kf._p(work), 1 if kf.time_major else 0, kf._p(out["mle"]), kf._p(sc_),
                               kf._p(out["gphi"]), kf._p(out["gq"]), kf._p(out["status"])))
    return out


@_route("test_loglik_grad")
def test_loglik_grad(shape, layout):
    """mk_loglik_grad (status prefilled with 0xA5A5A5A5) and the two-phase form, which returns the objective without a status."""
    for name in sc.CASES:
        c = sc.case(shape[0], shape[1], name)
        for v in _filters(*shape):
            bad, twin = _pair(c, layout, _grad_raw, **v)
            _check(c, bad, twin, "filter", "mk_loglik_grad %s %s" % (layout, v), warmup=0)

            def two_phase(kf, g):
                mle = kf.loglik_forward(g["phi"], g["q"], warmup=0, **cf.init(g))
                gphi, gq = kf.loglik_backward()
                return {"mle": mle, "gphi": gphi, "gq": gq}

            bad2, twin2 = _pair(c, layout, two_phase, **v)
            sc.check_containment(bad2, twin2, c, "two-phase gradient")
            sc.check_objective(bad2["mle"], c, 0, "two-phase gradient")
            assert all(np.array_equal(bad2[k], bad[k], equal_nan=True) for k in ("mle", "gphi", "gq")), (name, v)


@_route("test_loo_predict")
def test_loo_predict(shape, layout):
    for name in sc.CASES:
        c = sc.case(shape[0], shape[1], name)
        bad, twin = _pair(c, layout, lambda kf, g: {k: v for k, v in kf.loo_predict(g["phi"], g["q"], **cf.init(g)).items() if k != "_work"})
        _check(c, bad, twin, "filter", "loo_predict " + layout, warmup=0)


def test_no_leave_one_out_for_a_full_wavefront():
    kf = _engine(sc.case(60, 4, "neg_once")["bad"], "model_major")
    assert not kf.loo_supported()
    kf.close()


@_route("test_simulate_unconditional")
def test_simulate_unconditional(shape, layout):
    """simulate_unconditional (mk_draw_perturb against an all-zero record) has no status word: invalid parameters must show in the
    numbers.  A negative observation variance: the simulated record is NaN at every cell of that series, for every instance of
    the record; a NaN persistence: states, projections and record are NaN from the first step on.  Never a finite record for an
    invalid model, and the untouched instances bit-identical to the twin's."""
    N = shape[0]
    for name in sc.RECORD_CASES + ("nan_phi",):
        c = sc.case(shape[0], shape[1], name)
        bad, twin = _pair(c, layout, lambda kf, g: kf.simulate_unconditional(g["phi"], g["q"], 2, seed=ta.DRAW_SEED, P0=g["P0"], antithetic=True))
        assert set(bad) == {"xplus", "zxplus", "yplus"} and bad["yplus"].shape == (2, c["bad"]["B"], sc.T, N)
        sc.check_containment(bad, twin, c, "simulate_unconditional " + layout, axis=1)
        for i in range(c["bad"]["B"]):
            if i not in c["touched"]:
                assert all(np.isfinite(bad[k][:, i]).all() for k in bad), (name, i)
            elif name == "nan_phi":
                assert np.isnan(bad["yplus"][:, i]).all() and np.isnan(bad["zxplus"][:, i]).all() and np.isnan(bad["xplus"][:, i, :, N]).all(), (name, i)
            else:
                series = [0, 1] if name == "neg_twice_within" else [0]
                assert np.isnan(bad["yplus"][:, i][..., series]).all() and np.isfinite(bad["zxplus"][:, i]).all(), (name, i)


@_route("test_draw_smoothed")
def test_draw_smoothed(shape, layout):
    """Series and state draws (status [S,B]); the cases whose P0 has a Cholesky factor.  The untouched instances draw for draw
    against tests/draw_ref.py at the draws tier's bar; the draws of a flagged path are NaN, never finite numbers."""
    import draw_ref
    import oracle

    for name in sc.RECORD_CASES + ("nan_phi",):
        c = sc.case(shape[0], shape[1], name)
        g = c["bad"]
        for kind in ("series", "states"):
            bad, twin = _pair(c, layout, lambda kf, g_: kf.draw_smoothed(g_["phi"], g_["q"], 2, seed=ta.DRAW_SEED, what=kind, antithetic=True, **cf.init(g_)))
            tape = 16 < shape[0] + shape[1] <= 63 and kind == "series"
            what = "%s draws %s" % (kind, layout)
            sc.check_flags(bad["status"], c, "tape" if tape else "rts", what)
            sc.check_twin_flags(twin["status"], c, "tape" if tape else "rts", what)
            sc.check_containment({"draws": bad["draws"]}, {"draws": twin["draws"]}, c, what, axis=1)
            assert all(np.isnan(bad["draws"][:, i]).all() for i in c["touched"]), (what, name)
            for i in range(g["B"]):
                if i in c["touched"]:
                    continue
                r = i % g["R"]
                want = draw_ref.draw_model(oracle, g["obs"][r], g["phi"][i], g["q"][i], g["loadings"][r], 2, ta.DRAW_SEED, i, kind,
                                           g["obsvar"][r], g["x0"][i], g["P0"][i], g["scale"][r], g["offset"][r], antithetic=True)
                assert float(np.abs(bad["draws"][:, i] - want).max()) <= cf.DRAW_TOL, (what, name, i)


@_route("test_generic_family")
def test_generic_family(shape, layout):
    """kernel_family = generic (mk_generic.hip): filter, filter_smooth, the projection and the objective."""
    for name in sc.CASES:
        c = sc.case(shape[0], shape[1], name)
        bad, twin = _pair(c, layout, lambda kf, g: kf.filter(g["phi"], g["q"], **cf.init(g)), family="generic")
        _check(c, bad, twin, "filter", "generic filter " + layout)
        bad, twin = _pair(c, layout, lambda kf, g: kf.filter_smooth(g["phi"], g["q"], **cf.init(g)), family="generic")
        _check(c, bad, twin, "rts", "generic filter_smooth " + layout)
        bad, twin = _pair(c, layout, lambda kf, g: kf.simulate_smoothed(g["phi"], g["q"], **cf.init(g)), family="generic")
        _check(c, bad, twin, "rts", "generic simulate_smoothed " + layout, keys=("mle", "sim_means", "sim_vars"))
        for w in sc.WARMUPS:
            bad, twin = _pair(c, layout, lambda kf, g: {"mle": kf.loglik(g["phi"], g["q"], warmup=w, **cf.init(g))}, family="generic")
            sc.check_containment(bad, twin, c, "generic loglik")
            sc.check_objective(bad["mle"], c, w, "generic loglik")


def _smooth_raw(kf, g, F, Pf, prefill):
    """mk_smooth through the C ABI on dense filtered moments with d_status prefilled (engine.smooth hands over zeros)."""
    import torch
    from metran_amd._lib import Problem, check

    F, Pf = kf._layout(kf._dev(F)), kf._layout(kf._dev(Pf))
    B, T, n = (int(s) for s in F.shape)
    phi, q = kf._dev(g["phi"]), kf._dev(g["q"])
    prob = Problem(B, 1, T, g["N"], g["K"], 1, None, kf._p(phi), kf._p(q), None, None, None, None, 0, None, None)
    res = {"F": F, "Pf": Pf, "S": kf._empty_bt(B, T, n), "Ps": kf._empty_bt(B, T, n, n), "status": torch.zeros(B, dtype=torch.int32, device=kf.device)}
    if prefill:
        _prefill(res["status"])
    o = kf._outputs_struct(res)
    kf._bind_stream()
    check(kf._L.mk_smooth(kf._ctx, ctypes.byref(prob), ctypes.byref(o)))
    torch.cuda.synchronize()
    return {k: res[k] for k in ("S", "Ps", "status")}


def _smooth_dense_raw(kf, g, F, Pf, Xp, Pp):
    import torch
    from metran_amd._lib import check

    F, Pf, Xp, Pp, phi = (kf._dev(a) for a in (F, Pf, Xp, Pp, g["phi"]))
    B, T, n = (int(s) for s in F.shape)
    res = {"S": torch.empty((B, T, n), dtype=torch.float64, device=kf.device), "Ps": torch.empty((B, T, n, n), dtype=torch.float64, device=kf.device),
           "status": _prefill(torch.empty(B, dtype=torch.int32, device=kf.device))}
    kf._bind_stream()
    check(kf._L.mk_smooth_dense(kf._ctx, B, T, n, kf._p(phi), kf._p(F), kf._p(Pf), kf._p(Xp), kf._p(Pp), kf._p(res["S"]), kf._p(res["Ps"]),
                                kf._p(res["status"])))
    torch.cuda.synchronize()
    return res


@_route("test_smoother_entry_points")
def test_smoother_entry_points(shape, layout):
    """The ``indefinite`` case: the clean group filtered, Pf[T - 3] of instances 1 and 6 overwritten with -I, then mk_smooth
    (every RTS smoother of the shape, d_status prefilled with 0xA5A5A5A5 and through engine.smooth) and mk_smooth_dense:
    MK_FLAG_NOT_SPD | MK_FLAG_RANK_DEFICIENT on those two, nothing on the others, whose smoothed moments do not move."""
    g, touched = sc.indefinite_group(*shape)
    c = dict(name="indefinite", bad=g, twin=g, touched=touched)
    want = [(0, sc.FLAG_NOT_SPD | sc.FLAG_RANK_DEFICIENT if i in touched else 0) for i in range(g["B"])]
    kf = _engine(g, "model_major")
    r = kf.filter(g["phi"], g["q"], **cf.init(g))
    clean = [sc._np(r[k]).copy() for k in ("F", "Pf", "Xp", "Pp")]
    kf.close()
    broken = sc.indefinite_moments(g, touched, *clean)
    for v in _smoothers(*shape):
        kf = _engine(g, layout, **v)
        what = "mk_smooth %s %s" % (layout, v)
        bad, twin = _host(_smooth_raw(kf, g, broken[0], broken[1], True)), _host(_smooth_raw(kf, g, clean[0], clean[1], True))
        eng = _host(kf.smooth(g["phi"], g["q"], broken[0], broken[1]))
        kf.close()
        sc.check_status_values(bad["status"], want, what)
        sc.check_status_values(eng["status"], want, what + " (engine.smooth)")
        sc.check_status_values(twin["status"], [(0, 0)] * g["B"], what + " (clean)")
        sc.check_containment(bad, twin, c, what)
        sc.check_clean(bad, c, what)
    kf = _engine(g, layout)
    bad, twin = _host(_smooth_dense_raw(kf, g, *broken)), _host(_smooth_dense_raw(kf, g, *clean))
    kf.close()
    sc.check_status_values(bad["status"], want, "mk_smooth_dense")
    sc.check_status_values(twin["status"], [(0, 0)] * g["B"], "mk_smooth_dense (clean)")
    sc.check_containment(bad, twin, c, "mk_smooth_dense")
    sc.check_clean(bad, c, "mk_smooth_dense")


@_route("test_prefilled_status")
def test_prefilled_status(shape, layout):
    """mk_filter, mk_filter_smooth and mk_loo with d_status = 0xA5A5A5A5 on entry (the engine's ``buffers=`` hand the caller's
    arrays to the C ABI as they are): exactly the expected bits come back.  (mk_loglik_grad, mk_smooth, mk_smooth_dense:
    test_loglik_grad and test_smoother_entry_points.  (60,4), a full wavefront, has no mk_loo.)"""
    def filt(kf, g):
        res = kf._alloc_outputs(g["B"], ("F", "Pf", "Xp", "Pp"))
        _prefill(res["status"])
        return kf.filter(g["phi"], g["q"], buffers=res, **cf.init(g))

    def both(kf, g):
        res = kf._alloc_outputs(g["B"], ("F", "Pf", "Xp", "Pp", "S", "Ps"))
        _prefill(res["status"])
        return kf.filter_smooth(g["phi"], g["q"], buffers=res, **cf.init(g))

    def loo(kf, g):
        res = kf.alloc_loo(g["B"])
        _prefill(res["status"])
        return {"status": kf.loo_predict(g["phi"], g["q"], buffers=res, **cf.init(g))["status"]}

    for name in sc.CASES:
        c = sc.case(shape[0], shape[1], name)
        for fn, kind, abi in ((filt, "filter", "mk_filter"), (both, "rts", "mk_filter_smooth")) + (((loo, "filter", "mk_loo"),) if shape != (60, 4) else ()):
            bad, twin = _pair(c, layout, fn)
            sc.check_flags(bad["status"], c, kind, abi + " prefilled")
            sc.check_twin_flags(twin["status"], c, kind, abi + " prefilled")

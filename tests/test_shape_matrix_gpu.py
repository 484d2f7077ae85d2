"""GPU tier: every entry point that serves a shape, on the boundary shapes of tests/shape_matrix.py (both sides of every
compile-time switch of the specialised kernels), with the hard models of the property sweep (tests/hard_models.py: empty first
and last steps, never-observed series, persistence up to 1 - 1e-9, observation variances, non-default initial moments).

Per shape two groups, a short one (11 models) and a longer one (9 models): odd batches, so that the last wavefront of the split
layout (two or four models each) is partly empty.  Bars: the property sweep's (hard_models.mle_tolerance, filter_tolerances,
smoother_tolerance: the repository's 1e-9 / 1e-10 / 1e-9 plus the reference algorithm's own conditioning), the adjoint
gradient 1e-7 relative to its largest component (tests/test_adjoint.py), the two gradient walks against each other as in
tests/test_adjoint.py (the objective bit for bit, the gradient 1e-12 relative plus the conditioning term), and the leave-one-out predictions 1e-12 against their numpy restatement (tests/test_loo_gpu.py; plus
the conditioning term of the hard models) and the smoother's bar against masking one cell."""
import numpy as np
import pytest

import adjoint_ref
import hard_models
import loo_ref
import oracle
import shape_matrix

pytestmark = pytest.mark.gpu

STATE_KEYS = ("F", "Pf", "Xp", "Pp")
VARIANT_ERR = "round-1 wide smoother"


def _np(t):
    return t.detach().cpu().numpy()


def _take(g, B):
    """The first B models of a group."""
    out = dict(g, patterns=g["patterns"][:B])
    for k in ("obs", "phi", "q", "loadings", "obsvar", "x0", "P0"):
        out[k] = None if g[k] is None else g[k][:B]
    return out


def _groups():
    out = []
    for (N, K, T, B), g in hard_models.groups(shapes=shape_matrix.MATRIX, per_shape=21):
        if B % 2 == 0:
            g, B = _take(g, B - 1), B - 1
        out.append(((N, K, T, B), g))
    return out


GROUPS = _groups()
IDS = ["%dx%d_T%d_B%d" % key for key, _ in GROUPS]
_REFS = {}


def _refs(key, g, tag=""):
    """The oracle on every model of a group (computed once per group; ``tag``: a variant of the group, e.g. without R)."""
    if (key, tag) not in _REFS:
        _REFS[(key, tag)] = [hard_models.oracle_model(oracle, g, b) for b in range(key[3])]
    return _REFS[(key, tag)]


@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    import os

    old = os.environ.get("METRAN_HIP_CACHE")
    if old is None:
        os.environ["METRAN_HIP_CACHE"] = str(tmp_path_factory.getbasetemp() / "mkjit")
    yield
    if old is None:
        os.environ.pop("METRAN_HIP_CACHE", None)


def _engine(g, layout="model_major", packed_sym=False, obsvar="group"):
    from metran_amd.engine import BatchedKalman

    kf = BatchedKalman(0, layout=layout, packed_sym=packed_sym)
    kf.set_observations(g["obs"]).set_loadings(g["loadings"], g["obsvar"] if obsvar == "group" else obsvar)
    return kf


def _run(kf, fn, g, **kw):
    return getattr(kf, fn)(g["phi"], g["q"], x0=g["x0"], P0=g["P0"], **kw)


def _check_filter(r, g, refs, what, records=True, smoothed=True, unpack=None):
    from metran_amd.engine import FLAG_NONPOSITIVE_F, FLAG_NOT_SPD

    assert not (int(np.bitwise_or.reduce(_np(r["status"]))) & (FLAG_NONPOSITIVE_F | FLAG_NOT_SPD)), what
    full = {k: _np(unpack(r[k]) if unpack and k in ("Pf", "Pp", "Ps") else r[k]) for k in STATE_KEYS + ("S", "Ps") if k in r}
    if unpack:
        for k in ("Pf", "Pp", "Ps"):
            np.testing.assert_array_equal(full[k], np.swapaxes(full[k], -1, -2), err_msg=what + " " + k)
    for b, ref in enumerate(refs):
        w = "%s: model %d (%s)" % (what, b, g["patterns"][b])
        sc = ref["sigmacount"]
        assert abs(_np(r["mle"])[b] - ref["mle"]) <= hard_models.mle_tolerance(g, b, ref), w
        atol_sig, atol_mom = hard_models.filter_tolerances(g, b, ref)
        if records:
            assert int(_np(r["sigmacount"])[b]) == sc, w
            np.testing.assert_allclose(_np(r["sigmas"])[b, :sc], ref["sigmas"][:sc], rtol=1e-9, atol=atol_sig, err_msg=w)
            np.testing.assert_allclose(_np(r["detfs"])[b, :sc], ref["detfs"][:sc], rtol=0,
                                       atol=1e-10 + 1e-15 / float(g["q"][b].min()), err_msg=w)
            assert not _np(r["sigmas"])[b, sc:].any() and not _np(r["detfs"])[b, sc:].any(), w
        for k in STATE_KEYS:
            np.testing.assert_allclose(full[k][b], ref[k], rtol=0, atol=atol_mom, err_msg=w + " " + k)
        if smoothed:
            tol = hard_models.smoother_tolerance(g, b, ref)
            np.testing.assert_allclose(full["S"][b], ref["S"], rtol=0, atol=tol, err_msg=w + " S")
            np.testing.assert_allclose(full["Ps"][b], ref["Ps"], rtol=0, atol=tol, err_msg=w + " Ps")


@pytest.mark.parametrize("key,g", GROUPS, ids=IDS)
def test_filter_smooth_every_kernel(key, g, jit_cache):
    """filter_smooth in both layouts and with packed-symmetric records; for the wide shapes every wide-filter kernel that serves
    the shape and every wide-smoother variant."""
    from metran_amd._lib import MetranHipError

    N, K, T, B = key
    n = N + K
    refs = _refs(key, g)
    for layout in ("model_major", "time_major"):
        kf = _engine(g, layout)
        assert kf.specialised()
        _check_filter(_run(kf, "filter_smooth", g), g, refs, layout)
        kf.close()
    kf = _engine(g, "time_major" if T % 2 else "model_major", packed_sym=True)
    r = _run(kf, "filter_smooth", g)
    assert r["Pf"].shape == (B, T, n * (n + 1) // 2)
    _check_filter(r, g, refs, "packed_sym", unpack=kf.unpack_sym)
    kf.close()
    if n <= 16:
        return
    kf = _engine(g)
    if N <= 32:   # the split layout (the tier's default, tests/conftest.py) and one state per lane
        for wf in ("split", "lane_per_state"):
            kf.set_variant("wide_filter", wf)
            _check_filter(_run(kf, "filter_smooth", g), g, refs, "wide_filter " + wf)
        kf.set_variant("wide_filter", "split")
    for ws in ("v1", "mfma_unfolded", "mfma"):
        kf.set_variant("wide_smoother", ws)
        if ws == "v1" and not shape_matrix.SWITCHES["v1"][1](N, K):   # the round-1 kernel is built up to n = 51 only
            with pytest.raises(MetranHipError, match=VARIANT_ERR):
                _run(kf, "filter_smooth", g)
            continue
        _check_filter(_run(kf, "filter_smooth", g), g, refs, "wide_smoother " + ws)
    kf.close()


@pytest.mark.parametrize("key,g", GROUPS, ids=IDS)
def test_projection_and_state_variances_every_route(key, g, jit_cache):
    """simulate_smoothed and smooth_state_variances on the tape (16 < n <= 63; both tape writers where N <= 32) and on the
    filtered records, with a scaling, with the group's observation variances and without any."""
    N, K, T, B = key
    n = N + K
    rng = np.random.default_rng(N * 1000 + K * 100 + T)
    scale, offset = rng.uniform(0.5, 2.0, (B, N)), rng.normal(size=(B, N))
    served = shape_matrix.SWITCHES["tape"][1](N, K) and n > 16
    writers = ["observable", "state"] if served and N <= 32 else [None]
    if g["obsvar"] is None:   # the group as drawn, and the same models with observation variances (or without them)
        variants = [("", g), ("R", dict(g, obsvar=rng.uniform(0.0, 0.5, (B, N)) * (rng.random((B, N)) < 0.5)))]
    else:
        variants = [("", g), ("R0", dict(g, obsvar=None))]
    for tag, gg in variants:
        refs = _refs(key, gg, tag)
        kf = _engine(gg, "time_major" if T % 2 else "model_major")
        kf.set_scaling(scale, offset)
        assert kf.tape_path() == served
        for writer in writers:
            if writer:
                kf.set_variant("tape_filter", writer)
            for route in (["auto", "records"] if served else ["auto"]):
                kf.projection_path = route
                p = _run(kf, "simulate_smoothed", gg)
                s = _run(kf, "smooth_state_variances", gg)
                assert bool(p.get("_tape")) == (route == "auto" and served)
                assert bool(s.get("_tape")) == (route == "auto" and served and gg["obsvar"] is None)
                for b, ref in enumerate(refs):
                    what = "model %d (%s), route %s, writer %s, R %s" % (b, gg["patterns"][b], route, writer, gg["obsvar"] is not None)
                    tol = hard_models.smoother_tolerance(gg, b, ref)
                    Z = ref["Z"] * scale[b][:, None]
                    m_ref = ref["S"] @ Z.T + offset[b]
                    v_ref = np.maximum(np.einsum("jn,tnm,jm->tj", Z, ref["Ps"], Z), 0.0)
                    sc2 = float(scale[b].max()) ** 2
                    np.testing.assert_allclose(_np(p["sim_means"])[b], m_ref, rtol=0, atol=2 * tol * sc2, err_msg=what + " sim_means")
                    np.testing.assert_allclose(_np(p["sim_vars"])[b], v_ref, rtol=0, atol=2 * tol * sc2, err_msg=what + " sim_vars")
                    np.testing.assert_allclose(_np(s["S"])[b], ref["S"], rtol=0, atol=tol, err_msg=what + " state means")
                    np.testing.assert_allclose(_np(s["var"])[b], np.diagonal(ref["Ps"], axis1=1, axis2=2), rtol=0, atol=tol,
                                               err_msg=what + " state variances")
                    for out in (p, s):
                        assert abs(_np(out["mle"])[b] - ref["mle"]) <= hard_models.mle_tolerance(gg, b, ref), what
        kf.close()


@pytest.mark.parametrize("key,g", GROUPS, ids=IDS)
def test_objective_and_gradient(key, g, jit_cache):
    """loglik at warm-up 0, 1 and 2; loglik_grad with and without the update tape, against each other and against the numpy
    adjoint; the sparse objective (several parameter sets on one record) where n <= 16."""
    N, K, T, B = key
    n = N + K
    refs = _refs(key, g)
    kf = _engine(g)
    for warm in (0, 1, 2):
        got = _np(kf.loglik(g["phi"], g["q"], warmup=warm, x0=g["x0"], P0=g["P0"]))
        for b, ref in enumerate(refs):
            o, oi, oc = oracle.set_observations(g["obs"][b])
            sc = ref["sigmacount"]
            want = oracle.get_mle(ref["sigmas"][:sc], ref["detfs"][:sc], oc, warmup=warm)
            assert abs(got[b] - want) <= hard_models.mle_tolerance(g, b, ref, want), (b, warm, g["patterns"][b])
    assert kf.has_adjoint()
    kf.close()
    # the gradient with the update tape and with the recomputing walk, both behind the one-model-per-wavefront filter (the
    # update tape's writer: the same forward kernel on both sides, as in tests/test_adjoint.py), and -- where N <= 32 -- the
    # recomputing walk behind the split-layout filter (the tier's default, tests/conftest.py)
    res = {}
    for upd, wf in ((True, "lane_per_state"), (False, "lane_per_state"), (False, "split")):
        if wf == "split" and not (n > 16 and N <= 32):
            continue
        kf = _engine(g)
        if n > 16:
            kf.set_variant("wide_filter", wf)
        kf.adjoint_updates = upd
        res[upd, wf] = tuple(_np(t) for t in _run(kf, "loglik_grad", g))
        assert (getattr(kf, "_grad_upd", None) is not None) == (upd and n > 16)
        kf.close()
    tape, walk = res[True, "lane_per_state"], res[False, "lane_per_state"]
    assert np.array_equal(tape[0], walk[0])   # the objective does not know about the tape
    for b, ref in enumerate(refs):
        # the two walks form (d, 1/f, v) in different arithmetic: rounding, amplified like everything divided by f
        # (hard_models.conditioning: ~1e-15 for an ordinary model)
        c = hard_models.conditioning(g, b, ref)
        for i, name in ((1, "gphi"), (2, "gq")):
            assert np.abs(tape[i][b] - walk[i][b]).max() <= (1e-12 + c) * max(1.0, np.abs(walk[i][b]).max()), (b, name, g["patterns"][b])
    for (upd, wf), (f, gphi, gq) in res.items():
        for b, ref in enumerate(refs):
            assert abs(f[b] - ref["mle"]) <= hard_models.mle_tolerance(g, b, ref), (b, upd, wf)
        for b in range(0, B, max(1, B // 3)):
            if g["phi"][b].max() > 1.0 - 1e-6:
                continue   # d/dq of a model with q ~ 1e-9 is ~1e9: covered by the objective itself
            _, rphi, rq = adjoint_ref.gradient(g["obs"][b], g["phi"][b], g["q"][b], g["loadings"][b], 1,
                                               None if g["x0"] is None else g["x0"][b], None if g["P0"] is None else g["P0"][b],
                                               None if g["obsvar"] is None else g["obsvar"][b])
            for got, want, name in ((gphi[b], rphi, "gphi"), (gq[b], rq, "gq")):
                assert np.abs(got - want).max() <= 1e-7 * max(1.0, np.abs(want).max()), (b, name, upd, wf, g["patterns"][b])
    if n > 16:
        return
    from metran_amd.engine import BatchedKalman

    for b in (0, B - 1):
        kf = BatchedKalman(0)
        kf.set_observations(g["obs"][b:b + 1]).set_loadings(g["loadings"][b:b + 1], None if g["obsvar"] is None else g["obsvar"][b:b + 1])
        S = 5
        rng = np.random.default_rng(b)
        phi = np.clip(g["phi"][b][None] * (1.0 + 0.01 * rng.standard_normal((S, n))), 0.0, 1.0 - 1e-10)
        q = g["q"][b][None] * (1.0 + 0.01 * rng.standard_normal((S, n)))
        x0 = None if g["x0"] is None else np.repeat(g["x0"][b:b + 1], S, 0)
        P0 = None if g["P0"] is None else np.repeat(g["P0"][b:b + 1], S, 0)
        got = _np(kf.loglik(phi, q, x0=x0, P0=P0))
        for s in range(S):
            gs = dict(g, phi=phi[s][None], q=q[s][None], obs=g["obs"][b:b + 1], loadings=g["loadings"][b:b + 1],
                      obsvar=None if g["obsvar"] is None else g["obsvar"][b:b + 1],
                      x0=None if g["x0"] is None else g["x0"][b:b + 1], P0=None if g["P0"] is None else g["P0"][b:b + 1])
            ref = hard_models.oracle_model(oracle, gs, 0, smooth=False)
            assert abs(got[s] - ref["mle"]) <= hard_models.mle_tolerance(gs, 0, ref), (b, s, g["patterns"][b])
        kf.close()


@pytest.mark.parametrize("key,g", GROUPS, ids=IDS)
def test_leave_one_out(key, g, jit_cache):
    """loo_predict against the tape-walk restatement and, on two cells of the first models, against masking the cell and
    smoothing with the reference algorithm; n = 64 is refused."""
    from metran_amd._lib import MetranHipError

    N, K, T, B = key
    n = N + K
    kf = _engine(g, "time_major" if (N + T) % 2 else "model_major")
    if n > 63:
        assert not kf.loo_supported()
        with pytest.raises(MetranHipError, match="N=%d, K=%d" % (N, K)):
            _run(kf, "loo_predict", g)
        kf.close()
        return
    assert kf.loo_supported()
    rng = np.random.default_rng(N * 100 + K)
    scale, offset = rng.uniform(0.5, 2.0, (B, N)), rng.normal(size=(B, N))
    kf.set_scaling(scale, offset)
    r = _run(kf, "loo_predict", g)
    gm, gv = _np(r["loo_means"]), _np(r["loo_vars"])
    seen = np.isfinite(g["obs"])
    assert np.array_equal(np.isnan(gm), ~seen) and np.array_equal(np.isnan(gv), ~seen)
    refs = _refs(key, g)
    for b in range(B):
        if not seen[b].any():
            continue
        Rb = None if g["obsvar"] is None else g["obsvar"][b]
        x0 = None if g["x0"] is None else g["x0"][b]
        P0 = None if g["P0"] is None else g["P0"][b]
        what = "model %d (%s)" % (b, g["patterns"][b])
        m, v = loo_ref.loo_tape(g["obs"][b], g["phi"][b], g["q"][b], g["loadings"][b], Rb, x0, P0)
        m = m * scale[b] + offset[b]
        v = np.maximum(v, 0.0) * scale[b] ** 2
        c = hard_models.conditioning(g, b, refs[b])
        big, bigv = max(1.0, np.nanmax(np.abs(m[seen[b]]))), max(1.0, np.nanmax(v[seen[b]]))
        np.testing.assert_allclose(gm[b][seen[b]], m[seen[b]], rtol=0, atol=(1e-12 + c) * big, err_msg=what + " means")
        np.testing.assert_allclose(gv[b][seen[b]], v[seen[b]], rtol=0, atol=(1e-12 + c) * bigv, err_msg=what + " vars")
        if b < 2:
            tol = hard_models.smoother_tolerance(g, b, refs[b])
            cells = loo_ref.sample_cells(g["obs"][b], rng, 2)
            bm, bv = loo_ref.loo_brute(oracle, g["obs"][b], g["phi"][b], g["q"][b], g["loadings"][b], cells, Rb, x0, P0)
            js = [c_[1] for c_ in cells]
            np.testing.assert_allclose([gm[b][c_] for c_ in cells], bm * scale[b][js] + offset[b][js], rtol=0,
                                       atol=tol * float(scale[b].max()), err_msg=what + " masked means")
            np.testing.assert_allclose([gv[b][c_] for c_ in cells], np.maximum(bv, 0.0) * scale[b][js] ** 2, rtol=0,
                                       atol=tol * float(scale[b].max()) ** 2, err_msg=what + " masked vars")
    kf.close()


@pytest.mark.parametrize("key,g", GROUPS, ids=IDS)
def test_generic_kernel_family(key, g, jit_cache):
    """The size-generic kernels (mk_generic.hip) on the same groups: the six state arrays, the objective, the projection and the
    state variances."""
    N, K, T, B = key
    kf = _engine(g, "model_major" if (N + T) % 2 else "time_major")
    kf.set_variant("kernel_family", "generic")
    assert not kf.has_adjoint() and not kf.tape_path() and not kf.loo_supported()
    refs = _refs(key, g)
    r = _run(kf, "filter_smooth", g)
    _check_filter(r, g, refs, "generic")
    s = _run(kf, "smooth_state_variances", g)
    p = _run(kf, "simulate_smoothed", g)
    mle = _np(kf.loglik(g["phi"], g["q"], x0=g["x0"], P0=g["P0"]))
    for b, ref in enumerate(refs):
        what = "model %d (%s)" % (b, g["patterns"][b])
        for val in (mle[b], _np(s["mle"])[b], _np(p["mle"])[b]):
            assert abs(val - ref["mle"]) <= hard_models.mle_tolerance(g, b, ref), what
        tol = hard_models.smoother_tolerance(g, b, ref)
        np.testing.assert_allclose(_np(s["S"])[b], ref["S"], rtol=0, atol=tol, err_msg=what + " state means")
        np.testing.assert_allclose(_np(s["var"])[b], np.diagonal(ref["Ps"], axis1=1, axis2=2), rtol=0, atol=tol,
                                   err_msg=what + " state variances")
        np.testing.assert_allclose(_np(p["sim_means"])[b], ref["S"] @ ref["Z"].T, rtol=0, atol=2 * tol, err_msg=what + " sim_means")
        np.testing.assert_allclose(_np(p["sim_vars"])[b], np.maximum(np.einsum("jn,tnm,jm->tj", ref["Z"], ref["Ps"], ref["Z"]), 0.0),
                                   rtol=0, atol=2 * tol, err_msg=what + " sim_vars")
    kf.close()


# ------------------------------------------------------------------- filter_wave_kernel: the forms no other test launches
# The one-model-per-wavefront filter (mk_kernels.hip: filter_wave_kernel<N, K, OUT, BOOK, SYM>) is launched by the tests above
# and by tests/test_innovations_gpu.py (OUT 0 with BOOK) and tests/test_status_gpu.py (OUT 2) in every form but three: the
# filtered packed-symmetric record alone (OUT 3, SYM) and the two tapes with per-step sigmas / detfs booked (OUT 4, BOOK).
WAVE_FORMS = {
    "filtered_record_sym": (13, 4),    # n = 17, the narrowest wide shape; simulate_smoothed of a packed_sym engine
    "tape_booked": (33, 4),            # N > 32: the tape's writer; simulate_smoothed with dense sigmas / detfs attached
    "state_tape_booked": (33, 4),      # ... and smooth_state_variances over the STATE tape
}


def _wave_group(N, K):
    """B = 3: one surplus wavefront in the 4-model workgroup (the inst > B - 1 clamp).  T = 18: one tile edge and the row clamp
    of the second tile.  30 % of the cells missing (hard_models' "iid") and one step fully empty, another one per model, so
    that the compressed index falls behind t (the scattered pad store).  No observation variances: the STATE tape serves R = 0."""
    B, T = 3, 18
    rng = np.random.default_rng([N, K, T, B])
    g = dict(obs=np.empty((B, T, N)), phi=np.empty((B, N + K)), q=np.empty((B, N + K)), loadings=np.empty((B, N, K)),
             patterns=["iid + empty step %d" % (3 + 5 * b) for b in range(B)], obsvar=None, x0=None, P0=None)
    for b in range(B):
        g["obs"][b], g["phi"][b], g["q"][b], g["loadings"][b] = hard_models.draw_model(rng, N, K, T, "iid")
        g["obs"][b, 3 + 5 * b] = np.nan
        assert np.isfinite(g["obs"][b, -1]).any() and 0.2 < np.isnan(g["obs"][b]).mean() < 0.45
    return g


@pytest.mark.parametrize("layout", ["model_major", "time_major"])
@pytest.mark.parametrize("form", sorted(WAVE_FORMS))
def test_wave_filter_remaining_forms(form, layout, jit_cache):
    N, K = WAVE_FORMS[form]
    n, B, T = N + K, 3, 18
    g = _wave_group(N, K)
    refs = _refs((N, K, T, B), g, "wave forms")
    kf = _engine(g, layout, packed_sym=(form == "filtered_record_sym"))
    kf.set_variant("wide_filter", "lane_per_state")
    if form == "filtered_record_sym":
        assert not kf.tape_path()
        r = _run(kf, "simulate_smoothed", g)
        assert "_tape" not in r and r["Pf"].shape == (B, T, n * (n + 1) // 2)
    else:
        assert kf.tape_path() and kf.state_tape_path()
        bufs = kf.alloc_projection(B) if form == "tape_booked" else kf.alloc_state_variances(B)
        bufs["sigmas"], bufs["detfs"] = kf._empty_bt(B, T), kf._empty_bt(B, T)
        r = _run(kf, "simulate_smoothed" if form == "tape_booked" else "smooth_state_variances", g, buffers=bufs)
        assert r["_tape"]
    assert not int(np.bitwise_or.reduce(_np(r["status"])))
    sig, det = _np(r["sigmas"]), _np(r["detfs"])
    for b, ref in enumerate(refs):
        w = "%s %s: model %d (%s)" % (form, layout, b, g["patterns"][b])
        sc = ref["sigmacount"]
        assert sc == T - 1, w
        assert abs(_np(r["mle"])[b] - ref["mle"]) <= hard_models.mle_tolerance(g, b, ref), w
        atol_sig, atol_mom = hard_models.filter_tolerances(g, b, ref)
        assert int(_np(r["sigmacount"])[b]) == sc, w
        np.testing.assert_allclose(sig[b, :sc], ref["sigmas"][:sc], rtol=1e-9, atol=atol_sig, err_msg=w)
        np.testing.assert_allclose(det[b, :sc], ref["detfs"][:sc], rtol=0, atol=1e-10 + 1e-15 / float(g["q"][b].min()), err_msg=w)
        assert not sig[b, sc:].any() and not det[b, sc:].any(), w
        tol = hard_models.smoother_tolerance(g, b, ref)
        if form == "filtered_record_sym":
            np.testing.assert_allclose(_np(r["F"])[b], ref["F"], rtol=0, atol=atol_mom, err_msg=w + " F")
            np.testing.assert_allclose(_np(kf.unpack_sym(r["Pf"]))[b], ref["Pf"], rtol=0, atol=atol_mom, err_msg=w + " Pf")
        if form == "state_tape_booked":
            np.testing.assert_allclose(_np(r["S"])[b], ref["S"], rtol=0, atol=tol, err_msg=w + " state means")
            np.testing.assert_allclose(_np(r["var"])[b], np.diagonal(ref["Ps"], axis1=1, axis2=2), rtol=0, atol=tol,
                                       err_msg=w + " state variances")
        else:
            Z = ref["Z"]
            np.testing.assert_allclose(_np(r["sim_means"])[b], ref["S"] @ Z.T, rtol=0, atol=2 * tol, err_msg=w + " sim_means")
            np.testing.assert_allclose(_np(r["sim_vars"])[b], np.maximum(np.einsum("jn,tnm,jm->tj", Z, ref["Ps"], Z), 0.0),
                                       rtol=0, atol=2 * tol, err_msg=w + " sim_vars")
    kf.close()

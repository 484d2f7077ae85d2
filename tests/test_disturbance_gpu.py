"""Smoothed state disturbances on the GPU (C ABI mk_disturbances: adjoint_kernel for N + K <= 16, adjoint_wide_kernel for
16 < N + K <= 64, each in its disturbance mode): against the numpy restatements (tests/disturbance_ref.py, pinned to the oracle
and to the dense joint Gaussian by tests/test_disturbance_host.py), at the walkers' prologue lengths, with more instances than
records, next to an invalid model, under two warm-ups, the refusals, and end to end through MetranBatch."""
import ctypes
import functools

import numpy as np
import pytest

import call_forms as cf
import disturbance_ref as dr
import oracle
import status_cases as sc
from test_loo_gpu import _batch

pytestmark = pytest.mark.gpu

# (12,4): n = 16, the last shape of the 16-lane walk; (13,4): the first of the one-model-per-wavefront walk; (60,4): n = 64
SHAPES = [(8, 2), (5, 1), (12, 4), (13, 4), (32, 4), (33, 4), (60, 4)]
RAW_TOL = 1e-12        # against dist_adjoint, relative to the largest modulus (tests/test_loo_gpu.py's bar against its restatement)
SMOOTH_BAR = 1e-9      # against dist_definition / dist_joint: the smoothed moments' bar (tests/test_hip_parity.py: SMOOTH_ATOL)


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module", params=["model_major", "time_major"])
def layout(request):
    return request.param


@pytest.fixture(scope="module", autouse=True)
def jit_cache(tmp_path_factory):
    import os

    old = os.environ.get("METRAN_HIP_CACHE")
    if old is None:
        os.environ["METRAN_HIP_CACHE"] = str(tmp_path_factory.getbasetemp() / "mkjit")
    yield
    if old is None:
        os.environ.pop("METRAN_HIP_CACHE", None)


def _assert_raw(got_r, got_n, want_r, want_n, what):
    assert got_r.shape == want_r.shape and got_n.shape == want_n.shape, what
    er, en = np.abs(got_r - want_r).max(), np.abs(got_n - want_n).max()
    assert er <= RAW_TOL * max(1.0, np.abs(want_r).max()), "%s: r is %.3g from the restatement" % (what, er)
    assert en <= RAW_TOL * max(1.0, np.abs(want_n).max()), "%s: N_ii is %.3g from the restatement" % (what, en)
    assert (got_n >= 0).all(), what


def _oracle_moments(y, phi, q, G, R, x0, P0):
    N, K = G.shape
    n = N + K
    Z = np.concatenate([np.eye(N), G], axis=1)
    o, oi, oc = oracle.set_observations(y)
    _, _, _, F, Pf, Xp, Pp = oracle.seqkalmanfilter(o, np.diag(phi), np.diag(q), Z, np.zeros(N) if R is None else R, oi, oc,
                                                    np.zeros(n) if x0 is None else x0, np.eye(n) if P0 is None else P0)
    S, Ps = oracle.kalmansmoother(F, Pf, Xp, Pp, np.diag(phi))
    return F, Pf, Xp, Pp, S, Ps


# ---- 1. against the references ----
@functools.lru_cache(maxsize=None)
def _reference_case(shape, with_r, with_init):
    """Inputs and both references of one case, computed once and shared by the two layouts (read-only)."""
    N, K = shape
    n = N + K
    d, obs = _batch(N, K, seed=N * 10 + K)
    B = obs.shape[0]
    rng = np.random.default_rng(N + K)
    R = rng.uniform(0.05, 0.4, (B, N)) * (rng.random((B, N)) < 0.6) if with_r else None
    x0 = rng.normal(size=(B, n)) if with_init else None
    A = rng.normal(size=(B, n, n))
    P0 = A @ A.transpose(0, 2, 1) / n + 0.5 * np.eye(n) if with_init else None
    opt = lambda a, b: None if a is None else a[b]  # noqa: E731
    raw, mom = [], []
    for b in range(B):
        args = (obs[b], d["phi"][b], d["q"][b], d["loadings"][b], opt(R, b), opt(x0, b), opt(P0, b))
        raw.append(dr.dist_adjoint(*args))
        mom.append(dr.dist_definition(d["phi"][b], d["q"][b], *_oracle_moments(*args)))
    out = dict(obs=obs, phi=d["phi"], q=d["q"], loadings=d["loadings"], R=R, x0=x0, P0=P0,
               r=np.stack([a for a, _ in raw]), ninfo=np.stack([b for _, b in raw]),
               mean=np.stack([a for a, _ in mom]), var=np.stack([b for _, b in mom]))
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("with_r", [False, True], ids=["R0", "R"])
@pytest.mark.parametrize("with_init", [False, True], ids=["default", "x0P0"])
def test_kernels_match_restatement_and_definition(shape, with_r, with_init, layout):
    from metran_amd.engine import BatchedKalman

    c = _reference_case(shape, with_r, with_init)
    kf = BatchedKalman(0, layout=layout)
    kf.set_observations(c["obs"]).set_loadings(c["loadings"], c["R"])
    assert kf.disturbances_supported()
    init = {} if c["x0"] is None else dict(x0=c["x0"], P0=c["P0"])
    out = kf.disturbances(c["phi"], c["q"], **init)
    assert int(out["status"].abs().sum().item()) == 0
    gr, gn = _np(out["r"]), _np(out["ninfo"])
    what = "(%d,%d) %s" % (shape[0], shape[1], layout)
    for b in range(gr.shape[0]):
        _assert_raw(gr[b], gn[b], c["r"][b], c["ninfo"][b], "%s instance %d" % (what, b))
    q = c["q"][:, None, :]
    em = np.abs(q * gr - c["mean"])[:, 1:].max()
    ev = np.abs(q - q * q * gn - c["var"])[:, 1:].max()
    print("%s: q r and q - q^2 N against dist_definition: %.2e, %.2e" % (what, em, ev))
    assert em <= SMOOTH_BAR and ev <= SMOOTH_BAR, what
    kf.close()


# ---- 2. the walkers' prologues ----
@pytest.mark.parametrize("T", [1, 2, 3])
@pytest.mark.parametrize("shape", [(8, 2), (13, 4), (32, 4), (5, 1)], ids=lambda s: "%dx%d" % s)
def test_prologue_lengths(shape, T, layout):
    """T = 1, 2 and 3: the prefetch prologue of each walk and its first steady iteration; (5,1) with x0 / P0 against the dense
    joint Gaussian, the one reference that covers t = 0."""
    from metran_amd.engine import BatchedKalman

    N, K = shape
    n = N + K
    d, obs = _batch(N, K, T=12, B=5, seed=3 * N + K)
    obs = obs[:, 4:4 + T].copy()            # a quarter of the cells missing
    obs[0, 0, 1:] = np.nan                  # instance 0 starts with a one-series step,
    obs[0, 0, 0] = 0.3
    obs[1, 0] = np.nan                      # instance 1 with an empty one (T = 1: no observation at all),
    obs[2, 0] = np.where(np.isfinite(obs[2, 0]), obs[2, 0], -0.4)   # instance 2 with a full one
    rng = np.random.default_rng(T)
    x0 = rng.normal(size=(5, n))
    A = rng.normal(size=(5, n, n))
    P0 = A @ A.transpose(0, 2, 1) / n + 0.5 * np.eye(n)
    kf = BatchedKalman(0, layout=layout)
    kf.set_observations(obs).set_loadings(d["loadings"])
    out = kf.disturbances(d["phi"], d["q"], x0=x0, P0=P0)
    assert int(out["status"].abs().sum().item()) == 0
    gr, gn = _np(out["r"]), _np(out["ninfo"])
    assert gr.shape == (5, T, n)
    for b in range(5):
        args = (obs[b], d["phi"][b], d["q"][b], d["loadings"][b], None, x0[b], P0[b])
        wr, wn = dr.dist_adjoint(*args)
        _assert_raw(gr[b], gn[b], wr, wn, "(%d,%d) T=%d instance %d" % (N, K, T, b))
        if shape == (5, 1):
            jm, jv = dr.dist_joint(*args)
            q = d["q"][b]
            assert np.abs(q * gr[b] - jm).max() <= SMOOTH_BAR and np.abs(q - q * q * gn[b] - jv).max() <= SMOOTH_BAR
    kf.close()


# ---- 3. instances and records ----
def _run_group(g, layout):
    from metran_amd.engine import BatchedKalman

    kf = BatchedKalman(0, layout=layout)
    kf.set_observations(g["obs"]).set_loadings(g["loadings"], g["obsvar"])
    out = kf.disturbances(g["phi"], g["q"], **cf.init(g))
    res = {"r": _np(out["r"]).copy(), "ninfo": _np(out["ninfo"]).copy(), "status": _np(out["status"]).copy()}
    kf.close()
    return res


@pytest.mark.parametrize("shape", [(8, 2), (13, 4), (60, 4)], ids=lambda s: "%dx%d" % s)
def test_more_instances_than_records(shape, layout):
    """R = 3 records, S = 5 parameter sets, B = 15: every instance against the restatement on ITS record, and the 15-instance
    call bit for bit the five 3-instance calls."""
    g = cf.group(*shape)
    assert (g["R"], g["S"], g["B"]) == (3, 5, 15)
    out = _run_group(g, layout)
    assert not out["status"].any()
    for i in range(g["B"]):
        r = i % g["R"]
        wr, wn = dr.dist_adjoint(g["obs"][r], g["phi"][i], g["q"][i], g["loadings"][r], g["obsvar"][r], g["x0"][i], g["P0"][i])
        _assert_raw(out["r"][i], out["ninfo"][i], wr, wn, cf._what(g, i))
    cf.check_position_independent(lambda grp: {k: v for k, v in _run_group(grp, layout).items() if k != "status"}, g,
                                  "disturbances (%d,%d) %s" % (shape[0], shape[1], layout))


# ---- 4. an invalid model next to valid ones ----
@pytest.mark.parametrize("shape", [(8, 2), (32, 4)], ids=lambda s: "%dx%d" % s)
def test_invalid_model_is_contained(shape, layout):
    c = sc.case(shape[0], shape[1], "neg_once")
    bad, twin = _run_group(c["bad"], layout), _run_group(c["twin"], layout)
    what = "disturbances (%d,%d) %s" % (shape[0], shape[1], layout)
    sc.check_flags(bad["status"], c, "filter", what)          # as mk_loo reports them: the filter's bits
    sc.check_twin_flags(twin["status"], c, "filter", what)
    sc.check_containment(bad, twin, c, what)


# ---- 5. the warm-up is ignored ----
@pytest.mark.parametrize("shape", [(8, 2), (13, 4)], ids=lambda s: "%dx%d" % s)
def test_independent_of_the_warmup(shape):
    from metran_amd import _lib
    from metran_amd.engine import BatchedKalman

    N, K = shape
    d, obs = _batch(N, K, T=12, B=3, seed=5)
    kf = BatchedKalman(0)
    kf.set_observations(obs).set_loadings(d["loadings"])
    phi, q = kf._dev(d["phi"]), kf._dev(d["q"])
    L = _lib.lib()
    got = []
    for warmup in (0, 3):
        prob, keep, B = kf._problem(phi, q, warmup, None, None)
        assert prob.warmup == warmup
        res = kf.alloc_disturbances(B)
        _lib.check(L.mk_disturbances(kf._ctx, ctypes.byref(prob), kf._p(res["_work"]), 0, kf._p(res["r"]), kf._p(res["ninfo"]),
                                     kf._p(res["status"])))
        got.append((_np(res["r"]).copy(), _np(res["ninfo"]).copy()))
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes()
    assert np.abs(got[0][0]).max() > 0
    kf.close()


# ---- 6. refusals ----
def test_unserved_shapes_and_buffers_are_refused():
    import torch

    from metran_amd import _lib
    from metran_amd._lib import MetranHipError, Problem
    from metran_amd.engine import BatchedKalman
    from metran_amd.synthetic import make_dfm_batch

    d = make_dfm_batch(2, 8, 2, 16, seed=3)
    kf = BatchedKalman(0)
    kf.set_observations(d["obs"]).set_loadings(d["loadings"])
    L = _lib.lib()
    phi, q = kf._dev(d["phi"]), kf._dev(d["q"])
    prob, keep, B = kf._problem(phi, q, 0, None, None)
    res = kf.alloc_disturbances(B)
    ptr = {k: kf._p(res[k]) for k in ("_work", "r", "ninfo")}
    # the size-generic kernel family has no such walk: the engine and the C ABI both say so
    kf.set_variant("kernel_family", "generic")
    assert not kf.disturbances_supported()
    with pytest.raises(MetranHipError, match="N=8, K=2"):
        kf.disturbances(d["phi"], d["q"])
    rc = L.mk_disturbances(kf._ctx, ctypes.byref(prob), ptr["_work"], 0, ptr["r"], ptr["ninfo"], None)
    assert rc == -2 and b"N=8, K=2" in L.mk_last_error()
    kf.set_variant("kernel_family", "specialised")
    assert kf.disturbances_supported()
    # a shape no specialised kernel serves: stride 0, MK_ERR_SHAPE before any launch
    assert L.mk_disturbance_work_stride(70, 2) == 0
    assert L.mk_disturbance_work_stride(8, 2) == L.mk_record_stride(10) and L.mk_disturbance_work_stride(32, 4) == L.mk_record_stride(36)
    buf = torch.zeros(72 * 72, dtype=torch.float64, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    wide = Problem(1, 1, 4, 70, 2, 0, p, p, p, p, None, None, None, 0, None, None)
    rc = L.mk_disturbances(kf._ctx, ctypes.byref(wide), p, 0, p, p, None)
    assert rc == -2 and b"N=70, K=2" in L.mk_last_error()
    # a missing buffer
    for name in ("_work", "r", "ninfo"):
        args = dict(ptr, **{name: None})
        rc = L.mk_disturbances(kf._ctx, ctypes.byref(prob), args["_work"], 0, args["r"], args["ninfo"], None)
        assert rc == -1 and b"d_work, d_r and d_ninfo are required" in L.mk_last_error()
    # a buffer smaller than the call needs (an allocation of its own: its size is known exactly)
    small = ctypes.c_void_p()
    assert L.mk_malloc(kf._ctx, 128, ctypes.byref(small)) == 0
    try:
        for name, label in (("_work", b"d_work"), ("r", b"d_r"), ("ninfo", b"d_ninfo")):
            args = dict(ptr, **{name: small})
            rc = L.mk_disturbances(kf._ctx, ctypes.byref(prob), args["_work"], 0, args["r"], args["ninfo"], None)
            assert rc == -1 and label + b" (" in L.mk_last_error(), (name, L.mk_last_error())
    finally:
        L.mk_free(kf._ctx, small)
    kf.close()


# ---- 7. end to end ----
def test_metran_batch_matches_smoothed_state_differences(g1):
    """MetranBatch on the worked example, two models of different lengths: the smoothed disturbance of every state is the
    smoothed state minus phi times the smoothed state of the step before (get_state_means), at sampled steps."""
    import pandas as pd

    from metran_amd.batch import MetranBatch

    idx = pd.DatetimeIndex(g1["index_ns"].astype("datetime64[ns]"))
    raw = g1["obs"] * g1["oseries_std"] + g1["oseries_mean"]
    series = [pd.Series(raw[:, j], index=idx, name="B21B021400%d" % (j + 1)).dropna() for j in range(raw.shape[1])]
    short = [s.iloc[: len(s) // 2] for s in series]
    mb = MetranBatch([series, short], factors=g1["loadings"])
    astar = np.stack([g1["alpha_star"], g1["alpha_star"] * 1.1])
    phi = _np(mb.kf.params_from_alpha(mb._alpha(astar), dt=mb.dt)[0])
    mean, var = (_np(t) for t in mb.get_state_disturbances(astar))
    u = _np(mb.get_auxiliary_residuals(astar))
    n = mb.N + mb.K
    assert mean.shape == var.shape == u.shape == (2, mb.T, n) and (var >= 0).all()
    rng = np.random.default_rng(0)
    for r in range(2):
        Lr = int(mb.batch.lengths[r])
        S = mb.get_state_means(r, alpha=astar).values
        assert S.shape == (Lr, n)
        ts = np.unique(np.concatenate([[1, 2, Lr // 2, Lr - 2, Lr - 1], rng.integers(1, Lr, 40)]))
        np.testing.assert_allclose(mean[r, ts], S[ts] - phi[r] * S[ts - 1], rtol=0, atol=1e-8)
        frame = mb.get_state_disturbance(r, n - 1, alpha=astar)
        assert list(frame.columns) == ["mean", "lower", "upper"] and frame.index.equals(mb.batch.index[r])
        np.testing.assert_allclose(frame["mean"].values[ts], (S[ts] - phi[r] * S[ts - 1])[:, n - 1], rtol=0, atol=1e-8)
        assert np.isnan(u[r, Lr:]).all() and np.isfinite(u[r, :Lr]).any()
    table = mb.screen_breaks(astar)
    assert table.shape == (2 * n, 4) and (table["nobs"] > 0).all() and table["pvalue"].between(0, 1).all()
    assert "dist" in mb._cache

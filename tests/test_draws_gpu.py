"""Posterior draws on the GPU (draw_kernels.hip behind mk_draw_normals / mk_draw_perturb / mk_draw_combine, and
BatchedKalman.draw_smoothed over the existing smoothing routes): against the numpy restatement (tests/draw_ref.py) number for
number and draw for draw, the exact identities of a draw against simulate_smoothed of the same engine, bit-for-bit
invariance under chunking / sub-ranges / layout, MetranBatch end to end, and the refusals."""
import ctypes

import numpy as np
import pytest

import draw_ref
import oracle
from conftest import golden_models
from metran_amd.synthetic import make_dfm_batch

pytestmark = pytest.mark.gpu

TOL = 1e-9        # the tier's smoothed-moment bar
PERTURB_TOL = 1e-11


def _np(t):
    return t.detach().cpu().numpy()


def _engine(layout="model_major"):
    from metran_amd.engine import BatchedKalman

    return BatchedKalman(0, layout=layout)


def _normals(kf, seed, first_instance, ninst, first_draw, ndraws, antithetic, T, ncomp, raw):
    import torch

    out = torch.full((ndraws, ninst, T + 1, ncomp), float("nan"), dtype=torch.float64, device="cuda")
    rc = kf._L.mk_draw_normals(kf._ctx, seed, first_instance, ninst, first_draw, ndraws, int(antithetic), T, ncomp, int(raw),
                               ctypes.c_void_p(out.data_ptr()))
    assert rc == 0, kf._L.mk_last_error()
    torch.cuda.synchronize()
    return _np(out)


@pytest.mark.parametrize("ncomp", [1, 10, 17])
def test_raw_integers_equal_the_restatement(ncomp):
    kf = _engine()
    seed = 0x9E3779B97F4A7C15
    got = _normals(kf, seed, 3, 4, 2, 3, False, 25, ncomp, True)
    want = draw_ref.normal_block(seed, 3, 4, 2, 3, False, 25, ncomp, raw=True)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("antithetic", [False, True])
def test_normals_match_the_restatement(antithetic):
    kf = _engine()
    got = _normals(kf, 77, 5, 6, 3, 5, antithetic, 200, 13, False)
    want = draw_ref.normal_block(77, 5, 6, 3, 5, antithetic, 200, 13)
    err = np.abs(got - want).max()
    print("normals: max abs error %.3e (largest |z| %.2f)" % (err, np.abs(want).max()))
    assert err <= 1e-13


def _batch(N, K, T, B, seed, missing=0.3):
    d = make_dfm_batch(B, N, K, T, seed=seed, missing=missing)
    obs = d["obs"].copy()
    obs[:, 0] = np.nan                       # an empty first step
    obs[B - 1, :, N - 1] = np.nan            # a series that is never observed
    return d, obs


def _extras(B, N, K, seed, full):
    """(obsvar, x0, P0, scale, offset) -- obsvar / x0 / P0 None unless ``full``."""
    rng = np.random.default_rng(seed)
    n = N + K
    scale, offset = rng.uniform(0.5, 2.0, (B, N)), rng.normal(size=(B, N))
    if not full:
        return None, None, None, scale, offset
    A = rng.normal(size=(B, n, n))
    return rng.uniform(0.05, 0.4, (B, N)), rng.normal(size=(B, n)), A @ A.transpose(0, 2, 1) / n + 0.5 * np.eye(n), scale, offset


def _perturb(kf, d, ndraws, seed, first_instance, first_draw, antithetic, P0):
    import torch

    prob, keep, B = kf._problem(d["phi"], d["q"], 1, None, P0)
    L0 = torch.linalg.cholesky(keep[3]).contiguous() if P0 is not None else None
    ystar, zx, xp = kf._draw_perturb(prob, B, ndraws, seed, first_instance, first_draw, antithetic, L0, True, True)
    torch.cuda.synchronize()
    return ystar, zx, xp


@pytest.mark.parametrize("layout", ["model_major", "time_major"])
@pytest.mark.parametrize("full", [False, True], ids=["defaults", "P0_R"])
@pytest.mark.parametrize("shape", [(8, 2, 5), (5, 1, 7), (32, 4, 3), (11, 6, 3), (70, 3, 1)], ids=lambda s: "%dx%d_B%d" % s)   # (11,6): factors beyond the four kept in registers
def test_perturb_matches_the_restatement(shape, full, layout):
    N, K, B = shape
    T, S, seed, fi, fd = 23, 3, 4242, 4, 3
    d, obs = _batch(N, K, T, B, seed=N + K)
    R, _, P0, _, _ = _extras(B, N, K, 1, full)
    kf = _engine(layout)
    kf.set_observations(obs).set_loadings(d["loadings"], R)
    for antithetic in (False, True):
        ystar, zx, xp = (_np(a).reshape(S, B, T, -1) for a in _perturb(kf, d, S, seed, fi, fd, antithetic, P0))
        ncomp = N + K + (N if full else 0)
        z = draw_ref.normal_block(seed, fi, B, fd, S, antithetic, T, ncomp)
        worst = 0.0
        for s in range(S):
            for i in range(B):
                L0 = None if P0 is None else np.linalg.cholesky(P0[i])
                rx, rzx, _, rys = draw_ref.unconditional(obs[i], d["phi"][i], d["q"][i], d["loadings"][i], z[s, i],
                                                        None if R is None else R[i], L0)
                assert np.array_equal(np.isnan(ystar[s, i]), ~np.isfinite(obs[i]))
                seen = np.isfinite(obs[i])
                worst = max(worst, np.abs(xp[s, i] - rx).max(), np.abs(zx[s, i] - rzx).max(), np.abs(ystar[s, i][seen] - rys[seen]).max())
        print("perturb %s %s antithetic=%s: max abs error %.3e" % (shape, layout, antithetic, worst))
        assert worst <= PERTURB_TOL


def test_perturb_on_the_edge_case_fixtures():
    """edge_cases.npz: an empty first step, a never-observed series and the other corner records of the golden set."""
    for k, m in golden_models("edge_cases.npz"):
        kf = _engine("time_major")
        kf.set_observations(m["obs"][None]).set_loadings(m["loadings"][None])
        d = {"phi": m["phi"][None], "q": m["q"][None]}
        T, N = m["obs"].shape
        ystar, zx, xp = (_np(a).reshape(2, T, -1) for a in _perturb(kf, d, 2, 9, 0, 0, False, None))
        z = draw_ref.normal_block(9, 0, 1, 0, 2, False, T, m["phi"].size)
        for s in range(2):
            rx, rzx, _, rys = draw_ref.unconditional(m["obs"], m["phi"], m["q"], m["loadings"], z[s, 0])
            seen = np.isfinite(m["obs"])
            assert np.array_equal(np.isnan(ystar[s]), ~seen), k
            assert np.abs(xp[s] - rx).max() <= PERTURB_TOL and np.abs(zx[s] - rzx).max() <= PERTURB_TOL
            assert not seen.any() or np.abs(ystar[s][seen] - rys[seen]).max() <= PERTURB_TOL


# (N, K, projection_path, kernel family, full = with obsvar / x0 / P0)
ROUTES = [(8, 2, "auto", "specialised", False), (8, 2, "auto", "specialised", True), (5, 1, "auto", "specialised", False),
          (14, 3, "auto", "specialised", False), (32, 4, "auto", "specialised", False), (32, 4, "auto", "specialised", True),
          (32, 4, "records", "specialised", False), (20, 2, "auto", "specialised", False), (48, 3, "auto", "specialised", False),
          (8, 2, "auto", "generic", False)]


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: "%dx%d_%s_%s_%s" % (r[0], r[1], r[2], r[3], "full" if r[4] else "plain"))
def test_draws_match_the_restatement(route):
    N, K, path, family, full = route
    B, T, S, seed = 3, 30, 4, 31337
    d, obs = _batch(N, K, T, B, seed=3 * N + K)
    R, x0, P0, scale, offset = _extras(B, N, K, 2, full)
    kf = _engine("time_major")
    kf.set_observations(obs).set_loadings(d["loadings"], R).set_scaling(scale, offset)
    kf.projection_path = path
    kf.set_variant("kernel_family", family)
    if path == "auto" and family == "specialised" and N + K > 16:
        assert kf.tape_path()
    base = kf.simulate_smoothed(d["phi"], d["q"], x0=x0, P0=P0)
    sim = _np(base["sim_means"]).copy()
    assert int(base["status"].abs().sum().item()) == 0
    for what in ("series", "states"):
        out = kf.draw_smoothed(d["phi"], d["q"], S, seed=seed, what=what, x0=x0, P0=P0, antithetic=True, first_draw=2, first_instance=5)
        got = _np(out["draws"])
        assert got.shape == (S, B, T, N if what == "series" else N + K) and tuple(out["status"].shape) == (S, B)
        assert int(out["status"].abs().sum().item()) == 0
        worst = 0.0
        for i in range(B):
            want = draw_ref.draw_model(oracle, obs[i], d["phi"][i], d["q"][i], d["loadings"][i], S, seed, 5 + i, what,
                                       None if R is None else R[i], None if x0 is None else x0[i], None if P0 is None else P0[i],
                                       scale[i], offset[i], antithetic=True, first_draw=2)
            worst = max(worst, np.abs(got[:, i] - want).max())
        print("draws %s %s: max abs error %.3e" % (route, what, worst))
        assert worst <= TOL
        if what == "series":
            # the antithetic pair (draws 2, 3) averages to the engine's own smoothed projection; an observed cell without
            # observation variance returns the observation
            assert np.abs(0.5 * (got[0] + got[1]) - sim).max() <= TOL
            assert np.abs(0.5 * (got[2] + got[3]) - sim).max() <= TOL
            if R is None:
                seen = np.isfinite(obs)
                want_obs = obs * scale[:, None] + offset[:, None]
                for s in range(S):
                    assert np.abs(got[s][seen] - want_obs[seen]).max() <= TOL
            assert np.abs(got[0] - got[2])[~np.isfinite(obs)].max() > 1e-3


@pytest.mark.parametrize("shape", [(8, 2), (32, 4)], ids=["8x2", "32x4"])
def test_draws_do_not_depend_on_chunks_ranges_or_layout(shape):
    import torch

    N, K = shape
    B, T, S, seed = 8, 20, 8, 99
    d, obs = _batch(N, K, T, B, seed=N)
    results = {}
    for layout in ("model_major", "time_major"):
        kf = _engine(layout)
        kf.set_observations(obs).set_loadings(d["loadings"])
        for what in ("series", "states"):
            full = kf.draw_smoothed(d["phi"], d["q"], S, seed=seed, what=what)["draws"]
            one = kf.draw_smoothed(d["phi"], d["q"], S, seed=seed, what=what, chunk=1)["draws"]
            assert torch.equal(full, one), (layout, what, "chunk size 1 against all draws at once")
            three = kf.draw_smoothed(d["phi"], d["q"], S, seed=seed, what=what, chunk=3)["draws"]
            assert torch.equal(full, three), (layout, what, "chunk size 3")
            part = kf.draw_smoothed(d["phi"], d["q"], 3, seed=seed, what=what, first_draw=3)["draws"]
            assert torch.equal(part, full[3:6]), (layout, what, "draws 3..5 alone")
            results[(layout, what)] = full
        # records 4..7 as a batch of their own, numbered from 4: the same perturbed records and unconditional paths
        whole = [a.unflatten(0, (2, B)) for a in _perturb(kf, d, 2, seed, 0, 0, False, None)]
        sub = _engine(layout)
        sub.set_observations(obs[4:]).set_loadings(d["loadings"][4:])
        tail = [a.unflatten(0, (2, 4)) for a in _perturb(sub, {"phi": d["phi"][4:], "q": d["q"][4:]}, 2, seed, 4, 0, False, None)]
        for a, b in zip(whole, tail):
            assert torch.equal(torch.nan_to_num(a[:, 4:], nan=-7.0), torch.nan_to_num(b, nan=-7.0)), (layout, "first_instance = 4")
    for what in ("series", "states"):
        assert torch.equal(results[("model_major", what)], results[("time_major", what)]), (what, "model-major against time-major")


def _check_against_restatement(kf, d, obs, loadings, R, S, seed, what):
    out = kf.draw_smoothed(d["phi"], d["q"], S, seed=seed, what=what, chunk=2)     # S = 3: a tail chunk of another size
    assert int(out["status"].abs().sum().item()) == 0
    got = _np(out["draws"])
    for i in range(obs.shape[0]):
        want = draw_ref.draw_model(oracle, obs[i], d["phi"][i], d["q"][i], loadings[i], S, seed, i, what, None if R is None else R[i])
        assert np.abs(got[:, i] - want).max() <= TOL, (what, i)


@pytest.mark.parametrize("shape", [(8, 2), (32, 4)], ids=["8x2", "32x4"])
def test_an_engine_that_changes_between_calls(shape):
    """One engine, several calls: new loadings and observation variances of the same shape, another projection path, the other
    kernel family and new records between them -- every call draws from the engine as it stands then."""
    N, K = shape
    B, T, S, seed = 3, 24, 3, 555
    d, obs = _batch(N, K, T, B, seed=7 * N + K)
    kf = _engine("time_major")
    kf.set_observations(obs).set_loadings(d["loadings"])
    for what in ("series", "states"):
        _check_against_restatement(kf, d, obs, d["loadings"], None, S, seed, what)
    G2 = d["loadings"] * np.random.default_rng(1).uniform(0.3, 0.9, d["loadings"].shape)
    R2 = np.random.default_rng(2).uniform(0.05, 0.3, (B, N))
    kf.set_loadings(G2, R2)
    for what in ("series", "states"):
        _check_against_restatement(kf, d, obs, G2, R2, S, seed, what)
    kf.set_loadings(G2)
    kf.projection_path = "records"
    for what in ("series", "states"):
        _check_against_restatement(kf, d, obs, G2, None, S, seed, what)
    kf.projection_path = "auto"
    kf.set_variant("kernel_family", "generic")
    _check_against_restatement(kf, d, obs, G2, None, S, seed, "series")
    kf.set_variant("kernel_family", "specialised")
    obs2 = np.where(np.random.default_rng(3).random(obs.shape) < 0.5, np.nan, d["obs"])
    kf.set_observations(obs2).set_loadings(G2)
    for what in ("series", "states"):
        _check_against_restatement(kf, d, obs2, G2, None, S, seed, what)


def test_simulate_unconditional():
    N, K, B, T, S = 8, 2, 3, 16, 2
    d, obs = _batch(N, K, T, B, seed=1)
    R = np.random.default_rng(0).uniform(0.1, 0.3, (B, N))
    kf = _engine()
    kf.set_observations(obs).set_loadings(d["loadings"], R)
    held = kf.obs
    out = kf.simulate_unconditional(d["phi"], d["q"], S, seed=6)
    assert kf.obs is held
    z = draw_ref.normal_block(6, 0, B, 0, S, False, T, N + K + N)
    for s in range(S):
        for i in range(B):
            rx, rzx, ryp, _ = draw_ref.unconditional(obs[i], d["phi"][i], d["q"][i], d["loadings"][i], z[s, i], R[i])
            for key, ref in (("xplus", rx), ("zxplus", rzx), ("yplus", ryp)):
                assert np.abs(_np(out[key])[s, i] - ref).max() <= PERTURB_TOL, key


def test_metran_batch_end_to_end(g1):
    import pandas as pd

    from metran_amd.batch import MetranBatch

    idx = pd.DatetimeIndex(g1["index_ns"].astype("datetime64[ns]"))
    raw = g1["obs"] * g1["oseries_std"] + g1["oseries_mean"]
    series = [pd.Series(raw[:, j], index=idx, name="B21B021400%d" % (j + 1)).dropna() for j in range(raw.shape[1])]
    short = [s.iloc[: len(s) // 2] for s in series]
    mb = MetranBatch([series, short], factors=g1["loadings"])
    astar = np.stack([g1["alpha_star"], g1["alpha_star"] * 1.1])
    S = 2
    draws = _np(mb.get_simulation_draws(S, seed=3, alpha=astar))
    assert draws.shape == (S, 2, mb.T, mb.N)
    obs = _np(mb.kf.obs)
    seen = np.isfinite(obs)
    want = obs * _np(mb._std)[:, None] + _np(mb._mean)[:, None]
    for s in range(S):
        assert np.abs(draws[s][seen] - want[seen]).max() <= TOL * max(1.0, np.abs(want[seen]).max())
    gap = ~seen & (np.arange(mb.T)[None, :, None] < np.asarray(mb.batch.lengths)[:, None, None])
    assert np.abs(draws[0] - draws[1])[gap].max() > 1e-3
    # antithetic pairs average to get_simulated_means
    pair = _np(mb.get_simulation_draws(2, seed=3, alpha=astar, antithetic=True))
    means = _np(mb.get_simulated_means(astar))
    assert np.abs(0.5 * (pair[0] + pair[1]) - means).max() <= TOL * max(1.0, np.abs(means).max())
    frame = mb.get_simulation_draw(1, "B21B0214002", S, seed=3, alpha=astar)
    L = int(mb.batch.lengths[1])
    assert frame.shape == (L, S) and list(frame.columns) == ["draw0", "draw1"] and frame.index.equals(mb.batch.index[1])
    np.testing.assert_array_equal(frame.values, draws[:, 1, :L, 1].T)
    st = _np(mb.get_state_draws(S, seed=3, alpha=astar))
    assert st.shape == (S, 2, mb.T, mb.N + mb.K)
    Z = np.concatenate([np.broadcast_to(np.eye(mb.N), (2, mb.N, mb.N)), mb.factors], axis=2)
    proj = np.einsum("rjn,srtn->srtj", Z, st) * _np(mb._std)[None, :, None] + _np(mb._mean)[None, :, None]
    assert np.abs(proj - draws).max() <= TOL * max(1.0, np.abs(draws).max())


def test_refusals():
    import torch

    from metran_amd import _lib
    from metran_amd._lib import Problem

    L = _lib.lib()
    d, obs = _batch(8, 2, 16, 2, seed=3)
    kf = _engine()
    kf.set_observations(obs).set_loadings(d["loadings"])
    prob, keep, B = kf._problem(d["phi"], d["q"], 1, None, None)
    good = torch.empty((B, 16, 10), dtype=torch.float64, device="cuda")
    p = ctypes.c_void_p(good.data_ptr())
    # a missing required pointer
    assert L.mk_draw_perturb(kf._ctx, ctypes.byref(prob), 1, 0, 0, 1, 0, None, None, p, p) == -1 and b"d_ystar" in L.mk_last_error()
    assert L.mk_draw_combine(kf._ctx, ctypes.byref(prob), 1, 0, 0, None, p) == -1 and b"d_plus" in L.mk_last_error()
    assert L.mk_draw_normals(kf._ctx, 1, 0, 1, 0, 1, 0, 4, 10, 0, None) == -1 and b"d_out" in L.mk_last_error()
    noobs = Problem(*[getattr(prob, f[0]) for f in Problem._fields_])
    noobs.d_obs = None
    assert L.mk_draw_perturb(kf._ctx, ctypes.byref(noobs), 1, 0, 0, 1, 0, None, p, None, None) == -1 and b"d_obs" in L.mk_last_error()
    # a buffer smaller than the call needs (an allocation of its own: its size is known exactly)
    small = ctypes.c_void_p()
    assert L.mk_malloc(kf._ctx, 128, ctypes.byref(small)) == 0
    try:
        assert L.mk_draw_perturb(kf._ctx, ctypes.byref(prob), 1, 0, 0, 1, 0, None, small, None, None) == -1
        assert b"d_ystar" in L.mk_last_error()
        assert L.mk_draw_perturb(kf._ctx, ctypes.byref(prob), 1, 0, 0, 1, 0, None, p, None, small) == -1
        assert b"d_xplus" in L.mk_last_error()
        assert L.mk_draw_combine(kf._ctx, ctypes.byref(prob), 1, 1, 0, p, small) == -1 and b"d_inout" in L.mk_last_error()
        assert L.mk_draw_normals(kf._ctx, 1, 0, 1, 0, 1, 0, 4, 10, 0, small) == -1 and b"d_out" in L.mk_last_error()
    finally:
        L.mk_free(kf._ctx, small)
    # more states than the library serves
    big = Problem(1, 1, 4, 120, 9, 0, p, p, p, p, None, None, None, 0, None, None)
    assert L.mk_draw_perturb(kf._ctx, ctypes.byref(big), 1, 0, 0, 1, 0, None, p, None, None) == -2 and b"N=120, K=9" in L.mk_last_error()
    assert L.mk_draw_perturb(kf._ctx, ctypes.byref(prob), 1, 0, 0, 0, 0, None, p, None, None) == -1 and b"ndraws" in L.mk_last_error()
    with pytest.raises(ValueError):
        kf.draw_smoothed(d["phi"], d["q"], 2, what="nope")

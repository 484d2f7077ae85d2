"""GPU: the record smoother with the forward substitution folded into the pivot chain (Sweeps<n>::factor_forward, DESIGN.md
section 4) against the oracle's C port, at the tolerances of tests/test_hip_parity.py (smoothed moments 1e-9 absolute) and
tests/test_hip_singular.py (1e-9 where the reference is well defined) for the same outputs.

* chain boundaries: n = 2 (one fused stage, no trailing update) .. n = 10 (two K), and n = 11 -- the tiled, untouched path;
* time and batch boundaries: T = 1, 2, 3, 5, 40 x B = 1, 5, 17 (partial groups, a partial workgroup), both layouts, both
  record forms, the three routes through the kernel (records, + projection, + state variances);
* the cold path made deterministic: a model with q_r = 0 and row / column r of P0 zero has row r of every covariance, and so
  pivot r of every step, exactly 0.0 -- its whole wavefront re-factorises at every step and must restore the right-hand
  sides the fused sweep has overwritten."""
import numpy as np
import pytest

import oracle
from metran_amd.params import observation_matrix
from metran_amd.synthetic import make_dfm_batch

pytestmark = pytest.mark.gpu

SMOOTH_ATOL = 1e-9
_ENGINES, _REFS = {}, {}


def _np(t):
    return t.detach().cpu().numpy()


def _like(got, full):
    """The oracle's covariances in the form the engine hands out: whole, or the upper triangle by rows (packed-symmetric)."""
    if got.dim() == full.ndim:
        return full
    iu = np.triu_indices(full.shape[-1])
    return full[..., iu[0], iu[1]]


def _engine(layout, sym):
    from metran_amd.engine import BatchedKalman

    if (layout, sym) not in _ENGINES:
        _ENGINES[layout, sym] = BatchedKalman(0, layout=layout, packed_sym=sym)
    return _ENGINES[layout, sym]


def _case(N, K, T, B):
    """Seeded inputs and the oracle's smoothed moments, computed once per (N, K, T, B)."""
    if (N, K, T, B) not in _REFS:
        d = make_dfm_batch(B, N, K, T, seed=700 + 10 * N + K, missing=0.2 if T > 1 else 0.0, first_step="random")
        ref = oracle.dfm_batch(d["obs"], d["phi"], d["q"], d["loadings"])
        assert np.isfinite(ref["S"]).all() and np.isfinite(ref["Ps"]).all()
        for a in list(d.values()) + [ref["S"], ref["Ps"]]:
            a.setflags(write=False)
        _REFS[N, K, T, B] = d, ref
    return _REFS[N, K, T, B]


def _check_three_routes(kf, d, S, Ps, P0=None, rows=slice(None)):
    B, N = d["obs"].shape[0], d["obs"].shape[2]
    kf.set_observations(d["obs"]).set_loadings(d["loadings"])
    r = kf.filter_smooth(d["phi"], d["q"], P0=P0)
    np.testing.assert_allclose(_np(r["S"])[rows], S[rows], rtol=0, atol=SMOOTH_ATOL, err_msg="S")
    np.testing.assert_allclose(_np(r["Ps"])[rows], _like(r["Ps"], Ps)[rows], rtol=0, atol=SMOOTH_ATOL, err_msg="Ps")
    Z = np.concatenate([np.broadcast_to(np.eye(N), (B, N, N)), d["loadings"]], axis=2)
    p = kf.simulate_smoothed(d["phi"], d["q"], P0=P0)
    assert not p.get("_tape")
    np.testing.assert_allclose(_np(p["sim_means"])[rows], np.einsum("bjn,btn->btj", Z, S)[rows], rtol=0, atol=SMOOTH_ATOL, err_msg="sim_means")
    np.testing.assert_allclose(_np(p["sim_vars"])[rows], np.maximum(np.einsum("bjn,btnm,bjm->btj", Z, Ps, Z), 0.0)[rows], rtol=0,
                               atol=SMOOTH_ATOL, err_msg="sim_vars")
    v = kf.smooth_state_variances(d["phi"], d["q"], P0=P0)
    assert not v.get("_tape")
    np.testing.assert_allclose(_np(v["S"])[rows], S[rows], rtol=0, atol=SMOOTH_ATOL, err_msg="state means")
    np.testing.assert_allclose(_np(v["var"])[rows], np.diagonal(Ps, axis1=2, axis2=3)[rows], rtol=0, atol=SMOOTH_ATOL, err_msg="state variances")
    return r, p, v


@pytest.mark.parametrize("sym", [False, True], ids=["square", "packed"])
@pytest.mark.parametrize("layout", ["model_major", "time_major"])
@pytest.mark.parametrize("N,K", [(1, 1), (2, 1), (4, 3), (8, 2), (7, 3), (9, 2)])
def test_chain_boundaries(N, K, layout, sym):
    d, ref = _case(N, K, 40, 5)
    r, p, v = _check_three_routes(_engine(layout, sym), d, ref["S"], ref["Ps"])
    assert not _np(r["status"]).any() and not _np(p["status"]).any() and not _np(v["status"]).any()


@pytest.mark.parametrize("B", [1, 5, 17])
@pytest.mark.parametrize("T", [1, 2, 3, 5, 40])
def test_time_and_batch_boundaries(T, B):
    d, ref = _case(8, 2, T, B)
    for layout in ("model_major", "time_major"):
        for sym in (False, True):
            r, p, v = _check_three_routes(_engine(layout, sym), d, ref["S"], ref["Ps"])
            assert not _np(r["status"]).any() and not _np(p["status"]).any() and not _np(v["status"]).any()


def _singular_reference(d, P0):
    """The oracle's filter and smoother model by model with the given initial covariance (its batch entry starts from I)."""
    B, T, N = d["obs"].shape
    n = d["phi"].shape[1]
    S, Ps = np.empty((B, T, n)), np.empty((B, T, n, n))
    for b in range(B):
        o, oi, oc = oracle.set_observations(d["obs"][b])
        Phi, Q, Z = np.diag(d["phi"][b]), np.diag(d["q"][b]), observation_matrix(d["loadings"][b])
        f = oracle.seqkalmanfilter(o, Phi, Q, Z, np.zeros(N), oi, oc, np.zeros(n), P0[b])
        S[b], Ps[b] = oracle.kalmansmoother(f[3], f[4], f[5], f[6], Phi)
    return S, Ps


def _singular_case(N, K, r, where):
    """Six regular models and one whose state r is identically zero: first, last, or alone in its wavefront of four (B = 9:
    models 8 .. 11 of the last wavefront are replicas of model 8)."""
    key = ("sing", N, K, r, where)
    if key not in _REFS:
        B = {"first": 7, "last": 7, "alone": 9}[where]
        at = {"first": 0, "last": 3, "alone": 8}[where]
        d = make_dfm_batch(B, N, K, 40, seed=900 + 10 * N + K, missing=0.0, first_step="observed")
        d = {k: a.copy() for k, a in d.items()}
        P0 = np.tile(np.eye(N + K), (B, 1, 1))
        d["q"][at, r] = 0.0
        P0[at, r, :] = 0.0
        P0[at, :, r] = 0.0
        S, Ps = _singular_reference(d, P0)
        assert np.isfinite(S).all() and np.isfinite(Ps).all()       # checked on the CPU before anything goes to the GPU
        assert not Ps[at, :, r, :].any() and not Ps[at, :, :, r].any()
        _REFS[key] = d, P0, S, Ps, at
    return _REFS[key]


@pytest.mark.parametrize("where", ["first", "last", "alone"])
@pytest.mark.parametrize("N,K,r", [(8, 2, 0), (8, 2, 4), (8, 2, 7), (2, 1, 0), (2, 1, 1)])
def test_cold_path_restores_the_right_hand_sides(N, K, r, where):
    from metran_amd.engine import FLAG_RANK_DEFICIENT

    d, P0, S, Ps, at = _singular_case(N, K, r, where)
    B = d["obs"].shape[0]
    others = np.array([b for b in range(B) if b != at])
    for layout in ("model_major", "time_major"):
        for sym in (False, True):
            kf = _engine(layout, sym)
            outs = _check_three_routes(kf, d, S, Ps, P0=P0)
            for res in outs:     # the redo was taken by that model, and by no other
                st = _np(res["status"])
                assert st[at] == FLAG_RANK_DEFICIENT, (layout, sym, st)
                assert not st[others].any(), (layout, sym, st)
            # the regular models next to it: bit-equal to a run without the singular neighbour
            sub = {k: np.ascontiguousarray(a[others]) for k, a in d.items()}
            kf.set_observations(sub["obs"]).set_loadings(sub["loadings"])
            alone = kf.filter_smooth(sub["phi"], sub["q"], P0=np.ascontiguousarray(P0[others]))
            assert not _np(alone["status"]).any()
            np.testing.assert_array_equal(_np(outs[0]["S"])[others], _np(alone["S"]))
            np.testing.assert_array_equal(_np(outs[0]["Ps"])[others], _np(alone["Ps"]))
            pa = kf.simulate_smoothed(sub["phi"], sub["q"], P0=np.ascontiguousarray(P0[others]))
            np.testing.assert_array_equal(_np(outs[1]["sim_means"])[others], _np(pa["sim_means"]))
            np.testing.assert_array_equal(_np(outs[1]["sim_vars"])[others], _np(pa["sim_vars"]))
            va = kf.smooth_state_variances(sub["phi"], sub["q"], P0=np.ascontiguousarray(P0[others]))
            np.testing.assert_array_equal(_np(outs[2]["S"])[others], _np(va["S"]))
            np.testing.assert_array_equal(_np(outs[2]["var"])[others], _np(va["var"]))

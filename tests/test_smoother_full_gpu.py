"""GPU: the launch-uniform FULL form of the record smoother's rank-K covariance step (smoother_record_kernel LR + FULL, DESIGN.md
section 4) -- taken when the count that ``full_records_kernel`` makes once per observation set finds EVERY step of EVERY record
full, for n <= 10, full-square records and no observation variances.  The form looks at no observation and carries no flag.

Shapes (1,1), (4,1), (8,2), (7,3), and (12,2) where the form does not exist; T = 1 (no loop iteration), 2 (one), 3 (the first
one with a prefetch behind it), 17 (a steady loop); B = 1, 4 (a full wavefront), 5 (a partial one) and 6 instances on 2 records
(B > R); both layouts; no gaps.  Every case:

(a) ``S`` and ``Ps`` against the oracle at 1e-9;
(b) bit-equal to the per-model path: the same models with one more model appended whose record has a missing cell ("all" is false
    for that launch: the neighbours take the rank-K step per model, under the flag) and without it ("all" is true);
(c) the two epilogue routes (``simulate_smoothed``, ``smooth_state_variances``), which have no rank-K step, equal the general-only
    variant (``set_variant("smoother16", "record_general")``) bit for bit.

There is no kernel-name hook in the engine, so "the form ran" is the criterion of tests/test_smoother_lowrank_gpu.py: ``Ps`` differs
from the general-only variant's in the last bits and ``S`` does not.  The counting rule of ``full_records_kernel`` (every record,
every step) is a device kernel without a host twin in ``tests/``: it is covered here through (b) and the invalidation test."""
import numpy as np
import pytest

import hard_models as hm
import oracle
from metran_amd.params import observation_matrix
from metran_amd.synthetic import make_dfm_batch

pytestmark = pytest.mark.gpu

SMOOTH_ATOL = 1e-9
SHAPES = [(1, 1), (4, 1), (8, 2), (7, 3), (12, 2)]
BATCHES = [(1, 1), (4, 4), (5, 5), (6, 2)]   # (instances B, records R): instance b reads record b % R
_ENGINES, _CASES = {}, {}


def _np(t):
    return t.detach().cpu().numpy()


def _engine(layout, variant):
    from metran_amd.engine import BatchedKalman

    key = (layout, variant)
    if key not in _ENGINES:
        # "stepwise": one record alone goes through the batched filter_kernel too, as it does with a second record beside it
        _ENGINES[key] = BatchedKalman(0, layout=layout).set_variant("smoother16", variant).set_variant("single_record", "stepwise")
    return _ENGINES[key]


def _case(N, K, T, B, R):
    """Seeded inputs without gaps (records 0..R-1, parameter sets 0..B-1), one more record WITH a missing cell and its parameter
    sets, and the oracle's moments of the B instances (computed once)."""
    key = (N, K, T, B, R)
    if key not in _CASES:
        reps = B // R
        d = make_dfm_batch(B + reps, N, K, T, seed=6100 + 100 * N + 10 * K + T, missing=0.0)
        obs, load = d["obs"][:R + 1].copy(), d["loadings"][:R + 1].copy()
        obs[R, T // 2, N - 1] = np.nan          # the appended record: one cell missing
        rec = np.arange(B) % R
        ref = oracle.dfm_batch(obs[rec], d["phi"][:B], d["q"][:B], load[rec])
        assert np.isfinite(ref["S"]).all() and np.isfinite(ref["Ps"]).all()
        Z = np.concatenate([np.broadcast_to(np.eye(N), (B, N, N)), load[rec]], axis=2)
        want = {"S": ref["S"], "Ps": ref["Ps"], "sim_means": np.einsum("bjn,btn->btj", Z, ref["S"]),
                "sim_vars": np.maximum(np.einsum("bjn,btnm,bjm->btj", Z, ref["Ps"], Z), 0.0), "var": np.diagonal(ref["Ps"], axis1=2, axis2=3)}
        bars = np.array([hm.smoother_tolerance({"obs": obs[rec], "phi": d["phi"][:B], "q": d["q"][:B], "loadings": load[rec]}, b,
                                               {"Pp": ref["Pp"][b], "F": ref["F"][b]}) for b in range(B)])
        case = {"obs": obs, "loadings": load, "phi": d["phi"], "q": d["q"], "want": want, "bars": bars}
        for a in list(case.values()) + list(want.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CASES[key] = case
    return _CASES[key]


ROUTES = (("filter_smooth", ("S", "Ps")), ("simulate_smoothed", ("sim_means", "sim_vars")), ("smooth_state_variances", ("S", "var")))


def _run(kf, c, route, B, R, appended):
    """The B instances on records 0..R-1 -- alone ("all" holds), or with the gapped record R and its B / R instances appended,
    instance i = j (R + 1) + r reading record r.  Returns the outputs of the B shared instances, in the order of the run alone."""
    reps = B // R
    if appended:
        Ra = R + 1
        par = np.array([j * R + r if r < R else B + j for j in range(reps) for r in range(Ra)])
        shared = np.array([j * Ra + r for j in range(reps) for r in range(R)])
    else:
        Ra, par, shared = R, np.arange(B), np.arange(B)
    kf.set_observations(np.ascontiguousarray(c["obs"][:Ra])).set_loadings(np.ascontiguousarray(c["loadings"][:Ra]))
    r = getattr(kf, route)(np.ascontiguousarray(c["phi"][par]), np.ascontiguousarray(c["q"][par]))
    assert not r.get("_tape")
    assert not _np(r["status"]).any(), route
    return {k: _np(r[k])[shared] for k in dict(ROUTES)[route]}


@pytest.mark.parametrize("T", [1, 2, 3, 17])
@pytest.mark.parametrize("N,K", SHAPES)
def test_full_form(N, K, T):
    for B, R in BATCHES:
        c = _case(N, K, T, B, R)
        for layout in ("model_major", "time_major"):
            kf, kg = _engine(layout, "record"), _engine(layout, "record_general")
            what = (N, K, T, B, R, layout)
            for route, keys in ROUTES:
                got = _run(kf, c, route, B, R, appended=False)
                for k in keys:
                    np.testing.assert_allclose(got[k], c["want"][k], rtol=0, atol=SMOOTH_ATOL, err_msg="(a) %s %s %s" % (route, k, what))
                if route == "filter_smooth":
                    per_model = _run(kf, c, route, B, R, appended=True)
                    for k in keys:
                        np.testing.assert_array_equal(got[k], per_model[k], err_msg="(b) %s %s %s" % (route, k, what))
                if route != "filter_smooth" or N + K > 10:
                    gen = _run(kg, c, route, B, R, appended=False)
                    for k in keys:
                        np.testing.assert_array_equal(got[k], gen[k], err_msg="(c) %s %s %s" % (route, k, what))


@pytest.mark.parametrize("layout", ["model_major", "time_major"])
@pytest.mark.parametrize("N,K", [(8, 2), (4, 1)])
def test_the_rank_k_products_are_what_ran(N, K, layout):
    """With every step of every record full the default takes the rank-K products at every step: the two forms sum in another
    order, so Ps differs from the general-only variant's in the last bits -- and S, which the step does not touch, does not."""
    c = _case(N, K, 17, 4, 4)
    got = _run(_engine(layout, "record"), c, "filter_smooth", 4, 4, appended=False)
    gen = _run(_engine(layout, "record_general"), c, "filter_smooth", 4, 4, appended=False)
    diff = np.abs(got["Ps"] - gen["Ps"]).reshape(4, -1).max(axis=1)
    assert (diff > 0.0).all(), diff
    assert (diff <= c["bars"]).all(), (diff, c["bars"])
    np.testing.assert_array_equal(got["Ps"][:, -1], gen["Ps"][:, -1])
    np.testing.assert_array_equal(got["S"], gen["S"])


@pytest.mark.parametrize("layout", ["model_major", "time_major"])
def test_a_changed_cell_invalidates_the_answer(layout):
    """The answer "all" is kept per observation set: the same engine, given the same tensor with one cell overwritten by NaN
    (``set_observations`` calls ``mk_observations_changed``), returns what a fresh engine returns, and the first result again, bit
    for bit, once the cell is restored."""
    import torch
    from metran_amd.engine import BatchedKalman

    N, K, T, B = 8, 2, 17, 4
    c = _case(N, K, T, B, B)
    kf = BatchedKalman(0, layout=layout)
    obs = torch.from_numpy(c["obs"][:B].copy()).to(kf.device)
    load, phi, q = (np.ascontiguousarray(c[k][:B]) for k in ("loadings", "phi", "q"))

    def run(engine):
        r = engine.set_observations(obs).set_loadings(load).filter_smooth(phi, q)
        assert not _np(r["status"]).any()
        return _np(r["S"]), _np(r["Ps"])

    first = run(kf)
    np.testing.assert_allclose(first[0], c["want"]["S"], rtol=0, atol=SMOOTH_ATOL)
    np.testing.assert_allclose(first[1], c["want"]["Ps"], rtol=0, atol=SMOOTH_ATOL)
    kept = obs[2, 5, 3].item()
    obs[2, 5, 3] = float("nan")
    gapped, fresh = run(kf), run(BatchedKalman(0, layout=layout))
    np.testing.assert_array_equal(gapped[0], fresh[0])
    np.testing.assert_array_equal(gapped[1], fresh[1])
    assert np.abs(gapped[1][2] - first[1][2]).max() > 1e-6   # the cell is gone from model 2's result ...
    np.testing.assert_array_equal(gapped[1][[0, 1, 3]], first[1][[0, 1, 3]])   # ... and from nobody else's
    obs[2, 5, 3] = kept
    again = run(kf)
    np.testing.assert_array_equal(again[0], first[0])
    np.testing.assert_array_equal(again[1], first[1])


def _singular_reference(d, P0):
    B, T, N = d["obs"].shape
    n = d["phi"].shape[1]
    S, Ps = np.empty((B, T, n)), np.empty((B, T, n, n))
    for b in range(B):
        o, oi, oc = oracle.set_observations(d["obs"][b])
        Phi, Q, Z = np.diag(d["phi"][b]), np.diag(d["q"][b]), observation_matrix(d["loadings"][b])
        f = oracle.seqkalmanfilter(o, Phi, Q, Z, np.zeros(N), oi, oc, np.zeros(n), P0[b])
        S[b], Ps[b] = oracle.kalmansmoother(f[3], f[4], f[5], f[6], Phi)
    return S, Ps


@pytest.mark.parametrize("N,K,r", [(8, 2, 4), (4, 1, 0)])
def test_cold_path_model_in_an_all_full_batch(N, K, r):
    """The q_r = 0 model of test_smoother_lowrank_gpu.py::test_cold_path_model_among_full_steps (pivot r of every step is exactly
    0.0: its wavefront re-factorises at every step, then runs the rank-K products) inside a batch without a gap: the rank flag is
    set on that model only and the neighbours are bit-equal to themselves run without it."""
    from metran_amd.engine import FLAG_RANK_DEFICIENT

    B, at = 7, 2
    d = {k: a.copy() for k, a in make_dfm_batch(B, N, K, 17, seed=5900 + N, missing=0.0).items()}
    P0 = np.tile(np.eye(N + K), (B, 1, 1))
    d["q"][at, r] = 0.0
    P0[at, r, :] = 0.0
    P0[at, :, r] = 0.0
    S, Ps = _singular_reference(d, P0)
    assert np.isfinite(S).all() and np.isfinite(Ps).all()
    others = np.array([b for b in range(B) if b != at])
    for layout in ("model_major", "time_major"):
        kf = _engine(layout, "record")
        kf.set_observations(d["obs"]).set_loadings(d["loadings"])
        res = kf.filter_smooth(d["phi"], d["q"], P0=P0)
        st = _np(res["status"])
        assert st[at] == FLAG_RANK_DEFICIENT and not st[others].any(), (layout, st)
        np.testing.assert_allclose(_np(res["S"]), S, rtol=0, atol=SMOOTH_ATOL)
        np.testing.assert_allclose(_np(res["Ps"]), Ps, rtol=0, atol=SMOOTH_ATOL)
        got_S, got_Ps = _np(res["S"])[others], _np(res["Ps"])[others]
        sub = {k: np.ascontiguousarray(a[others]) for k, a in d.items()}
        kf.set_observations(sub["obs"]).set_loadings(sub["loadings"])
        alone = kf.filter_smooth(sub["phi"], sub["q"], P0=np.ascontiguousarray(P0[others]))
        assert not _np(alone["status"]).any()
        np.testing.assert_array_equal(got_S, _np(alone["S"]))
        np.testing.assert_array_equal(got_Ps, _np(alone["Ps"]))

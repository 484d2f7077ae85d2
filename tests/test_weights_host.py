"""The numpy restatement of the observation weights (tests/weights_ref.py), pinned WITHOUT a GPU: to dense Gaussian conditioning,
to the oracle's own smoother and projection by linearity (unit impulses), to a fixture of the same impulses through the
reference's own filter, smoother and ``simulate`` (tests/golden/weights_ref_impulses.npz, made by
tests/golden/make_weights_golden.py); its deliberately wrong variants shown to be far outside the bar; the MetranBatch
accessors over a stand-in engine that answers from the restatement; and the binding of the two new entry points."""
import os
import re

import numpy as np
import pytest

import weights_ref
from conftest import ROOT, load_golden
from weights_engine import WeightsEngine, oracle_simulation

F64 = np.float64
DENSE_BAR = 1e-10    # absolute, against one dense solve
PARITY_BAR = 1e-9    # the project's parity bar against the oracle / the reference


def _model(N, K, T, seed, full):
    """(y, phi, q, G, R, x0, P0): 30 % missing, one empty step, ``full``: observation variances and initial moments given."""
    rng = np.random.default_rng(seed)
    n = N + K
    y = rng.normal(size=(T, N))
    y[rng.random((T, N)) < 0.3] = np.nan
    y[4] = np.nan
    y[0, 0], y[T - 1, N - 1] = 0.4, -0.7
    phi, q = rng.uniform(0.5, 0.95, n), rng.uniform(0.1, 0.5, n)
    G = rng.uniform(-0.6, 0.6, (N, K))
    A = rng.normal(size=(n, n))
    return (y, phi, q, G, rng.uniform(0.05, 0.4, N) if full else None, rng.normal(size=n) if full else None,
            A @ A.T / n + 0.5 * np.eye(n) if full else None)


CASES = [(3, 1, 12, 1, False), (3, 1, 12, 2, True), (4, 2, 9, 3, False), (4, 2, 9, 4, True)]


def _targets(y, states):
    T, N = y.shape
    seen = np.isfinite(y)
    t_obs = int(np.nonzero(seen[5:, 1])[0][0]) + 5
    t_mis = int(np.nonzero(~seen[5:, 0] & seen[5:].any(1))[0][0]) + 5 if (~seen[5:, 0] & seen[5:].any(1)).any() else 5
    return [(t_obs, 1), (t_mis, 0), (4, N - 1 if not states else N), (0, 0), (T - 1, N - 1)]


@pytest.mark.parametrize("case", CASES, ids=["%dx%d-T%d-%s" % (c[0], c[1], c[2], "full" if c[4] else "plain") for c in CASES])
@pytest.mark.parametrize("what", ["series", "states"])
def test_restatement_is_dense_gaussian_conditioning(case, what):
    """An observed cell, a missing cell of a partly observed step, a cell of the empty step (states: a common factor there),
    t* = 0 and t* = T - 1: the walks give what one dense solve on the joint covariance of states and data gives."""
    N, K, T, seed, full = case
    m = _model(N, K, T, seed, full)
    tg = _targets(m[0], what == "states")
    wd, icd = weights_ref.dense(*m, targets=tg, what=what)
    for dtype in (F64, np.longdouble):
        w, ic = weights_ref.weights(*m, targets=tg, what=what, dtype=dtype)
        assert np.array_equal(np.isnan(w), np.isnan(wd)) and np.array_equal(np.isnan(w[0]), ~np.isfinite(m[0]))
        assert np.nanmax(np.abs(w.astype(F64) - wd)) <= DENSE_BAR and np.max(np.abs(ic.astype(F64) - icd)) <= DENSE_BAR
    if not full:
        assert (icd == 0).all()


@pytest.mark.parametrize("case", CASES, ids=["%dx%d-T%d-%s" % (c[0], c[1], c[2], "full" if c[4] else "plain") for c in CASES])
def test_restatement_is_the_oracles_smoother_by_linearity(case):
    """w[s, i] = sim(y + e_{s,i})[t*, j*] - sim(y)[t*, j*] for every observed cell through the oracle's filter, smoother and
    projection, and sum w y + intercept = sim(y)[t*, j*]."""
    N, K, T, seed, full = case
    y, phi, q, G, R, x0, P0 = _model(N, K, T, seed, full)
    tg = _targets(y, False)
    w, ic = weights_ref.weights(y, phi, q, G, R, x0, P0, tg, dtype=F64)
    base, _ = oracle_simulation(y, phi, q, G, R, x0, P0)
    for s, i in zip(*np.nonzero(np.isfinite(y))):
        bumped = y.copy()
        bumped[s, i] += 1.0
        sim, _ = oracle_simulation(bumped, phi, q, G, R, x0, P0)
        for mth, (ts, col) in enumerate(tg):
            assert abs(w[mth, s, i] - (sim[ts, col] - base[ts, col])) <= PARITY_BAR, (mth, s, i)
    for mth, (ts, col) in enumerate(tg):
        assert abs(np.nansum(w[mth] * y) + ic[mth] - base[ts, col]) <= PARITY_BAR


def test_restatement_matches_the_references_impulses():
    g = load_golden("weights_ref_impulses.npz")
    y = g["obs"]
    assert y.shape == (40, 3) and np.isnan(y[17]).all() and abs(np.isnan(y).mean() - 0.3) < 0.1
    (t0, c0), (t1, c1), (t2, c2) = g["targets"]
    assert np.isfinite(y[t0, c0]) and t1 == 17 and t2 == 0      # an observed cell, a cell of the empty step, t* = 0
    for dtype in (F64, np.longdouble):
        w, ic = weights_ref.weights(y, g["phi"], g["q"], g["loadings"], targets=g["targets"], dtype=dtype)
        assert np.array_equal(np.isnan(w), np.isnan(g["weights"]))
        assert np.nanmax(np.abs(w.astype(F64) - g["weights"])) <= PARITY_BAR
        assert (ic == 0).all()
        for mth in range(3):
            assert abs(float(np.nansum(w[mth] * y)) - g["base"][mth]) <= PARITY_BAR


@pytest.mark.parametrize("bad", ["stop_at_target", "no_c", "descending", "records"])
def test_wrong_variants_are_far_outside_the_bar(bad):
    """Filter weights (the walk stops at t*), the missing + c at t*, the series of a step in the wrong order, and targets
    mapped to the wrong record: each misses the reference by more than a million bars."""
    g = load_golden("weights_ref_impulses.npz")
    y, phi, q, G = g["obs"], g["phi"], g["q"], g["loadings"]
    if bad != "records":
        w, _ = weights_ref.weights(y, phi, q, G, targets=g["targets"], dtype=F64, **{bad: True})
        miss = [np.nanmax(np.abs(w[mth] - g["weights"][mth])) for mth in range(3)]
        if bad == "stop_at_target":
            assert (np.nan_to_num(w[:, 22:]) == 0).all()       # nothing after the latest target: the filter's weights
        assert max(miss) > 1e6 * PARITY_BAR, miss
        return
    # two records with the fixture's targets on record 0 and others on record 1: an engine that looks the targets up by the
    # wrong record returns a full, plausible answer that is far off
    y2 = np.stack([y, np.roll(y, 3, axis=0)])
    tg = np.stack([g["targets"], np.array([[30, 0], [5, 1], [39, 2]])])
    eng = WeightsEngine(y2, np.stack([G, G]))
    ph, qq = np.stack([phi, phi]), np.stack([q, q])
    good = eng.observation_weights(ph, qq, tg)["weights"].numpy()
    assert np.nanmax(np.abs(good[0] - g["weights"])) <= PARITY_BAR
    eng.shift_records = 1
    wrong = eng.observation_weights(ph, qq, tg)["weights"].numpy()
    assert np.nanmax(np.abs(wrong[0] - g["weights"])) > 1e6 * PARITY_BAR


def test_the_gpu_tiers_per_record_target_lists_tell_the_records_apart():
    """tests/test_weights_gpu.py::test_every_record_has_its_own_target_list relies on this: on its inputs the restatement with
    an instance's own list is more than 2000 bars from the restatement with the other record's list, target by target -- so a
    kernel within one bar of the first is more than 1000 bars from the second."""
    import test_weights_gpu as tw

    for N, K in tw.PER_RECORD_SHAPES:
        p, tgs = tw._per_record_case(N, K)
        for what, tg in tgs.items():
            assert tg.shape[0] == tw.R_ and all(tuple(a) != tuple(b) for a, b in zip(tg[0], tg[1]))
            for b in range(tw.B_):
                (w, ic), gain = tw._reference(p, b, tg, what, dtype=F64)
                (wo, io), _ = tw._reference(p, b, tg[::-1], what, gain, dtype=F64)
                for m in range(tg.shape[1]):
                    assert np.nanmax(np.abs(w[m] - wo[m])) > 2000 * tw.BAR * max(1.0, np.nanmax(np.abs(w[m]))), (N, K, what, b, m)


def test_unused_and_out_of_range_targets_are_nan():
    y, phi, q, G, R, x0, P0 = _model(3, 1, 12, 5, True)
    for what, cols in (("series", 3), ("states", 4)):
        w, ic = weights_ref.weights(y, phi, q, G, R, x0, P0, [(-1, 0), (12, 0), (3, cols), (3, -1), (3, cols - 1)], what, dtype=F64)
        assert np.isnan(w[:4]).all() and np.isnan(ic[:4]).all() and np.isfinite(ic[4]) and np.isfinite(w[4][np.isfinite(y)]).all()


# ---- MetranBatch over a stand-in engine ----
def _shortest_window(aw, tstar, mass):
    """Brute force: the shortest [a, b] with a <= tstar <= b holding ``mass`` of sum(aw), the earliest among equals."""
    tot, best = aw.sum(), None
    for a in range(tstar + 1):
        for b in range(tstar, len(aw)):
            if aw[a:b + 1].sum() >= mass * tot * (1 - 1e-12) and (best is None or b - a < best[1] - best[0]):
                best = (a, b)
                break
    return best


def test_metran_batch_accessors_over_a_stand_in_engine():
    """The engine answers ``observation_weights`` from weights_ref and ``simulate_smoothed`` from the oracle
    (tests/weights_engine.py)."""
    import pandas as pd

    from batch_standin import stand_in, two_models
    from metran_amd.params import phi_q_from_alpha

    models, G = two_models()
    mb = stand_in(WeightsEngine, models, G)
    alpha = np.array([[8.0, 6.0, 9.0, 12.0], [5.0, 7.0, 8.0, 10.0]])
    phi, q = phi_q_from_alpha(alpha, G, 1.0)
    L = [int(v) for v in mb.batch.lengths]
    std, mean, yst = mb._std.numpy(), mb._mean.numpy(), mb.kf.obs_np
    r, name, j = 1, "s2", 2
    index = mb.batch.index[r]
    gap = int(np.nonzero(~np.isfinite(yst[r, 5:L[r], j]))[0][0]) + 5       # a gap-filled value
    gap2 = int(np.nonzero(~np.isfinite(yst[r, gap + 6:L[r], j]))[0][0]) + gap + 6
    times = [index[gap], index[0], L[r] - 1, index[gap2]]           # time stamps and integer steps alike
    steps = [gap, 0, L[r] - 1, gap2]
    ref_w, ref_ic = weights_ref.weights(yst[r], phi[r], q[r], G[r], targets=[(s, j) for s in steps], dtype=F64)

    st = mb.get_observation_weights(r, name, times, alpha=alpha, standardized=True)
    assert mb.kf.calls == 1 and list(st) == [index[s] for s in steps]
    orig = mb.get_observation_weights(r, name, times, alpha=alpha)
    assert mb.kf.calls == 1                                        # same parameter set and request: one engine call
    sim = mb.get_simulation(r, name, alpha=alpha, ci=None)
    sim_st = mb.get_simulation(r, name, alpha=alpha, ci=None, standardized=True)
    yor = yst[r] * std[r] + mean[r]
    for mth, s in enumerate(steps):
        fs, fo = st[index[s]], orig[index[s]]
        assert fs.shape == (L[r], 3) and fs.index.equals(index) and list(fs.columns) == ["s0", "s1", "s2"]
        np.testing.assert_array_equal(fs.values, ref_w[mth, :L[r]])
        assert fs.attrs["intercept"] == ref_ic[mth] == 0.0
        assert np.array_equal(np.isnan(fs.values), ~np.isfinite(yst[r, :L[r]]))
        # unit conversion: w std_name / std_i
        np.testing.assert_allclose(fo.values, ref_w[mth, :L[r]] * std[r, j] / std[r][None, :], rtol=1e-14, atol=0)
        # the reconstruction identity against get_simulation, in both units
        assert abs(np.nansum(fs.values * yst[r, :L[r]]) + fs.attrs["intercept"] - sim_st.iloc[s]) <= PARITY_BAR
        got = np.nansum(fo.values * (yor[:L[r]] - mean[r])) + mean[r, j] + fo.attrs["intercept"]
        assert abs(got - sim.iloc[s]) <= PARITY_BAR * max(1.0, abs(sim.iloc[s]))
    assert not np.isfinite(yst[r, gap, j]) and np.isnan(st[index[gap]].iloc[gap, j])   # a gap-fill has no own weight

    # a state, in the filter's units: the common factor
    sw = mb.get_state_weights(r, 3, [index[gap]], alpha=alpha)[index[gap]]
    wst, ics = weights_ref.weights(yst[r], phi[r], q[r], G[r], targets=[(gap, 3)], what="states", dtype=F64)
    np.testing.assert_array_equal(sw.values, wst[0, :L[r]])
    assert mb.kf.calls == 2
    with pytest.raises(IndexError):
        mb.get_state_weights(r, 4, [0], alpha=alpha)

    # shares: one row per (time, source series), summing to 1 per time; the 90 % window against brute force
    sh = mb.get_weight_shares(r, name, times, alpha=alpha)
    assert mb.kf.calls == 2 and list(sh.index.names) == ["time", "series"] and len(sh) == 4 * 3
    assert list(sh.columns) == ["sum_w", "share", "first", "last"]
    for mth, s in enumerate(steps):
        rows = sh.loc[index[s]]
        assert abs(rows["share"].sum() - 1.0) <= 1e-14
        aw = np.abs(np.nan_to_num(ref_w[mth]))
        for i in range(3):
            row = rows.loc["s%d" % i]
            assert abs(row["sum_w"] - np.nansum(ref_w[mth, :, i])) <= 1e-14
            assert abs(row["share"] - aw[:, i].sum() / aw.sum()) <= 1e-14
            if np.isfinite(yst[r, s, j]):
                continue   # an observed target (R = 0) is its own observation: the other weights are rounding noise, no window to speak of
            a, b = _shortest_window(aw[:, i], s, 0.9)
            assert (row["first"], row["last"]) == (index[a], index[b]), (mth, i)
            assert aw[a:b + 1, i].sum() >= 0.9 * aw[:, i].sum() * (1 - 1e-12) and a <= s <= b
    # a series that is never observed has no weight: share 0, no window
    mb.kf.obs_np[0, :, 1] = np.nan
    mb._cache.clear()
    none = mb.get_weight_shares(0, "s0", [3], alpha=alpha).loc[(mb.batch.index[0][3], "s1")]
    assert none["share"] == 0 and none["sum_w"] == 0 and pd.isna(none["first"]) and pd.isna(none["last"])

    # another parameter set: another run; argument errors
    mb.get_observation_weights(r, name, times, alpha=alpha * 1.01)
    assert mb.kf.calls == 4
    with pytest.raises(KeyError):
        mb.get_observation_weights(0, "nope", [0], alpha=alpha)
    with pytest.raises(KeyError):
        mb.get_observation_weights(0, "s0", [pd.Timestamp("1999-01-01")], alpha=alpha)
    with pytest.raises(IndexError):
        mb.get_observation_weights(1, "s0", [L[1]], alpha=alpha)
    with pytest.raises(ValueError):
        mb.get_observation_weights(0, "s0", [0])                   # no parameters


# ---- the binding ----
def test_the_two_entry_points_are_bound_as_the_header_declares_them():
    import __graft_entry__ as g
    from metran_amd import _lib

    src = open(os.path.join(ROOT, "include", "metran_hip.h")).read()
    for name in ("mk_weights_work_stride", "mk_observation_weights"):
        proto = re.search(r"MK_API\s+[\w\s\*]+?\b%s\s*\((.*?)\);" % name, src, re.S)
        assert proto, "%s is not declared in the header" % name
        assert len(proto.group(1).split(",")) == len(_lib.API[name][1]), name
    body = re.search(r"typedef struct mk_weights_request \{(.*?)\} mk_weights_request;", src, re.S).group(1)
    fields = [re.findall(r"(\w+)\s*$", d.strip())[0] for d in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if d.strip()]
    assert fields == [f[0] for f in _lib.WeightsRequest._fields_]
    assert re.search(r"#define MK_ABI_VERSION 7\b", src)
    if not os.path.exists(_lib.library_path()):
        g.build()
    L = _lib.lib()
    assert L.mk_abi_version() == 7 == _lib.ABI_VERSION
    # the stride without a GPU: the record plus N slots of (n + 3) & ~1 doubles; 0 where the shape is not served
    assert L.mk_weights_work_stride(3, 1) == L.mk_record_stride(4) + 3 * 6
    assert L.mk_weights_work_stride(8, 3) == L.mk_record_stride(11) + 8 * 14
    assert L.mk_weights_work_stride(61, 4) == 0 and L.mk_weights_work_stride(0, 1) == 0

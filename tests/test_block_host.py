"""Leave-block-out predictions without a GPU: the numpy restatement of the kernels' recursion (tests/block_ref.py) against the
DEFINITION (dense conditioning of the record's data vector in extended precision), the deliberately wrong variants far outside
the bars, the identities that tie the block to the leave-one-out predictions, the masked smoother and the objective, the host
layer of ``MetranBatch`` over a stand-in engine (tests/block_engine.py), and the ABI's declarations.

MEASURED (test_restatement_against_definition prints it): over every group, instance and block of the GPU tier the largest
(float64 restatement - definition) / (kappa * eps * unit), unit = scale for the means, scale^2 for the variances and max(1, m)
for quad and log det V, is mu = 1016 -- at (5,1), T = 70, on quad of a one-cell block (kappa = 1) whose quad is large, where the
extended-precision restatement is 690 from the definition too: it is the rounding of the inputs of e^2 / V, not of the solve.
Per group: 1016, 10.5, 16.5, 222, 55.3, 295, 9.2, 30.8.  block_ref.MU = 1100 is that rounded up, and the GPU tier's bar is the
LOO tier's flat bar + 4 * MU * kappa * eps * unit."""
import re

import numpy as np
import pytest

import block_ref as br
import call_forms as cf
from batch_standin import stand_in, two_models
from block_engine import BlockEngine
from conftest import ROOT

LD = np.longdouble
UNITS = dict(means=1, vars=2, quad=0, logdet=0, ovo=2)


def _mu(got, ref, g, i, blk):
    """The largest |got - ref| / (kappa * eps * unit) of a block, unit = scale, scale^2 or max(1, m)."""
    sc = float(br._model(g, i)[2][int(blk[0])])
    worst = 0.0
    for k, p in UNITS.items():
        a, b = np.atleast_1d(np.asarray(got[k], dtype=LD)), np.atleast_1d(np.asarray(ref[k], dtype=LD))
        ok = ~np.isnan(b)
        if ok.any():
            unit = sc ** p if p else max(1, ref["m"])
            worst = max(worst, float(np.abs(a[ok] - b[ok]).max()) / (ref["kappa"] * br.EPS * unit))
    return worst


@pytest.mark.parametrize("shape", br.GROUPS, ids=lambda s: "%dx%d-T%d" % s)
def test_restatement_against_definition(shape):
    """Both precisions of the restatement against the definition on every instance and block of the GPU tier's group; the float64
    restatement stays inside the bar WITHOUT the safety factor (so the reference alone does not use up the bar), the extended one
    too; mu (see the module docstring) is printed and held below block_ref.MU."""
    g = br.group(*shape)
    blocks = br.blocks(g)
    worst64 = worstld = mu = 0.0
    for i in range(g["B"]):
        for blk in blocks[i % g["R"]]:
            ref = br.definition(g, i, blk)
            if ref is None:
                assert br.recursion(g, i, blk) is None
                continue
            bar = br.bars(g, i, blk, ref, safety=1.0)
            r64, rld = br.recursion(g, i, blk, np.float64), br.recursion(g, i, blk, LD)
            assert not r64.get("degenerate") and r64["minpiv"] >= 100 * br.MIN_PIVOT, (i, blk, r64["minpiv"])
            d64, dld = br.distance(r64, ref, bar), br.distance(rld, ref, bar)
            assert d64 <= 1.0 and dld <= 1.0, (i, tuple(blk), ref["m"], ref["kappa"], d64, dld)
            assert br.distance(r64, rld, bar) <= 1.0, (i, tuple(blk))
            worst64, worstld = max(worst64, d64), max(worstld, dld)
            if ref["m"]:
                mu = max(mu, _mu(r64, ref, g, i, blk))
    print("(%d,%d) T=%d: float64 %.3g and extended %.3g of the bar without the safety factor; mu = %.3g" % (shape + (worst64, worstld, mu)))
    assert mu <= br.MU


def _instance_of(g, r):
    """An instance of record r whose i // S would name another record."""
    return next(i for i in range(g["B"]) if i % g["R"] == r and (i // g["S"]) % g["R"] != r)


def _lets_differ(g, r, blk, wrong, neighbour):
    """Whether the inputs let the wrong variant change the block at all."""
    js, t0, t1 = (int(x) for x in blk)
    seen = np.isfinite(g["obs"][r])
    cells = seen[t0:t1, js]
    if not cells.any():
        return False
    if wrong == "omega_gap":
        return any(not seen[e].any() and cells[:e - t0].any() and cells[e - t0 + 1:].any() for e in range(t0 + 1, t1 - 1))
    if wrong in ("omega_own_cell", "msc_sign"):
        return cells.sum() >= 2
    if wrong == "checkpoint_early":
        return t1 < g["T"] and seen[t1:].any()
    if wrong == "checkpoint_late":
        return seen[t1 - 1:].any()
    if wrong == "edge_lo":
        return cells[0] if t1 - t0 > 1 else (t0 > 0 and seen[t0 - 1, js])
    if wrong == "edge_hi":
        return cells[-1] if t1 - t0 > 1 else (t1 < g["T"] and seen[t1, js])
    if wrong == "keep_obsvar":
        return g["obsvar"][r, js] > 0
    if wrong == "neighbour_checkpoint":
        return seen[min(t1, neighbour):max(t1, neighbour)].any()
    return True


@pytest.mark.parametrize("wrong", br.WRONG)
@pytest.mark.parametrize("shape", [(8, 2, 17), (13, 4, 17)], ids=["8x2", "13x4"])
def test_wrong_variants_are_far_outside_the_bars(shape, wrong):
    """Each wrong variant is at least 1000 bars from the definition on some block of every record whose inputs let it differ (the
    record with a single observed step lets few of them), and at least two of the three records do (one for the observation variance, which about half the series have)."""
    g = br.group(*shape)
    blocks = br.blocks(g)
    records = 0
    for r in range(g["R"]):
        i = _instance_of(g, r)
        worst, could = 0.0, False
        for w, blk in enumerate(blocks[r]):
            if blk[0] < 0:
                continue
            others = [int(b[2]) for b in blocks[r] if b[0] >= 0 and b[2] != blk[2]]
            neighbour = others[w % len(others)]
            if not _lets_differ(g, r, blk, wrong, neighbour):
                continue
            could = True
            ref = br.definition(g, i, blk)
            got = br.recursion(g, i, blk, wrong=wrong, neighbour=neighbour)
            worst = np.inf if got.get("degenerate") else max(worst, br.distance(got, ref, br.bars(g, i, blk, ref)))
        if could:
            records += 1
            assert worst >= cf.FACTOR, "%s on record %d: only %.3g bars away" % (wrong, r, worst)
    assert records >= (1 if wrong == "keep_obsvar" else 2), wrong      # observation variances: about half the series have one


@pytest.mark.parametrize("shape", [(8, 2, 17), (13, 4, 17), (8, 2, 3)], ids=["8x2-T17", "13x4-T17", "8x2-T3"])
def test_identities(shape):
    """A one-cell block is the leave-one-out restatement's cell.  Masking the block in the oracle and smoothing gives the block's
    means and variances.  And the objective: with warm-up 0 the oracle's -2 log L is -2 log p(y) = sum over the observed cells of
    (log 2 pi + log f + v^2 / f).  p(y) = p(y_-I) p(y_I | y_-I) and -2 log p(y_I | y_-I) = m log 2 pi + log det V + quad, so
        -2 log L (block masked) = -2 log L (all) - (m log 2 pi + log det V + quad):
    masking takes the block's conditional density OUT.  In terms of the filter's own terms of the block's cells, B = sum over
    the block of (log f + v^2 / f): the terms of the cells OUTSIDE the block rise by B - (quad + log det V) when it is masked.
    (Masking lowers -2 log L whenever m log 2 pi + log det V + quad > 0; the sign is the one asserted here.)"""
    import oracle

    g = br.group(*shape)
    blocks = br.blocks(g)
    seen = 0
    for i in (0, 4, 8, 13):
        r = i % g["R"]
        full = cf.reference(g, i, 0, parts=("state", "loo"))
        d, rf, v = br.filter_tape(g, i)
        for blk in blocks[r]:
            js, t0, t1 = (int(x) for x in blk)
            if js < 0:
                continue
            got = br.recursion(g, i, blk)
            if got["m"] == 0:
                continue
            if t1 - t0 == 1:
                big = max(1.0, float(np.nanmax(np.abs(full["loo_means"]))))
                assert abs(got["means"][0] - full["loo_means"][t0, js]) <= cf.LOO_TOL * big
                assert abs(got["vars"][0] - full["loo_vars"][t0, js]) <= cf.LOO_TOL * big * big
            obs = g["obs"].copy()
            obs[r, t0:t1, js] = np.nan
            masked = cf.reference(cf.variant(g, obs=obs), i, 0, parts=("state",))
            have = np.isfinite(g["obs"][r, t0:t1, js])
            big = max(1.0, float(np.abs(masked["sim_means"]).max()))
            assert np.abs(got["means"] - masked["sim_means"][t0:t1, js])[have].max() <= 1e-9 * big
            assert np.abs(got["vars"] - masked["sim_vars"][t0:t1, js])[have].max() <= 1e-9 * big * big
            drop = got["m"] * np.log(2.0 * np.pi) + got["logdet"] + got["quad"]
            tol = 1e-10 * max(1.0, abs(full["mle"]), abs(drop))
            assert abs((full["mle"] - masked["mle"]) - drop) <= tol, (i, tuple(blk), full["mle"] - masked["mle"], drop)
            inside = rf[t0:t1, js] != 0
            block_terms = (-np.log(rf[t0:t1, js][inside]) + v[t0:t1, js][inside] ** 2 * rf[t0:t1, js][inside]).sum()
            outside_full = full["mle"] - got["m"] * np.log(2.0 * np.pi) - block_terms
            rise = masked["mle"] - outside_full
            assert abs(rise - (block_terms - got["quad"] - got["logdet"])) <= tol
            seen += 1
    assert seen >= 12
    assert oracle is not None


def _alpha():
    return np.array([[8.0, 6.0, 9.0, 12.0], [5.0, 7.0, 8.0, 10.0]])


def test_gap_predictions_over_a_stand_in_engine():
    """Index handling (timestamps and steps, end = None, a model without gaps), units, the rows of observed cells only, the cache,
    the refusal of a gap longer than 64 steps."""
    import pandas as pd

    models, G = two_models()
    mb = stand_in(BlockEngine, models, G)
    kf = mb.kf
    alpha = _alpha()
    idx0 = mb.batch.index[0]
    gaps = [(0, "s1", idx0[5], idx0[12]), (0, "s0", 30, None), (0, "s2", 3, 4)]
    frame = mb.get_gap_predictions(gaps, alpha=alpha)
    assert list(frame.columns) == ["observed", "predicted", "stderr"] and frame.index.names == ["model", "series", "gap", "time"]
    obs = kf.obs_np
    std, mean = mb._std.numpy(), mb._mean.numpy()
    n0 = int(np.isfinite(obs[0, 5:12, 1]).sum())
    rows = frame.loc[(0, "s1", 0)]
    assert len(rows) == n0 and all(idx0[5] <= t < idx0[12] for t in rows.index)
    assert len(frame.loc[(0, "s0", 1)]) == int(np.isfinite(obs[0, 30:, 0]).sum())
    first = rows.index[0]
    t = list(idx0).index(first)
    assert rows.loc[first, "observed"] == pytest.approx(obs[0, t, 1] * std[0, 1] + mean[0, 1], rel=1e-14)
    assert kf.calls.count(("block_predict", 2, 3)) == 1
    again = mb.get_gap_predictions(gaps, alpha=alpha, standardized=True)
    assert kf.calls.count(("block_predict", 2, 3)) == 1                   # the cache
    np.testing.assert_allclose(again["observed"].values * np.repeat(1.0, len(again)), (frame["observed"].values - np.array(
        [mean[0, mb._series(0, s)] for s in frame.index.get_level_values("series")])) / np.array(
        [std[0, mb._series(0, s)] for s in frame.index.get_level_values("series")]), rtol=1e-12)
    np.testing.assert_allclose(again["stderr"].values, frame["stderr"].values / np.array(
        [std[0, mb._series(0, s)] for s in frame.index.get_level_values("series")]), rtol=1e-12)
    # the standardised predictions are the restatement's own
    g = cf.variant(kf._group(*kf.params_from_alpha(alpha, dt=mb.dt)), scale=None, offset=None)
    ref = br.recursion(g, 0, (1, 5, 12))
    np.testing.assert_allclose(again.loc[(0, "s1", 0), "predicted"].values, ref["means"][np.isfinite(ref["means"])], rtol=0, atol=1e-12)
    info = frame.attrs["gaps"]
    assert info.loc[(0, "s1", 0), "n_obs"] == n0 and not info["degenerate"].any() and info.loc[(0, "s0", 1), "steps"] == 10
    assert isinstance(frame.index.get_level_values("time")[0], pd.Timestamp)
    with pytest.raises(ValueError, match="64"):
        stand_in(BlockEngine, *_long_models()).get_gap_predictions([(0, "s0", 0, 65)], alpha=np.array([[8.0, 6.0, 9.0, 12.0]]))
    with pytest.raises(KeyError):
        mb.get_gap_predictions([(0, "nobody", 3, 5)], alpha=alpha)
    with pytest.raises(IndexError):
        mb.get_gap_predictions([(2, "s1", 3, 5)], alpha=alpha)
    with pytest.raises(ValueError):
        mb.get_gap_predictions([(0, "s1", 5, 5)], alpha=alpha)
    with pytest.raises(ValueError):
        mb.get_gap_predictions([], alpha=alpha)


def _long_models():
    import pandas as pd

    rng = np.random.default_rng(8)
    idx = pd.date_range("2001-01-01", periods=80, freq="D")
    cols = [pd.Series(rng.normal(size=80), index=idx, name="s%d" % j) for j in range(3)]
    return [cols], np.array([[[0.6], [0.5], [-0.4]]])


def test_gap_fill_skill_over_a_stand_in_engine():
    """The tiling from t_first, the skipped blocks, the sums against a plain loop, length 1 from the leave-one-out route, and the
    same table when a tiny budget makes the models go one at a time."""
    models, G = two_models()
    mb = stand_in(BlockEngine, models, G)
    kf = mb.kf
    alpha = _alpha()
    table = mb.gap_fill_skill(lengths=(1, 4, 7), alpha=alpha, t_first=2, coverage=0.9)
    assert list(table.columns) == ["n_blocks", "n_cells", "bias", "rmse", "msse", "coverage", "log_score", "rmse_loo"]
    assert table.index.names == ["model", "series", "length"] and len(table) == 2 * 3 * 3
    assert list(table.index[:4]) == [(0, "s0", 1), (0, "s0", 4), (0, "s0", 7), (0, "s1", 1)]
    obs, std = kf.obs_np, mb._std.numpy()
    g = cf.variant(kf._group(*kf.params_from_alpha(alpha, dt=mb.dt)), scale=None, offset=None)
    for r, j, h in ((0, 1, 4), (1, 2, 7), (1, 0, 4)):
        Lr = int(mb.batch.lengths[r])
        nb = nc = 0
        err, msse, ls = [], [], []
        for t0 in range(2, Lr, h):
            t1 = min(t0 + h, Lr)
            if not np.isfinite(obs[r, t0:t1, j]).any():
                continue
            row = br.recursion(g, r, (j, t0, t1))
            nb, nc = nb + 1, nc + row["m"]
            have = np.isfinite(row["means"])
            err += list((obs[r, t0:t1, j] - row["means"])[have])
            msse.append(row["quad"] / row["m"])
            ls.append((row["m"] * np.log(2 * np.pi) + row["logdet"] + row["quad"]) / row["m"])
        got = table.loc[(r, "s%d" % j, h)]
        assert got["n_blocks"] == nb and got["n_cells"] == nc
        np.testing.assert_allclose([got["bias"], got["rmse"], got["msse"], got["log_score"]],
                                   [np.mean(err) * std[r, j], np.sqrt(np.mean(np.square(err))) * std[r, j], np.mean(msse), np.mean(ls)], rtol=1e-10)
        assert 0.0 <= got["coverage"] <= 1.0
    # length 1: the leave-one-out route; rmse_loo is its own rmse, and no block_predict call has one-step blocks
    ones = table.xs(1, level="length")
    np.testing.assert_allclose(ones["rmse"].values, ones["rmse_loo"].values, rtol=1e-12)
    sevens = table.xs(7, level="length")
    assert (sevens["rmse"].values >= 0.999 * sevens["rmse_loo"].values).sum() >= 4      # a week's gap is not easier than one day's
    skipped = sum(1 for t0 in range(2, 40, 4) if not np.isfinite(obs[0, t0:t0 + 4, 0]).any())
    assert table.loc[(0, "s0", 4), "n_blocks"] == len(range(2, 40, 4)) - skipped
    calls = [c for c in kf.calls if c[0] == "block_predict"]
    assert len(calls) == 2 and all(c[1] == 2 for c in calls)
    before = len(kf.calls)
    per = 8.0 * (max(c[2] for c in calls) * (4 + 16 + 2 * 7 + 4.5) + mb.T * kf._reader_stride("blocks"))
    small = mb.gap_fill_skill(lengths=(1, 4, 7), alpha=alpha, t_first=2, coverage=0.9, budget=1.5 * per)
    chunks = [c for c in kf.calls[before:] if c[0] == "block_predict"]
    assert len(chunks) == 4 and all(c[1] == 1 for c in chunks)
    assert np.array_equal(small.values, table.values, equal_nan=True) and small.index.equals(table.index)
    with pytest.raises(MemoryError):
        mb.gap_fill_skill(lengths=(4,), alpha=alpha, budget=8.0)
    with pytest.raises(ValueError):
        mb.gap_fill_skill(lengths=(65,), alpha=alpha)
    with pytest.raises(ValueError):
        mb.gap_fill_skill(lengths=(4,), alpha=alpha, coverage=1.5)


def test_abi_declares_the_block_entry_points():
    """include/metran_hip.h and the ctypes binding agree on the three entry points and on mk_block_request's fields; the engine has
    the method, the allocator and the accessor."""
    from metran_amd import _lib
    from metran_amd.batch import MetranBatch
    from metran_amd.engine import BatchedKalman

    src = open(ROOT + "/include/metran_hip.h").read()
    declared = set(re.findall(r"MK_API\s+[\w\s\*]+?\b(mk_\w+)\s*\(", src))
    for name in ("mk_block_max_cells", "mk_block_work_stride", "mk_block_predict"):
        assert name in declared and name in _lib.API
    body = re.search(r"typedef struct mk_block_request \{(.*?)\} mk_block_request;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.findall(r"(\w+)\s*$", d.strip())[0] for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in _lib.BlockRequest._fields_]
    assert "MK_ABI_VERSION 7" in src and _lib.ABI_VERSION == 7
    assert "blocks" in BatchedKalman._READERS and isinstance(BatchedKalman.block_predict_supported, property)
    assert all(hasattr(BatchedKalman, k) for k in ("block_predict", "alloc_block_predict"))
    assert all(hasattr(MetranBatch, k) for k in ("get_gap_predictions", "gap_fill_skill"))
    hip = open(ROOT + "/metran_amd/csrc/block_kernels.hip").read()
    assert "regress_min_pivot" in hip and "1e-12" not in hip.split("#include")[-1]     # the regression's constant, not restated


def test_the_degenerate_block_is_degenerate_on_the_cpu():
    """The construction of the GPU tier's degenerate block (block_ref.degenerate_group): in the float64 restatement the scaled pivot
    of the block (0, 4, 6) of instance 0 is below regress_min_pivot by a factor of at least 100, every other block's of both
    instances is above it by at least 100, and every f of the filter is positive."""
    g = br.degenerate_group()
    for i in range(g["B"]):
        _, rf, _ = br.filter_tape(g, i)
        assert (rf[np.isfinite(g["obs"][0])] > 0).all() and np.isfinite(rf).all()
        for w, blk in enumerate(br.DEGENERATE_BLOCKS[0]):
            row = br.recursion(g, i, blk)
            if (i, w) == (0, 0):
                assert row.get("degenerate") and row["minpiv"] <= br.MIN_PIVOT / 100 and row["m"] == 2
                assert np.isnan(row["means"]).all() and np.isnan(row["quad"])
            else:
                assert not row.get("degenerate") and row["minpiv"] >= 100 * br.MIN_PIVOT, (i, w, row["minpiv"])

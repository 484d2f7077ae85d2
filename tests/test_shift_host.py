"""The level-shift scan without a GPU: the numpy restatement of the kernel's recursion (tests/shift_ref.py) against the DEFINITION
(dense precision of the record's data vector in extended precision), the deliberately wrong variants outside the bar, the
equality with the regression of one level effect, the host layer of ``MetranBatch`` over a stand-in engine
(tests/shift_engine.py), a planted shift that the definition and ``detect_level_shifts`` find, and the ABI's declarations.

MEASURED (test_restatement_against_definition prints it): over every group, instance and candidate of the GPU tier the largest
(float64 restatement - definition) / (eps * scale), scale = |x|'|u| for A and |x|'|M||x| for D, is mu = 1288 -- at (8,2), T = 2,
where the extended-precision restatement is 27 times closer to the definition: it is the rounding of the float64 walk (the
differences that form N and M_ss under the given P0), not the recursion.  Per group, in shift_ref.GROUPS' order: 101, 14.1,
1288, 429, 22, 195, 18.6, 443, 7.25, 261, 35.3.  shift_ref.MU = 1300 is that rounded up, and the GPU tier's bar is
4 * MU * eps * scale + 1e-12.  The two groups this tier adds, (60,4) and (15,1) at T = 5, measure 3899 and 4263 and are held to a
bar of their own (shift_ref.MU_EXTRA = 4300): the other groups keep theirs.

Which groups can tell a wrong variant from the right recursion (TELLS; measured, then asserted): a group with T = 1 tells none of
the variants that need an earlier cell of the same series (its Omega is never read), and none is claimed for it."""
import re

import numpy as np
import pytest

import regress_ref
import shift_ref as sr
from batch_standin import stand_in, two_models
from conftest import ROOT
from shift_engine import ShiftEngine, raw_facade

LD = np.longdouble
IDS = lambda s: "%dx%d-T%d" % s  # noqa: E731


@pytest.mark.parametrize("shape", sr.GROUPS, ids=IDS)
def test_restatement_against_definition(shape):
    """Both precisions of the restatement against the definition on every instance and candidate of the GPU tier's group; the
    float64 restatement stays inside the bar WITHOUT the safety factor (so the reference alone does not use up the bar), the
    extended one too; mu (see the module docstring) is printed and held below shift_ref.MU."""
    g = sr.group(*shape)
    worst64 = worstld = mu = 0.0
    for i in range(g["B"]):
        ref = sr.definition(g, i)
        bar = sr.bars(ref, safety=1.0)
        r64, rld = sr.recursion(g, i, np.float64), sr.recursion(g, i, LD)
        seen = np.isfinite(g["obs"][i % g["R"]])
        assert np.array_equal(np.isfinite(r64["num"]), seen) and np.array_equal(np.isfinite(ref["num"].astype(float)), seen)
        assert (ref["den"][seen] > 0).all()
        d64, dld = sr.distance(r64, ref, bar), sr.distance(rld, ref, bar)
        assert d64 <= 1.0 and dld <= 1.0, (i, d64, dld)
        worst64, worstld, mu = max(worst64, d64), max(worstld, dld), max(mu, sr.mu_of(r64, ref))
    print("(%d,%d) T=%d: float64 %.3g and extended %.3g of the bar without the safety factor; mu = %.3g" % (shape + (worst64, worstld, mu)))
    assert mu <= sr.MU_EXTRA.get(shape, sr.MU)


@pytest.mark.parametrize("shape", [(8, 2), (13, 4)], ids=["8x2", "13x4"])
def test_status_twins_are_inside_the_measured_mu(shape):
    """The clean twins of tests/status_cases.py, which tests/test_shift_gpu.py::test_status holds to the same bar: their mu is
    below shift_ref.MU too (printed)."""
    import status_cases as sc

    g = sc.case(shape[0], shape[1], "neg_once")["twin"]
    mu = max(sr.mu_of(sr.recursion(g, i), sr.definition(g, i)) for i in range(g["B"]))
    print("(%d,%d) twin of neg_once: mu = %.3g" % (shape + (mu,)))
    assert mu <= sr.MU


# instances of the records 1, 2 and 0 whose i // S names another record
WRONG_INSTANCES = (1, 5, 9)
SEVERAL = tuple(s for s in sr.GROUPS if s not in sr.SINGLE_STEP)     # some series has two cells
# wrong variant -> the groups in which it is outside the bar on one of WRONG_INSTANCES (measured: 9e8 bars and more everywhere)
TELLS = {
    "omega_gap": tuple(s for s in sr.GROUPS if s[2] >= 17) + ((8, 2, 3),),   # an empty step between two cells of a series
    "own_cell_first": tuple(s for s in sr.GROUPS if s[2] > 1),               # (differs at T = 1 too: not claimed)
    "m_sign": SEVERAL,                # needs an earlier cell of the same series
    "d_single": SEVERAL,              # the same
    "store_early": tuple(s for s in sr.GROUPS if s[2] > 1),                  # (differs at T = 1 too: not claimed)
    "record_div": tuple(s for s in sr.GROUPS if s[2] > 1),                   # (differs at T = 1 too: not claimed)
    "neighbour_omega": SEVERAL,       # needs an earlier cell of the same series
}


@pytest.mark.parametrize("wrong", sr.WRONG)
def test_wrong_variants_are_outside_the_bar(wrong):
    """Each wrong variant is outside the bar around the definition -- by the factor printed -- in every group TELLS names, on some
    instance of WRONG_INSTANCES; T = 1 is claimed for none (one cell per series: Omega is written and never read)."""
    assert set(TELLS) == set(sr.WRONG)
    line = []
    for shape in TELLS[wrong]:
        g = sr.group(*shape)
        worst = 0.0
        for i in WRONG_INSTANCES:
            worst = max(worst, sr.distance(sr.recursion(g, i, wrong=wrong), sr.definition(g, i)))
        line.append("%s %.3g" % (IDS(shape), worst))
        assert worst > 1.0, "%s at %s: only %.3g bars away" % (wrong, IDS(shape), worst)
    print("%s, bars from the definition: %s" % (wrong, ", ".join(line)))


@pytest.mark.parametrize("shape", [(8, 2, 17), (13, 4, 17)], ids=IDS)
def test_equals_the_regression_of_one_level_effect(shape):
    """For a candidate tau >= t_first = 1 the regression restatement (tests/regress_ref.py, extended precision) with the single
    effect (j, level, tau, T) gives beta = A / D, cov = 1 / D and gain = A^2 / D: (beta / cov, 1 / cov) is inside the scan's bar
    around the definition, and gain inside what those two bars allow A^2 / D."""
    g = sr.group(*shape)
    N, T = g["N"], g["T"]
    checked = 0
    for i in (0, 7, 14):
        r = i % g["R"]
        ref = sr.definition(g, i)
        bar = sr.bars(ref)
        seen = np.isfinite(g["obs"][r])
        for j in range(N):
            steps = [t for t in np.nonzero(seen[:, j])[0] if t >= 1]
            for tau in steps[::4]:
                out = regress_ref.regression(g["obs"][r], g["phi"][i], g["q"][i], g["loadings"][r], g["obsvar"][r], g["x0"][i], g["P0"][i],
                                             [(j, regress_ref.LEVEL, tau, T)], 1)
                assert not out["dropped"][0]
                A, D = ref["num"][tau, j], ref["den"][tau, j]
                beta, cov = LD(out["beta"][0]), LD(out["cov"][0, 0])
                assert abs(beta / cov - A) <= bar["num"][tau, j] and abs(1 / cov - D) <= bar["den"][tau, j], (i, j, tau)
                allow = (2 * abs(A) * bar["num"][tau, j] + A * A / D * bar["den"][tau, j]) / D + 1e-12
                assert abs(LD(out["gain"]) - A * A / D) <= allow, (i, j, tau)
                checked += 1
    assert checked >= 30


# ------------------------------------------------------------------------------------------------------------- host layer
ALPHA = np.full((2, 4), 10.0)


def _facade():
    models, G = two_models()
    return stand_in(ShiftEngine, models, G)


def _scan(mb):
    g = mb.kf._group(*mb.kf.params_from_alpha(ALPHA, dt=mb.dt))
    return [sr.recursion(g, i) for i in range(mb.R)]


def test_statistics_units_nan_pattern_and_cache():
    mb = _facade()
    kf = mb.kf
    orig = mb.get_level_shift_statistics(ALPHA)
    assert [c[0] for c in kf.calls] == ["level_shifts"]
    std_units = mb.get_level_shift_statistics(ALPHA, standardized=True)
    frame = mb.get_level_shift(1, "s2", alpha=ALPHA)
    assert [c[0] for c in kf.calls] == ["level_shifts"]             # a second call, other units, one series: nothing is launched
    seen = np.isfinite(kf.obs_np)
    std = mb._std.numpy()
    rows = _scan(mb)
    for key in ("estimate", "stderr", "t"):
        assert tuple(orig[key].shape) == (mb.R, mb.T, mb.N)
        assert np.array_equal(np.isfinite(orig[key].numpy()), seen) and np.array_equal(np.isfinite(std_units[key].numpy()), seen)
    for r in range(mb.R):
        A, D = rows[r]["num"], rows[r]["den"]
        assert np.allclose(std_units["estimate"][r].numpy()[seen[r]], (A / D)[seen[r]], rtol=1e-14, atol=0)
        assert np.allclose(std_units["stderr"][r].numpy()[seen[r]], (1 / np.sqrt(D))[seen[r]], rtol=1e-14, atol=0)
        assert np.allclose(std_units["t"][r].numpy()[seen[r]], (A / np.sqrt(D))[seen[r]], rtol=1e-14, atol=0)
        for key in ("estimate", "stderr"):   # original units: times the series' standard deviation; the mean does not enter
            assert np.allclose(orig[key][r].numpy()[seen[r]], (std_units[key][r].numpy() * std[r][None, :])[seen[r]], rtol=1e-14, atol=0)
        assert np.array_equal(orig["t"][r].numpy(), std_units["t"][r].numpy(), equal_nan=True)
    L = int(mb.batch.lengths[1])
    assert list(frame.columns) == ["estimate", "stderr", "t"] and frame.index.equals(mb.batch.index[1][:L])
    assert np.array_equal(frame["t"].values, orig["t"][1, :L, 2].numpy(), equal_nan=True)
    mb.get_level_shift_statistics(ALPHA + 1.0)                       # another parameter set is another run
    assert [c[0] for c in kf.calls] == ["level_shifts"] * 2


@pytest.mark.parametrize("t_first,min_segment", [(1, 5), (12, 3), (0, 1), (1, 100)])
def test_screen_candidates_and_sidak(t_first, min_segment):
    """The candidates counted cell by cell, the maximum over them, Sidak's 1 - (1 - p)^m; rows without candidates NaN / NaT."""
    import pandas as pd
    from scipy.stats import norm

    mb = _facade()
    table = mb.screen_level_shifts(alpha=ALPHA, t_first=t_first, min_segment=min_segment)
    assert list(table.columns) == ["max_abs_t", "time", "estimate", "stderr", "ncand", "pvalue"]
    assert list(table.index.names) == ["model", "series"] and len(table) == mb.R * mb.N
    stat = {k: v.numpy() for k, v in mb.get_level_shift_statistics(ALPHA).items()}
    seen = np.isfinite(mb.kf.obs_np)
    some = 0
    for r in range(mb.R):
        for j, name in enumerate(mb.batch.names[r]):
            row = table.loc[(r, name)]
            steps = list(np.nonzero(seen[r, :, j])[0])
            cand = [t for k, t in enumerate(steps) if t >= t_first and k >= min_segment and len(steps) - k >= min_segment]
            assert row["ncand"] == len(cand)
            if not cand:
                assert np.isnan(row["max_abs_t"]) and pd.isna(row["time"]) and np.isnan(row["estimate"]) and np.isnan(row["stderr"]) and np.isnan(row["pvalue"])
                continue
            some += 1
            best = max(cand, key=lambda t: abs(stat["t"][r, t, j]))
            assert row["time"] == mb.batch.index[r][best] and row["max_abs_t"] == abs(stat["t"][r, best, j])
            assert row["estimate"] == stat["estimate"][r, best, j] and row["stderr"] == stat["stderr"][r, best, j]
            p = 2.0 * norm.sf(row["max_abs_t"])
            assert row["pvalue"] == pytest.approx(1.0 - (1.0 - p) ** len(cand), rel=1e-9, abs=1e-15)
            assert (p <= row["pvalue"] <= min(1.0, len(cand) * p * (1 + 1e-12))) or len(cand) == 1
    assert (some == 0) == (min_segment == 100)


def _records(kf):
    return kf.obs_np, kf.obs_np.copy()


def _restored(kf, before):
    return kf.obs_np is before[0] and np.array_equal(kf.obs_np, before[1], equal_nan=True) and not kf.observations_adjusted


def test_detect_stopping_rules():
    mb = _facade()
    kf = mb.kf
    before = _records(kf)
    nothing = mb.detect_level_shifts(level=1e-300, alpha=ALPHA, min_segment=5)          # nothing is that significant: one scan
    assert len(nothing) == 0 and list(nothing.columns) == list(mb._INTERVENTION_COLUMNS) and list(nothing.index.names) == ["model", "effect"]
    assert kf.scans == 1 and kf.regressions == 0 and _restored(kf, before)
    fitted = mb.fit_interventions([(0, "s0", "level", 10)], alpha=ALPHA)
    assert list(fitted.columns) == list(nothing.columns)
    kf.scans = kf.regressions = 0
    one = mb.detect_level_shifts(level=1 - 1e-12, max_shifts=1, alpha=ALPHA, min_segment=5)   # everything passes: one per model, one round
    assert kf.scans == 1 and kf.regressions == 1 and _restored(kf, before)
    assert sorted(one.index.get_level_values("model")) == [0, 1] and (one["kind"] == "level").all() and one["end"].isna().all()
    screen = mb.screen_level_shifts(alpha=ALPHA, min_segment=5)
    for r in range(mb.R):                    # the model's candidate with the largest |t| over all its series
        best = screen.xs(r, level="model")["max_abs_t"].idxmax()
        assert one.loc[(r, 0), "series"] == best and one.loc[(r, 0), "start"] == screen.loc[(r, best), "time"]
    kf.scans = kf.regressions = 0
    three = mb.detect_level_shifts(level=1 - 1e-12, max_shifts=3, alpha=ALPHA, min_segment=5)
    assert kf.scans == 3 and _restored(kf, before)
    for r in range(mb.R):                    # three rounds, three different (series, date) pairs per model, the first one as above
        rows = three.xs(r, level="model")
        assert len(rows) == 3 and len(set(zip(rows["series"], rows["start"]))) == 3
        assert rows.iloc[0]["series"] == one.loc[(r, 0), "series"] and rows.iloc[0]["start"] == one.loc[(r, 0), "start"]
    for bad in (0, 17):
        with pytest.raises(ValueError):
            mb.detect_level_shifts(max_shifts=bad, alpha=ALPHA)
    with pytest.raises(ValueError):
        mb.detect_level_shifts(level=0.0, alpha=ALPHA)


@pytest.mark.parametrize("fails", ["regression", "scan"])
def test_detect_restores_the_records_when_a_step_raises(fails):
    """The second regression raises when the records are as they were, the second scan when they are adjusted: either way the
    records are the very arrays they were."""
    mb = _facade()
    kf = mb.kf
    before = _records(kf)
    if fails == "regression":
        kf.fail_regression_at = 2
    else:
        kf.fail_scan_at = 2
    with pytest.raises(RuntimeError, match="on purpose"):
        mb.detect_level_shifts(level=1 - 1e-12, max_shifts=4, alpha=ALPHA, min_segment=5)
    assert kf.scans >= 2 if fails == "scan" else kf.regressions == 2
    assert _restored(kf, before)


def test_detect_refuses_adjusted_records():
    mb = _facade()
    kf = mb.kf
    mb.fit_interventions([(0, "s0", "level", 10)], alpha=ALPHA)
    mb.adjust_observations()
    assert kf.observations_adjusted
    adjusted = kf.obs_np
    with pytest.raises(ValueError, match="adjusted"):
        mb.detect_level_shifts(alpha=ALPHA)
    assert kf.obs_np is adjusted and kf.observations_adjusted and kf.scans == 0      # nothing was touched
    mb.unadjust_observations()
    assert not kf.observations_adjusted


# ------------------------------------------------------------------------------------------------------------ planted shifts
def planted_models():
    """The planted-shift records (shift_ref.planted) as the series ``MetranBatch`` takes: (models, loadings, alpha, index); for
    ``shift_engine.raw_facade``, which keeps them in the units they were simulated in."""
    import pandas as pd

    d = sr.planted()
    idx = pd.date_range("2001-01-01", periods=sr.PLANT_T, freq="D")
    models = [[pd.Series(d["obs"][r, :, j], index=idx, name="s%d" % j).dropna() for j in range(sr.PLANT_N)] for r in range(sr.PLANT_R)]
    return models, d["loadings"], d["alpha"], idx


def check_planted(mb, alpha, idx):
    """``detect_level_shifts`` returns exactly the planted (model, series, date) rows, nothing for the untouched models."""
    frame = mb.detect_level_shifts(level=0.01, alpha=alpha, min_segment=sr.PLANT_MIN_SEGMENT)
    got = sorted((model, row["series"], row["start"]) for (model, _), row in frame.iterrows())
    assert got == sorted((r, "s%d" % j, idx[t]) for r, j, t in sr.PLANTED), got
    assert (frame["kind"] == "level").all() and frame["end"].isna().all() and not frame["dropped"].any()
    assert (frame["estimate"] > 0).all() and (frame["t"] > 5).all()
    return frame


def test_planted_shifts_are_found():
    """A shift of 10 one-step prediction standard deviations: the DEFINITION puts the largest |t| of the series, over the
    candidates, at exactly the planted step; ``detect_level_shifts`` over the stand-in returns exactly the three planted rows."""
    models, loadings, alpha, idx = planted_models()
    mb = raw_facade(ShiftEngine, models, loadings)
    kf = mb.kf
    before = _records(kf)
    assert np.array_equal(kf.obs_np, sr.planted()["obs"], equal_nan=True)
    phi, q = kf.params_from_alpha(alpha, dt=mb.dt)
    g = sr.plant_group(kf.obs_np, kf.load_np, phi.numpy(), q.numpy())
    cand = mb._shift_candidates(1, sr.PLANT_MIN_SEGMENT)
    for r, j, t in sr.PLANTED:
        ref = sr.definition(g, r)
        tt = np.abs((ref["num"] / np.sqrt(ref["den"])).astype(float))[:, j]
        assert cand[r, t, j]
        assert int(np.argmax(np.where(cand[r, :, j], tt, -1.0))) == t, (r, j, t, int(np.argmax(np.where(cand[r, :, j], tt, -1.0))))
    check_planted(mb, alpha, idx)
    assert _restored(kf, before)


def test_abi_declarations():
    """The header, the ctypes prototypes and the C file name the same two entry points and the same request."""
    from metran_amd import _lib

    header = open(ROOT + "/include/metran_hip.h").read()
    assert re.search(r"MK_API int64_t mk_shift_work_stride\(int64_t N, int64_t K\);", header)
    assert re.search(r"MK_API int mk_level_shifts\(mk_context \*ctx, const mk_problem \*prob, double \*d_work, int time_major, "
                     r"const mk_shift_request \*req,\s+uint32_t \*d_status\);", header)
    body = re.search(r"typedef struct mk_shift_request \{(.*?)\} mk_shift_request;", header, re.S).group(1)
    assert re.findall(r"double \*(\w+);", body) == [name for name, _ in _lib.ShiftRequest._fields_] == ["d_num", "d_den"]
    capi = open(ROOT + "/metran_amd/csrc/mk_capi.hip").read()
    assert "MK_API int64_t mk_shift_work_stride(" in capi and "MK_API int mk_level_shifts(" in capi

"""Window statistics of posterior draws, CPU tier: the numpy restatement (tests/ensemble_ref.py) pinned against independent
formulations, each deliberate mistake shown to be visible on the shared test inputs, the window translation
(metran_amd/windows.py) against pandas' resample, and the kernels of ensemble_kernels.hip themselves, compiled for the host
(tests/ensemble_host_emulation.py), against the restatement in both layouts."""
import numpy as np
import pandas as pd
import pytest

import ensemble_ref as ref
from metran_amd.windows import step_windows

EPS = 2.0 ** -52


# ------------------------------------------------------------------ the restatement against independent formulations
@pytest.mark.parametrize("S", [2, 3, 5, 33, 64, 65, 1000])
def test_summary_restatement_against_numpy(S):
    values = ref.summary_values(S)
    got = ref.ensemble_summary(values, ref.PROBS)
    for cell in range(values.shape[1]):
        x = values[:, cell][np.isfinite(values[:, cell])]
        assert got[cell, 0] == x.size
        if x.size == 0:
            assert np.isnan(got[cell, 1:]).all()
            continue
        bar = 4.0 * EPS * np.abs(x).max()
        assert got[cell, 3] == np.min(x) and got[cell, 4] == np.max(x)
        assert abs(got[cell, 1] - np.mean(x)) <= x.size * EPS * np.abs(x).max()   # pairwise against sequential adds
        if x.size > 1:
            assert abs(got[cell, 2] - np.std(x, ddof=1)) <= bar
        else:
            assert np.isnan(got[cell, 2])
        assert np.abs(got[cell, 5:] - np.quantile(x, ref.PROBS)).max() <= bar


def _spell_by_run_lengths(under):
    """Longest run of True: the lengths between the edges of the padded indicator."""
    edges = np.flatnonzero(np.diff(np.concatenate([[0], under.astype(np.int8), [0]])))
    return float((edges[1::2] - edges[::2]).max()) if edges.size else 0.0


@pytest.mark.parametrize("T", [1, 2, 33, 200])
def test_path_restatement_against_independent_formulations(T):
    paths, thr = ref.synthetic_paths(3, 15, T, 8)
    for win in ref.window_sets(T):
        got = ref.path_functionals(paths, win, thr)
        R, W = win.shape[:2]
        for s, i, j in [(0, 0, 7), (1, 1, 0), (2, 4, 7), (2, 5, 7), (0, 14, 2), (1, 7, 1)]:
            for w in range(W):
                a, b = win[i % R, w]
                y, c, five = paths[s, i, a:b, j], thr[i % R, j], got[s, i, j, w]
                if b == a or np.isnan(y).any():
                    assert np.isnan(five).all()
                    continue
                assert abs(five[0] - np.mean(y)) <= (b - a) * EPS * np.abs(y).max()
                assert five[1] == np.min(y) and five[2] == np.max(y)
                if np.isnan(c):
                    assert np.isnan(five[3:]).all()
                else:
                    assert five[3] == np.count_nonzero(y < c) / (b - a) and five[4] == _spell_by_run_lengths(y < c)


def test_each_mistake_is_visible_on_the_test_inputs():
    """Every mutated restatement differs from the right one on the inputs the kernels are tested with."""
    T = 33
    paths, thr = ref.synthetic_paths(3, 15, T, 8)
    win = ref.window_sets(T)[1]
    good = ref.path_functionals(paths, win, thr)
    for wrong in ("long_start", "long_stop", "le", "carry", "nan_counted"):
        assert not ref.same_bits(ref.path_functionals(paths, win, thr, wrong=wrong), good), wrong
    # `le` is seen through the one level that equals a path value, and nowhere else
    le = ref.path_functionals(paths, win, thr, wrong="le")
    differs = np.argwhere(~(np.isclose(le, good, rtol=0, atol=0, equal_nan=True)))
    assert {tuple(d[:3]) for d in differs} == {(0, 0, 7)}
    values = ref.summary_values(33)
    right = ref.ensemble_summary(values, ref.PROBS)
    for wrong, col in (("m_divisor", 2), ("ceil", 6)):
        bad = ref.ensemble_summary(values, ref.PROBS, wrong=wrong)
        assert np.abs(bad[0, col] - right[0, col]) > 1e3 * ref.summary_bar(values)[0], wrong


# ------------------------------------------------------------------ the window translation against pandas
def _ragged_daily_frames():
    rng = np.random.default_rng(5)
    frames = []
    for start, days in (("2001-01-17", 800), ("2000-11-30", 1100), ("2001-03-01", 420)):
        index = pd.date_range(start, periods=days, freq="D")
        keep = np.ones(days, dtype=bool)
        keep[rng.integers(0, days, days // 6)] = False
        keep[200:275] = False                      # a gap that swallows whole months
        frames.append(pd.DataFrame(rng.standard_normal((int(keep.sum()), 2)), index=index[keep], columns=["a", "b"]))
    return frames


@pytest.mark.parametrize("alias", ["MS", "YS"])
def test_window_translation_against_resample(alias):
    frames = _ragged_daily_frames()
    T = max(len(f) for f in frames) + 3            # padded steps beyond every model's length
    steps, starts = step_windows([f.index for f in frames], alias, T)
    W = steps.shape[1]
    assert steps.shape == (len(frames), W, 2) and steps.dtype == np.int64
    paths = np.full((1, len(frames), T, 2), 1e6)   # the padding would be seen in any window that reached it
    for r, f in enumerate(frames):
        paths[0, r, : len(f)] = f.values
    got = ref.path_functionals(paths, steps, None)
    for r, f in enumerate(frames):
        res = f.resample(alias)
        mean, low = res.mean(), res.min()
        assert list(starts[r]) == list(mean.index)
        assert (steps[r, len(starts[r]):] == T).all()                      # the pads are (T, T)
        for j in range(2):
            np.testing.assert_allclose(got[0, r, j, : len(mean), 0], mean.values[:, j], rtol=0, atol=400 * EPS * np.abs(f.values).max(),
                                       equal_nan=True)   # pairwise against sequential adds over at most 366 steps
            np.testing.assert_array_equal(got[0, r, j, : len(low), 1], low.values[:, j])
        assert np.isnan(got[0, r, :, len(mean):]).all()
        assert alias == "YS" or np.isnan(mean.values).any()                # the swallowed months are there, as empty windows


def test_explicit_windows_and_their_refusals():
    index = pd.date_range("2020-01-01", periods=60, freq="D")
    steps, starts = step_windows([index, index[10:40]], [("2020-01-01", "2020-01-11"), ("2020-01-11", "2020-01-11"),
                                                          ("2020-02-01", "2021-01-01")], 60)
    assert steps.tolist() == [[[0, 10], [10, 10], [31, 60]], [[0, 0], [0, 0], [21, 30]]]
    assert all(list(s) == list(pd.DatetimeIndex(["2020-01-01", "2020-01-11", "2020-02-01"])) for s in starts)
    for bad in ([("2020-01-05", "2020-01-01")], [("2020-01-01", "2020-01-10"), ("2020-01-09", "2020-01-20")],
                [("2020-02-01", "2020-02-05"), ("2020-01-01", "2020-01-05")], []):
        with pytest.raises(ValueError):
            step_windows([index], bad, 60)
    with pytest.raises(ValueError):
        step_windows([index], "MS", 59)


# ------------------------------------------------------------------ the kernels themselves, compiled for the host
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    import ensemble_host_emulation

    return ensemble_host_emulation, ensemble_host_emulation.build(tmp_path_factory.mktemp("ensemble_emulation"))


# widths: one column, several paths per wavefront, more than one block (15 * 36, 3 * 15 * 73 lanes); T: one step, two, an odd length
@pytest.mark.parametrize("T,Wd,S", [(1, 1, 1), (2, 8, 3), (33, 36, 1), (33, 73, 3), (200, 8, 3)])
def test_path_kernel_matches_the_restatement_bit_for_bit(emu, T, Wd, S):
    mod, L = emu
    paths, thr = ref.synthetic_paths(S, 15, T, Wd)
    for win in ref.window_sets(T):
        for th in (None, thr):
            want = ref.path_functionals(paths, win, th)
            for tm in (False, True):
                assert ref.same_bits(mod.path_functionals(L, paths, win, th, tm), want), (win.shape, th is None, tm)


def test_path_kernel_stays_inside_its_arrays_whatever_the_order(emu):
    """Unsorted and overlapping windows with 0 <= a <= b <= T: not the precondition, but every output is written and none of
    them from outside the paths (the poison behind them would show)."""
    mod, L = emu
    T = 33
    paths, thr = ref.synthetic_paths(1, 15, T, 8)
    win = np.tile(np.array([[20, 33], [0, 33], [5, 5], [33, 33], [2, 30]], dtype=np.int64), (3, 1, 1))
    for tm in (False, True):
        got = mod.path_functionals(L, paths, win, thr, tm)
        assert not (got == -777.0).any()
        finite = got[np.isfinite(got[..., 1])]
        assert (finite[:, 1] >= np.nanmin(paths)).all() and (finite[:, 2] <= np.nanmax(paths)).all()


@pytest.mark.parametrize("S", [1, 2, 3, 5, 33, 64, 65, 1000])
def test_summary_kernel_matches_the_restatement(emu, S):
    """Compiled without fused multiply-adds, the host build follows the restatement's roundings: the fixed-order statistics
    are bit-identical and the others inside the GPU tier's bar."""
    mod, L = emu
    values = ref.summary_values(S)
    want, got = ref.ensemble_summary(values, ref.PROBS), mod.ensemble_summary(L, values, ref.PROBS)
    assert ref.same_bits(got[:, [0, 1, 3, 4]], want[:, [0, 1, 3, 4]])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert (np.abs(np.nan_to_num(got - want)) <= ref.summary_bar(values)[:, None]).all()


def test_summary_kernel_at_the_cap_and_beyond(emu):
    mod, L = emu
    cap = L.max_draws()
    assert cap >= 4096
    values = ref.summary_values(cap)[:, [0, 3, 5]]
    want, got = ref.ensemble_summary(values, ref.PROBS), mod.ensemble_summary(L, values, ref.PROBS)
    assert ref.same_bits(got[:, [0, 1, 3, 4]], want[:, [0, 1, 3, 4]])
    assert (np.abs(np.nan_to_num(got - want)) <= ref.summary_bar(values)[:, None]).all()
    out = np.zeros((1, 5))
    assert L.run_ensemble_summary(cap + 1, 1, 0, None, mod.ptr(np.zeros((cap + 1, 1))), mod.ptr(out)) != 0   # refused by the launcher

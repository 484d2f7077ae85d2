"""CPU tier of the time axis (tests/time_axis.py): the constants restated there still read in the kernel source, the groups are
what the axis needs, the inputs of tests/test_time_axis_gpu.py can tell right from wrong -- every tile or pipeline mistake,
restated as an edit of the observations, moves every checked quantity of every record by at least call_forms.FACTOR bars --,
the check functions of the GPU file run over the CPU engine first, and the GPU file's parametrisation holds every length for
every shape, layout and route.  No deliberately broken kernel is built or run: this file is the evidence that the GPU file
would notice one."""
import inspect

import numpy as np
import pytest
import torch

import adjoint_ref
import call_forms as cf
import oracle
import time_axis as ta
from oracle_engine import OracleEngine

ALL_SHAPES = tuple(ta.SHAPES) + ((70, 3),)
GROUPS = [(s, T) for s in ta.SHAPES for T in ta.DENSE_LENGTHS] + [((70, 3), T) for T in ta.GENERIC_LENGTHS]
GROUP_IDS = ["%dx%d-T%d" % (s[0], s[1], T) for s, T in GROUPS]


# ---------------------------------------------------------------------------------------------------------- the source
@pytest.mark.parametrize("entry", ta.SOURCE, ids=[e[0] for e in ta.SOURCE])
def test_constant_reads_in_the_source_as_restated(entry):
    what, fname, text, count = entry
    assert ta.source_lines(fname).count(text) == count, (
        "%s: %r is no longer %d line(s) of %s -- update tests/time_axis.py (and the lengths that follow from it)" % (what, text, count, fname))


@pytest.mark.parametrize("name", sorted(ta.WALKERS))
def test_walker_reads_in_the_source_as_restated(name):
    fname, header, headers, depth, request, requests = ta.WALKERS[name]
    lines = ta.source_lines(fname)
    assert lines.count(header) == headers, (name, header)
    if request is not None:
        assert lines.count(request) == requests, (name, request)
    assert (request is None) == (depth == 0)


def test_lengths_follow_from_the_constants():
    assert ta.DENSE_LENGTHS == (1, 2, 3, 15, 16, 17, 32, 33) == ta.dense_lengths(ta.TS)
    assert ta.dense_lengths(32)[3:] == (31, 32, 33, 64, 65)          # another tile size asks for other lengths
    assert ta.EDGES == (16, 32) and ta.GENERIC_LENGTHS == ta.CPU_LENGTHS == (1, 2, 17)
    assert ta.TSP == ta.PASS == 256
    assert max(w[3] for w in ta.WALKERS.values()) == 2                # T = 3 is the first steady-state iteration


# ----------------------------------------------------------------------------------------------------------- the groups
@pytest.mark.parametrize("shape,T", GROUPS, ids=GROUP_IDS)
def test_groups_are_what_the_axis_needs(shape, T):
    N, K = shape
    g = ta.group(N, K, T)
    assert (g["T"], g["R"], g["S"], g["B"]) == (T, 3, 2 if shape == (70, 3) else 3, 6 if shape == (70, 3) else 9)
    if shape != (70, 3):
        assert all(g["B"] % m for m in (2, 4, 16))
    assert g["patterns"] == ["iid", "first", "steps"]
    assert not ta.edit_conditions(g["obs"]), ta.edit_conditions(g["obs"])
    assert g["phi"].max() < 1.0 - 1e-3 and 0.2 <= (g["obsvar"] == 0).mean() <= 0.8
    for key in ("phi", "q", "x0", "P0"):
        assert len({g[key][i].tobytes() for i in range(g["B"])}) == g["B"], key
    if T in (32, 33):   # an empty step right behind the first tile edge, in record 0 only
        assert [bool(np.isfinite(g["obs"][r, 16]).any()) for r in range(3)] == [False, True, True]
    if T > 1:           # empty steps exist, so the compressed index differs from the time index somewhere in the group
        assert any(not np.isfinite(g["obs"][r]).any(1).all() for r in range(3)) or T < 4


def test_edit_conditions_notice_an_unedited_group():
    g = cf.shared_group(8, 2, 33, 3, 3, 0, patterns=ta.PATTERNS, usable=lambda pat, y, taken: True)
    assert ta.edit_conditions(g["obs"])


# ----------------------------------------------------------------------------------------------------- sensitivity, dense
@pytest.mark.parametrize("shape,T", GROUPS, ids=GROUP_IDS)
def test_every_mistake_is_a_thousand_bars_away(shape, T):
    """Per group and mistake the smallest distance in bars over the records and the checked quantities (printed: run with -s).
    A group that fails gets another seed (time_axis.SEEDS) or another edit, never another factor."""
    g = ta.group(shape[0], shape[1], T)
    applied = 0
    for name in ta.MISTAKES:
        for k in (1, 2):
            apart = ta.sensitivity(g, name, k)
            if apart is None:
                continue
            applied += 1
            worst = min(apart, key=apart.get)
            print("(%d,%d) T = %2d  %-52s k = %d  smallest distance %.3g bars (%s)" % (shape[0], shape[1], T, name, k, apart[worst], worst))
            assert set(apart) == set(cf.quantities(*shape))
            short = {q: d for q, d in apart.items() if not d >= cf.FACTOR}
            assert not short, "%s, k = %d: within %g bars of the right reference in some record: %s" % (name, k, cf.FACTOR, short)
    # short walk always; the clamp from T = 2; the three tile mistakes per edge below T
    assert applied == 1 + (T >= 2) + 3 * sum(b < T for b in ta.EDGES)


# ---------------------------------------------------------------------------------------------------------- the CPU engine
class CpuEngine(OracleEngine):
    """OracleEngine with the calls of BatchedKalman that the dense check functions make and it lacks: loglik_grad and the
    two-phase form from the numpy adjoint, filter_smooth from the C oracle's batch entry point (plain groups only)."""

    def _grad_all(self, phi, q, warmup):
        phi, q = np.asarray(phi, float), np.asarray(q, float)
        rec = self._records(len(phi))
        out = [adjoint_ref.gradient(self.obs_np[r], phi[b], q[b], self.load_np[r], warmup=warmup) for b, r in enumerate(rec)]
        return tuple(torch.from_numpy(np.array([o[j] for o in out])) for j in range(3))

    def loglik_grad(self, phi, q, warmup=1):
        return self._grad_all(phi, q, warmup)

    def loglik_forward(self, phi, q, warmup=1):
        self._point = (phi, q, warmup)
        return self.loglik(phi, q, warmup)

    def loglik_backward(self):
        return self._grad_all(*self._point)[1:]

    def filter_smooth(self, phi, q):
        rec = self._records(len(phi))
        res = oracle.dfm_batch(self.obs_np[rec], np.asarray(phi, float), np.asarray(q, float), self.load_np[rec])
        out = {k: torch.from_numpy(v) for k, v in res.items()}
        out["status"] = torch.zeros(len(phi), dtype=torch.int32)
        return out


class ClampedEngine(CpuEngine):
    """The last row clamped one step short: step T-1 reads row T-2."""

    def set_observations(self, obs):
        obs = np.array(obs, float)
        obs[:, -1] = obs[:, -2]
        return super().set_observations(obs)


@pytest.mark.parametrize("T", ta.CPU_LENGTHS)
@pytest.mark.parametrize("shape", [(8, 2), (13, 4)], ids=["8x2", "13x4"])
def test_checks_pass_on_the_cpu_engine(shape, T):
    """The check functions of tests/test_time_axis_gpu.py are executed before a GPU minute is spent."""
    g = ta.group_plain(shape[0], shape[1], T)
    kf = CpuEngine(g["obs"], g["loadings"])
    ta.check_objective(kf, g)
    ta.check_gradient(kf, g, same_forward=False)
    ta.check_state(kf.filter_smooth(g["phi"], g["q"]), g, "CPU engine")


@pytest.mark.parametrize("T", [2, 17])
def test_checks_fail_on_an_engine_with_a_mistake(T):
    g = ta.group_plain(8, 2, T)
    kf = ClampedEngine(g["obs"], g["loadings"])
    with pytest.raises(AssertionError, match="bars from its reference"):
        ta.check_objective(kf, g)
    with pytest.raises(AssertionError, match="bars from its reference"):
        ta.check_gradient(kf, g, same_forward=False)
    with pytest.raises(AssertionError, match="bars from its reference"):
        ta.check_state(kf.filter_smooth(g["phi"], g["q"]), g, "clamped")


# ------------------------------------------------------------------------------------------------------------ the sparse
def test_every_sparse_pair_is_present():
    have = {(r["T"], len(r["steps"])) for r in map(ta.sparse_record, ta.SPARSE)}
    assert set(ta.SPARSE_PAIRS) <= have and (40, 0) in have and (1, 1) in have
    assert set(ta.SPARSE_PAIRS) == {(256, 255), (256, 256), (257, 257), (513, 256), (600, 512), (600, 513), (300, 257)}
    st = ta.sparse_record("T257_straddle")
    assert list(st["steps"]) == [63, 64, 255, 256] and st["T"] - 1 == 256   # both sides of 63|64 and of 255|256, and the last step
    assert {r["N"] for r in map(ta.sparse_record, ta.SPARSE)} == {5, 8}
    for name in ta.SPARSE:
        r = ta.sparse_record(name)
        assert np.array_equal(np.nonzero(np.isfinite(r["obs"]).any(1))[0], r["steps"])
        assert r["T"] <= 600 and r["phi"].shape == (13, r["N"] + r["K"]) and r["phi"][3, 0] == 0.0


@pytest.mark.parametrize("name", sorted(ta.SPARSE_MISTAKES))
def test_sparse_mistakes_are_a_thousand_bars_away(name):
    applied = 0
    for rname in ta.SPARSE:
        apart = ta.sparse_sensitivity(ta.sparse_record(rname), name)
        if apart is None:
            continue
        applied += 1
        print("%-14s %-46s %s" % (rname, name, "  ".join("%s %.3g" % kv for kv in apart.items())))
        short = {q: d for q, d in apart.items() if not d >= cf.FACTOR}
        assert not short, (rname, name, short)
    # the four records with more than 256 observed steps; a shift needs two entries behind position 256 (the two with 512, 513)
    assert applied == (1 if "straddling" in name else 2 if "shifted" in name else 4)


@pytest.mark.parametrize("name", ["T257_n257", "T257_straddle", "T40_empty", "T1"])
def test_sparse_objective_check_passes_on_the_cpu_engine(name):
    rec = ta.sparse_record(name)
    ta.check_sparse_objective(OracleEngine(rec["obs"][None], rec["loadings"][None]), rec)
    if len(rec["steps"]) > 1:
        y = rec["obs"].copy()
        y[rec["steps"][1]] = np.nan
        with pytest.raises(AssertionError):
            ta.check_sparse_objective(OracleEngine(y[None], rec["loadings"][None]), rec)


# -------------------------------------------------------------------------------------------------------- the coverage
def test_gpu_file_holds_every_length_for_every_shape_layout_and_route():
    import test_time_axis_gpu as gpu

    assert set(ta.SHAPES) == {(8, 2), (5, 1), (13, 4), (32, 4), (33, 4), (60, 4)} and ta.GENERIC_SHAPES == ((8, 2), (70, 3))
    for route, shapes in ta.ROUTES.items():
        fn = getattr(gpu, "test_" + route)
        marks = [m for m in fn.pytestmark if m.name == "parametrize"]
        assert len(marks) == 1 and marks[0].args[0] == "shape,layout", route
        assert list(marks[0].args[1]) == [(s, lay) for s in shapes for lay in ("model_major", "time_major")], route
        assert 'in ta.lengths(shape, "%s")' % route in inspect.getsource(fn), route
        want = ta.GENERIC_LENGTHS if route == "generic_family" else ta.DENSE_LENGTHS
        assert all(ta.lengths(s, route) == want for s in shapes), route
        served = tuple(ta.SHAPES) if route not in ("loo_predict", "generic_family") else shapes
        assert shapes == (served if route != "loo_predict" else tuple(s for s in ta.SHAPES if s != (60, 4))), route
    src = inspect.getsource(gpu)
    for variant in ('"blk"', '"v1"', '"mfma"', '"lane_per_state"', '"split"', '"auto"', '"state"', '"observable"', "packed_sym=True"):
        assert variant in src, variant
    names = inspect.getsource(gpu.test_sparse_objective) + inspect.getsource(gpu.test_sparse_record_filter)
    assert names.count("sorted(ta.SPARSE)") == 2

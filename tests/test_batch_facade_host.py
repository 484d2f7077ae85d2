"""The result cache and the shared tails of ``MetranBatch`` WITHOUT a GPU: over a stand-in engine that answers every cached
kind with tensors of the right shapes (the numbers are the business of the tiers of each accessor family), returns the
workspace and record keys the real engine returns, and logs its calls."""
import numpy as np
import pytest
import torch

from batch_standin import stand_in, two_models
from oracle_engine import OracleEngine

KEEP = {"project": {"sim_means", "sim_vars"}, "smoother": {"S", "var"}, "filter": {"F", "Pf"}, "loo": {"loo_means", "loo_vars"},
        "innov": {"v", "f", "pred_mean", "pred_var"}, "dist": {"r", "ninfo", "q"},
        "forecast": {"fan_mean", "fan_var", "track_mean", "track_var", "skill"}, "weights": {"weights", "intercept"}}
MEMO = {"project": set(), "smoother": {("decomp", False), ("decomp", True)},
        "filter": {("decomp", False), ("decomp", True), ("simf", False), ("simf", True)}}
ALPHA = np.array([[8.0, 6.0, 9.0, 12.0], [5.0, 7.0, 8.0, 10.0]])


class KindsEngine(OracleEngine):
    """Every engine call of the cached kinds: ``calls`` logs (name, whether the scaling was set) per call; each result carries
    what the real one carries beside its outputs (``_work``, record views, ``mle``, ``status``)."""
    status_bits = 0

    def __init__(self, obs=None, loadings=None, adjoint=True, log=None):
        super().__init__(obs, loadings, adjoint, log)
        self.calls, self.scale, self.offset, self._parent = [], None, None, None

    loadings = property(lambda self: torch.from_numpy(self.load_np))
    obs = property(lambda self: torch.from_numpy(self.obs_np))

    def set_scaling(self, scale=None, offset=None):
        self.scale, self.offset = scale, offset
        return self

    def mask_observations(self, mask):
        pass

    def unmask_observations(self):
        pass

    def subset(self, index):
        sub = KindsEngine(self.obs_np[np.asarray(index)], self.load_np[np.asarray(index)])
        sub._parent, sub.status_bits = self, self.status_bits
        return sub

    def _result(self, name, phi, **tails):
        (self._parent or self).calls.append((name, self.scale is not None))
        self.scale = self.offset = None                       # the next call shows whether the facade set it again
        B = phi.shape[0]
        res = {key: phi.sum() + torch.zeros((B,) + tuple(tail), dtype=torch.float64) for key, tail in tails.items()}
        res["_work"] = res["_rec_filt"] = torch.zeros((B, self.T, 3 * self.n * (self.n + 1)))
        res["mle"] = torch.zeros(B)
        res["status"] = torch.full((B,), self.status_bits, dtype=torch.int32)
        return res

    def simulate_smoothed(self, phi, q):
        res = self._result("simulate_smoothed", phi, sim_means=(self.T, self.N), sim_vars=(self.T, self.N))
        res["F"], res["Pf"] = res["_rec_filt"][..., :self.n], res["_rec_filt"][..., self.n:self.n * (self.n + 1)]
        return res

    def smooth_state_variances(self, phi, q):
        return self._result("smooth_state_variances", phi, S=(self.T, self.n), var=(self.T, self.n), F=(self.T, self.n))

    def filter(self, phi, q, outputs=("F", "Pf", "Xp", "Pp")):
        assert tuple(outputs) == ("F", "Pf")
        return self._result("filter", phi, F=(self.T, self.n), Pf=(self.T, self.n, self.n), sigmas=(self.T,))

    def simulate(self, Z, means, covs):
        return torch.einsum("rjn,rtn->rtj", Z, means), torch.einsum("rjn,rtnm,rjm->rtj", Z, covs, Z)

    def decompose(self, Z, means):
        return Z[:, None, :, : self.N].diagonal(dim1=2, dim2=3) * means[..., : self.N], torch.zeros((self.R, self.K, self.T, self.N))

    def loo_predict(self, phi, q):
        return self._result("loo_predict", phi, loo_means=(self.T, self.N), loo_vars=(self.T, self.N))

    def innovations(self, phi, q):
        return self._result("innovations", phi, **{key: (self.T, self.N) for key in ("v", "f", "pred_mean", "pred_var")})

    def disturbances(self, phi, q):
        return self._result("disturbances", phi, r=(self.T, self.n), ninfo=(self.T, self.n))

    def forecast(self, phi, q, horizon=14, outputs=("fan", "skill"), origins=None, track_horizon=1, t_first=1, coverage=0.95):
        tails = {}
        if "fan" in outputs:
            tails.update(fan_mean=(horizon, self.N), fan_var=(horizon, self.N))
        if "track" in outputs:
            tails.update(track_mean=(self.T, self.N), track_var=(self.T, self.N))
        if "skill" in outputs:
            tails.update(skill=(self.N, horizon, 6))
        return self._result("forecast", phi, **tails)

    def observation_weights(self, phi, q, targets, what="series"):
        M = len(targets)
        return self._result("observation_weights", phi, weights=(M, self.T, self.N), intercept=(M,))


# one accessor of every cached kind: kind -> (the facade's call, the engine call it makes, whether that call sets the scaling)
ONE_OF_EACH = {
    "project": (lambda mb, a: mb.get_simulated_means(a), "simulate_smoothed", True),
    "smoother": (lambda mb, a: mb.get_state_means(0, a), "smooth_state_variances", False),
    "filter": (lambda mb, a: mb.get_state_variances(0, a, method="filter"), "filter", False),
    "loo": (lambda mb, a: mb.get_loo_simulated_means(a), "loo_predict", True),
    "innov": (lambda mb, a: mb.get_innovations(a), "innovations", True),
    "dist": (lambda mb, a: mb.get_state_disturbances(a), "disturbances", False),
    "forecast": (lambda mb, a: mb.get_forecast_means(5, a), "forecast", True),
    "weights": (lambda mb, a: mb.get_state_weights(1, 3, [2, 7], a), "observation_weights", False),
}


@pytest.fixture()
def mb():
    return stand_in(KindsEngine, *two_models())


def test_the_table_of_kinds_is_the_one_stated_here():
    from metran_amd.batch import _KINDS

    assert {kind: set(keep) for kind, (_, _, keep) in _KINDS.items()} == KEEP
    assert {kind: scaling for kind, (_, scaling, _) in _KINDS.items()} == {kind: row[2] for kind, row in ONE_OF_EACH.items()}


@pytest.mark.parametrize("kind", list(ONE_OF_EACH))
def test_parameter_set_comparison(mb, kind):
    """The same values in a new tensor (or array) hit; another value or shape misses; None is ``mb.alpha``."""
    call, name, scaling = ONE_OF_EACH[kind]
    call(mb, ALPHA)
    assert mb.kf.calls == [(name, scaling)] and set(mb._cache) == {kind}
    entry = mb._cache[kind][1]
    call(mb, ALPHA.copy()), call(mb, torch.from_numpy(ALPHA.copy())), call(mb, ALPHA.tolist())
    assert len(mb.kf.calls) == 1 and mb._cache[kind][1] is entry                 # a hit returns the same object
    assert torch.equal(mb._cache[kind][0], torch.from_numpy(ALPHA))
    other = ALPHA.copy()
    other[1, 2] = np.nextafter(other[1, 2], np.inf)                              # one value, by one unit in the last place
    call(mb, other)
    assert len(mb.kf.calls) == 2 and mb._cache[kind][1] is not entry
    assert torch.equal(mb._cache[kind][0], torch.from_numpy(other))              # replaced: one parameter set per kind
    call(mb, ALPHA)
    assert len(mb.kf.calls) == 3
    with pytest.raises(ValueError):
        call(mb, ALPHA[:, :3])                                                   # another shape is refused before any comparison
    with pytest.raises(ValueError, match="no parameters"):
        call(mb, None)
    assert len(mb.kf.calls) == 3
    mb.alpha = mb.kf._dev(ALPHA)                                                 # what solve() assigns: fit.alpha
    call(mb, None)
    assert len(mb.kf.calls) == 3                                                 # ... the parameter set already held


def test_a_stored_parameter_set_of_another_shape_is_a_miss(mb):
    """The stored parameter set is compared by shape first: an entry left by another shape is recomputed, not compared."""
    mb.get_innovations(ALPHA)
    mb._cache["innov"] = (torch.zeros((2, 3), dtype=torch.float64), mb._cache["innov"][1])
    mb.get_innovations(ALPHA)
    assert len(mb.kf.calls) == 2 and tuple(mb._cache["innov"][0].shape) == (2, 4)


def test_kinds_hold_their_own_parameter_sets(mb):
    other = ALPHA * 1.01
    mb.get_simulated_means(ALPHA), mb.get_innovations(other)
    before = {kind: entry[1] for kind, entry in mb._cache.items()}
    mb.get_simulated_means(ALPHA), mb.get_innovations(other)
    assert len(mb.kf.calls) == 2
    mb.get_simulated_means(other)                                                # replaces that kind only
    assert mb._cache["project"][1] is not before["project"] and mb._cache["innov"][1] is before["innov"]


@pytest.mark.parametrize("kind", ["forecast", "weights"])
def test_requests_are_kept_per_parameter_set(mb, kind):
    first, second = {"forecast": (lambda a: mb.get_forecast_means(5, a), lambda a: mb.get_prediction_at(0, "s1", 3, a)),
                     "weights": (lambda a: mb.get_state_weights(1, 3, [2, 7], a), lambda a: mb.get_observation_weights(0, "s2", 4, a))}[kind]
    first(ALPHA), second(ALPHA)
    assert len(mb.kf.calls) == 2 and len(mb._cache[kind][1]) == 2
    first(ALPHA), second(ALPHA)
    assert len(mb.kf.calls) == 2                                                 # both requests of the parameter set are held
    second(ALPHA * 1.01)
    assert len(mb.kf.calls) == 3 and len(mb._cache[kind][1]) == 1                # another parameter set drops them all
    first(ALPHA)
    assert len(mb.kf.calls) == 4 and len(mb._cache[kind][1]) == 1


def test_forecast_and_weights_requests_name_every_argument(mb):
    """Two requests that differ in one argument are two entries."""
    for steps, t_first, coverage in ((4, 1, 0.95), (5, 1, 0.95), (5, 2, 0.95), (5, 2, 0.9)):
        mb.forecast_skill(steps, ALPHA, t_first=t_first, coverage=coverage)
    mb.get_prediction_at(0, "s0", 2, ALPHA), mb.get_prediction_at(0, "s0", 3, ALPHA), mb.get_forecast_means(5, ALPHA)
    assert len(mb._cache["forecast"][1]) == 7 == len(mb.kf.calls)
    mb.get_state_weights(0, 1, [2], ALPHA), mb.get_state_weights(1, 1, [2], ALPHA), mb.get_state_weights(1, 2, [2], ALPHA)
    mb.get_state_weights(1, 2, [2, 3], ALPHA), mb.get_observation_weights(1, "s2", [2, 3], ALPHA)
    assert len(mb._cache["weights"][1]) == 5 and len(mb.kf.calls) == 12


@pytest.mark.parametrize("clear", ["solve", "mask_observations", "unmask_observations"])
def test_the_three_places_that_clear_the_cache(mb, clear, monkeypatch):
    import metran_amd.batch as batch_module

    for call, _, _ in ONE_OF_EACH.values():
        call(mb, ALPHA)
    assert set(mb._cache) == set(KEEP) and len(mb.kf.calls) == 8
    if clear == "solve":
        fit = type("Fit", (dict,), {"alpha": mb.kf._dev(ALPHA)})()
        monkeypatch.setattr(batch_module, "calibrate_batch", lambda kf, **kwargs: fit)
        assert mb.solve() is fit and mb.alpha is fit.alpha
    elif clear == "mask_observations":
        mb.mask_observations(torch.zeros((2, mb.T, 3), dtype=torch.uint8))
    else:
        mb.unmask_observations()
    assert mb._cache == {}
    mb.get_simulated_means(ALPHA)
    assert len(mb.kf.calls) == 9


def test_a_cached_entry_holds_its_keep_list_and_nothing_else(mb):
    for call, _, _ in ONE_OF_EACH.values():
        call(mb, ALPHA)
    for standardized in (False, True):                        # everything the accessors derive once and keep beside it
        mb.get_simulated_means(ALPHA, standardized, method="filter")
        for method in ("smoother", "filter"):
            mb.decompose_simulation(0, "s1", ALPHA, standardized, method)
    mb.get_prediction_at(0, "s0", 2, ALPHA), mb.forecast_skill(4, ALPHA)
    assert set(mb._cache) == set(KEEP)
    for kind, (alpha, requests) in mb._cache.items():
        assert isinstance(alpha, torch.Tensor) and requests
        assert all((request is None) == (kind not in ("forecast", "weights")) for request in requests)
        for kept in requests.values():
            assert "_work" not in kept and "status" not in kept
            assert set(kept) <= KEEP[kind] | MEMO.get(kind, set()), (kind, set(kept))
            if kind not in ("forecast",):                     # a forecast holds the outputs of its request
                assert KEEP[kind] <= set(kept)
    assert set.union(*(set(kept) for kept in mb._cache["forecast"][1].values())) == KEEP["forecast"]
    assert set(mb._cache["filter"][1][None]) == KEEP["filter"] | MEMO["filter"]
    assert set(mb._cache["smoother"][1][None]) == KEEP["smoother"] | MEMO["smoother"]
    # a memo entry is computed once
    memo = mb._cache["filter"][1][None][("simf", True)]
    assert mb.get_simulated_variances(ALPHA, True, method="filter") is memo[1]


def test_a_refused_run_leaves_the_held_result(mb):
    from metran_amd._lib import MetranHipError

    mb.get_innovations(ALPHA)
    held = mb._cache["innov"]
    mb.kf.status_bits = 1   # FLAG_NONPOSITIVE_F
    with pytest.raises(MetranHipError, match=r"MetranBatch\(innov\)"):
        mb.get_innovations(ALPHA * 1.01)
    assert mb._cache["innov"] is held
    with pytest.raises(MetranHipError, match=r"MetranBatch\(weights\)"):
        mb.get_state_weights(0, 1, [2], ALPHA)
    assert "weights" not in mb._cache


@pytest.mark.parametrize("shape", [(2, 40, 3), (2, 5, 3), (4, 2, 40, 3)], ids=["RTN", "RHN", "SRTN"])
def test_units(mb, shape):
    """``_units`` against the explicit formula, any number of leading axes; original units pass through untouched."""
    rng = np.random.default_rng(len(shape))
    means, variances = torch.from_numpy(rng.normal(size=shape)), torch.from_numpy(rng.uniform(0.1, 2.0, size=shape))
    std, mean = mb._std.numpy(), mb._mean.numpy()
    m, v = mb._units(means, variances, True)
    at = (None,) * (len(shape) - 3) + (slice(None), None, slice(None))          # [R,N] against [..., R, steps, N]
    np.testing.assert_array_equal(m.numpy(), (means.numpy() - mean[at]) / std[at])
    np.testing.assert_array_equal(v.numpy(), variances.numpy() / (std * std)[at])
    for r in range(2):
        for j in range(3):
            np.testing.assert_array_equal(m.numpy()[..., r, :, j], (means.numpy()[..., r, :, j] - mean[r, j]) / std[r, j])
            np.testing.assert_array_equal(v.numpy()[..., r, :, j], variances.numpy()[..., r, :, j] / (std[r, j] * std[r, j]))
    assert mb._units(means, None, True)[1] is None
    same = mb._units(means, variances, False)
    assert same[0] is means and same[1] is variances


def test_shared_tails(mb):
    import pandas as pd
    from scipy.stats import norm

    for bad in (-1, 4):
        with pytest.raises(IndexError, match="Value of i must be >=0 and <4"):
            mb._check_state(bad)
    mb._check_state(0), mb._check_state(3)
    with pytest.raises(KeyError, match="Unknown name: s9"):
        mb._series(0, "s9")
    mb.shard = (7, 9)                                         # the rows of a sharded batch count from the rank's offset
    index = mb._rows(lambda r: ((name, h) for name in mb.batch.names[r] for h in (1, 2)), ["series", "horizon"])
    assert list(index.names) == ["model", "series", "horizon"]
    assert list(index) == [(r, "s%d" % j, h) for r in (7, 8) for j in range(3) for h in (1, 2)]
    assert list(mb.screen_breaks(ALPHA).index) == [(r, name) for r in (7, 8) for name in ("s0_sdf", "s1_sdf", "s2_sdf", "cdf1")]
    mb.shard = (0, 2)
    # series j of model r up to the model's own length, on its index
    rng = np.random.default_rng(0)
    means, variances = torch.from_numpy(rng.normal(size=(2, 40, 3))), torch.from_numpy(rng.uniform(0.1, 2.0, size=(2, 40, 3)))
    L = int(mb.batch.lengths[1])
    assert L < 40
    frame = mb._series_band(1, 2, means, variances, 0.05)
    assert list(frame.columns) == ["mean", "lower", "upper"] and frame.index.equals(mb.batch.index[1]) and len(frame) == L
    np.testing.assert_array_equal(frame["mean"].values, means.numpy()[1, :L, 2])
    half = norm.ppf(0.975) * np.sqrt(variances.numpy()[1, :L, 2])
    np.testing.assert_array_equal(frame["upper"].values, means.numpy()[1, :L, 2] + half)
    np.testing.assert_array_equal(frame["lower"].values, means.numpy()[1, :L, 2] - half)
    series = mb._series_band(1, 2, means, None, None)         # no band: the variances are not touched
    assert isinstance(series, pd.Series) and series.name == "s2" and series.equals(frame["mean"].rename("s2"))
    with pytest.raises(Exception, match="The value of alpha must be between 0 and 1.") as err:
        mb._series_band(1, 2, means, variances, 1.0)
    assert type(err.value) is Exception


def test_assemble_sets_every_attribute_the_constructor_sets():
    """The seam and ``__init__`` cannot drift apart: ``__init__`` assigns no attribute itself."""
    import ast
    import inspect
    import textwrap

    from metran_amd.batch import MetranBatch

    def assigned(fn):
        tree = ast.parse(textwrap.dedent(inspect.getsource(fn)))
        return {node.attr for node in ast.walk(tree) if isinstance(node, ast.Attribute) and isinstance(node.ctx, ast.Store)
                and isinstance(node.value, ast.Name) and node.value.id == "self"}

    assert assigned(MetranBatch.__init__) == set()
    want = {"kf", "batch", "shard", "alpha", "fit", "factors", "nfactors", "eigval", "fep", "dt", "R", "T", "N", "K", "_std", "_mean",
            "_cache", "n_models_total"}
    assert assigned(MetranBatch._assemble) == want
    mb = stand_in(KindsEngine, *two_models())
    assert want <= set(vars(mb)) and mb.shard == (0, 2) and mb.n_models_total == 2 and mb.dt == 1.0 and mb._cache == {}
    assert (mb.R, mb.T, mb.N, mb.K) == (2, 40, 3, 1) and list(mb.nfactors) == [1, 1] and mb.alpha is None and mb.fit is None

"""CPU tier of the call-form axis (tests/call_forms.py): the inputs of tests/test_call_forms_gpu.py can tell right from wrong.

For every shape and every checked quantity the reference is formed under each WRONG way of pairing instances with records
(or of applying the warm-up); it must be at least 1000 of the GPU test's bars from the right one on some instance of the
group, so that a kernel with that mistake cannot pass.  The check functions of the GPU file then run over the CPU engine
of tests/oracle_engine.py -- right, and with the mistakes built in -- and the degenerate warm-ups are pinned on the reference."""
import types

import numpy as np
import pytest

import adjoint_ref
import call_forms as cf
import oracle_engine
from oracle_engine import OracleEngine

IDS = ["%dx%d" % s for s in cf.SHAPES]
MEANS = ("mle", "F", "S", "sim_means", "gphi", "gq", "loo_means")   # what the initial state mean reaches (no covariance)
OBJECTIVE = ("mle", "gphi", "gq")
W = 2                                                               # the warm-up of the comparisons that do not vary it


def _of_instance(g, key):
    """The group whose ``key`` (x0, P0 or phi) is that of instance i % R instead of i's own."""
    return cf.variant(g, **{key: g[key][np.arange(g["B"]) % g["R"]]})


# name -> (how the wrong reference is formed from (group, i, asked warm-up), the quantities it must move, the warm-ups asked)
WRONG = {
    "record i // S": (lambda g, i, w: cf.reference(g, i, w, record_of=lambda j: j // g["S"]), cf.QUANTITIES, (W,)),
    "record i clamped to R": (lambda g, i, w: cf.reference(g, i, w, record_of=lambda j: min(j, g["R"] - 1)), cf.QUANTITIES, (W,)),
    "record 0": (lambda g, i, w: cf.reference(g, i, w, record_of=lambda j: 0), cf.QUANTITIES, (W,)),
    "x0 of instance i % R": (lambda g, i, w: cf.reference(_wrong_group(g, "x0"), i, w), MEANS, (W,)),
    "P0 of instance i % R": (lambda g, i, w: cf.reference(_wrong_group(g, "P0"), i, w), cf.QUANTITIES, (W,)),
    "phi of instance i % R": (lambda g, i, w: cf.reference(_wrong_group(g, "phi"), i, w), cf.QUANTITIES, (W,)),
    "warm-up weight on the time index": (lambda g, i, w: cf.reference(g, i, w, weight_index="time"), OBJECTIVE, (2, 3)),
    "warm-up 1 whatever was asked": (lambda g, i, w: cf.reference(g, i, 1), OBJECTIVE, cf.GRAD_WARMUPS),
}
_WRONG_GROUPS = {}


def _wrong_group(g, key):
    k = (g["N"], g["K"], key)
    if k not in _WRONG_GROUPS:
        _WRONG_GROUPS[k] = _of_instance(g, key)
    return _WRONG_GROUPS[k]


@pytest.mark.parametrize("name", sorted(WRONG))
@pytest.mark.parametrize("shape", cf.SHAPES, ids=IDS)
def test_wrong_indexing_is_a_thousand_bars_away(shape, name):
    g = cf.group(*shape)
    form, moved, warmups = WRONG[name]
    for w in warmups:
        apart = dict.fromkeys([q for q in cf.quantities(*shape) if q in moved], 0.0)
        for i in range(g["B"]):
            right, wrong = cf.reference(g, i, w), form(g, i, w)
            for q in apart:
                apart[q] = max(apart[q], cf.bars_apart(q, wrong[q], right[q], g, right["rec"]))
        short = {q: d for q, d in apart.items() if not d >= cf.FACTOR}
        assert not short, "%s, warm-up %d: within %g bars of the right reference on every instance: %s" % (name, w, cf.FACTOR, short)


@pytest.mark.parametrize("shape", cf.SHAPES, ids=IDS)
def test_groups_are_what_the_axis_needs(shape):
    """B > R with a partial last wavefront, records that all differ, a "single" record, empty steps ahead of the warm-up, about
    half the observation variances zero, typical persistence, instances that all differ."""
    N, K = shape
    g = cf.group(N, K)
    T, R, S = cf.sizes(N, K)
    assert (g["T"], g["R"], g["S"], g["B"]) == (T, R, S, S * R) and R == 3
    if N + K <= 64:
        assert g["B"] == 15 and all(g["B"] % m for m in (2, 4, 16))
    assert g["patterns"] == ["first", "steps", "single"]
    counts = [int(np.isfinite(g["obs"][r]).any(1).sum()) for r in range(R)]
    assert counts[2] == 1 and len(set(counts)) == R, counts          # sigmacount differs per record
    for r in (0, 1):
        assert not np.isfinite(g["obs"][r]).any(1)[:3].all() and counts[r] >= (4 if T >= 7 else 3)
    for key in ("obs", "loadings", "obsvar", "scale", "offset"):
        for a in range(R):
            for b in range(a + 1, R):
                assert not np.array_equal(g[key][a], g[key][b], equal_nan=True), key
    assert 0.2 <= (g["obsvar"] == 0).mean() <= 0.8
    assert g["phi"].max() < 1.0 - 1e-3 and g["phi"].min() > 0 and g["q"].min() > 0
    assert np.linalg.eigvalsh(g["P0"]).min() > 0
    for key in ("phi", "q", "x0", "P0"):
        assert len({g[key][i].tobytes() for i in range(g["B"])}) == g["B"], key
    dflt = cf.group_defaults(N, K)
    assert dflt["x0"] is None and dflt["P0"] is None and dflt["obs"] is g["obs"] and dflt["phi"] is g["phi"]


@pytest.mark.parametrize("shape", cf.SHAPES, ids=IDS)
def test_degenerate_warmups_on_the_reference(shape):
    """warmup >= sigmacount: the gradient is exactly zero and the objective is nobs(time index >= warmup) * log(2 pi);
    warmup >= T: the objective is 0."""
    g = cf.group(*shape)
    T = g["T"]
    for i in range(g["R"] + 1):                                      # every record once, and one instance of a later set
        sc = cf.reference(g, i, 0, parts=("state",))["sigmacount"]
        seen = np.isfinite(g["obs"][i % g["R"]])
        for w in sorted({sc, sc + 1, T, T + 1} | ({2} if g["patterns"][i % g["R"]] == "single" else set())):
            ref = cf.reference(g, i, w, parts=("state", "grad"))
            assert ref["mle"] == int(seen[w:].sum()) * np.log(2.0 * np.pi), (i, w)
            if w >= T:
                assert ref["mle"] == 0.0
            if "gphi" in ref:
                assert ref["gmle"] == ref["mle"] and not ref["gphi"].any() and not ref["gq"].any(), (i, w)
        if sc > 1:                                                   # ... and one step short of it neither is
            ref = cf.reference(g, i, sc - 1, parts=("state", "grad"))
            assert ref["mle"] != int(seen[sc - 1:].sum()) * np.log(2.0 * np.pi)
            assert "gphi" not in ref or (ref["gphi"].any() and ref["gq"].any())


def _oracle_checks(kf, g):
    """The objective and gradient checks of tests/test_call_forms_gpu.py that the CPU engine can serve."""
    cf.check_objective(kf, g, cf.loglik_warmups(g["T"]))
    cf.check_position_independent(lambda gg: {"mle": kf.loglik(gg["phi"], gg["q"], warmup=2)}, g, "loglik")
    if not cf.has_gradient(g["N"], g["K"]):
        return
    cf.check_gradient_alpha(kf, g, dt=0.5, warmup=2)
    alpha, _ = cf.alpha_group(g, 0.5)
    cf.check_two_phase(lambda a: kf.loglik_forward_alpha(a, dt=0.5, warmup=2), kf.loglik_backward_alpha,
                       lambda a: kf.loglik_grad_alpha(a, dt=0.5, warmup=2), alpha, alpha * 1.3, "two-phase", same_forward=False)

    def grad(gg):
        mle, ga = kf.loglik_grad_alpha(cf.alpha_group(gg, 0.5)[0], dt=0.5, warmup=2)
        return {"mle": mle, "galpha": ga}

    cf.check_position_independent(grad, g, "loglik_grad_alpha")


@pytest.mark.parametrize("shape", cf.SHAPES, ids=IDS)
def test_checks_pass_on_the_oracle_engine(shape):
    """OracleEngine maps instance to record as np.arange(B) % R: the check functions are exercised before a GPU minute is spent."""
    g = cf.group_plain(*shape)
    _oracle_checks(OracleEngine(g["obs"], g["loadings"]), g)


class _RecordOfTheGroupsFirstModel(OracleEngine):
    """Four models to a wavefront (the narrow kernels), all reading the record of the first."""
    per_wave = 4

    def _records(self, B):
        return (np.arange(B) // self.per_wave * self.per_wave) % self.R


class _RecordOfThePairsFirstModel(_RecordOfTheGroupsFirstModel):
    """Two models to a wavefront (the split layout with H = 32)."""
    per_wave = 2


class _RecordByInstance(OracleEngine):
    def _records(self, B):
        return np.minimum(np.arange(B), self.R - 1)


def test_checks_fail_on_a_mutated_engine(monkeypatch):
    """The same checks over an engine with each mistake built in: the record of a wavefront's first model for all four of
    it (and for both of a pair), the record taken by instance, and the adjoint's warm-up weight on the time index."""
    g = cf.group_plain(8, 2)
    for cls in (_RecordOfTheGroupsFirstModel, _RecordOfThePairsFirstModel, _RecordByInstance):
        kf = cls(g["obs"], g["loadings"])
        with pytest.raises(AssertionError, match="bars from its reference"):
            cf.check_objective(kf, g, cf.loglik_warmups(g["T"]))
        with pytest.raises(AssertionError, match="of its bound|bars from its reference"):
            cf.check_gradient_alpha(kf, g, dt=0.5, warmup=2)
    with pytest.raises(AssertionError, match="depends on their position"):
        kf = _RecordOfTheGroupsFirstModel(g["obs"], g["loadings"])
        cf.check_position_independent(lambda gg: {"mle": kf.loglik(gg["phi"], gg["q"], warmup=2)}, g, "loglik")

    def on_the_time_index(*a, **kw):
        return adjoint_ref.gradient(*a, weight_index="time", **kw)

    monkeypatch.setattr(oracle_engine, "adjoint_ref", types.SimpleNamespace(gradient=on_the_time_index))
    kf = OracleEngine(g["obs"], g["loadings"])
    cf.check_objective(kf, g, cf.loglik_warmups(g["T"]))             # the objective does not go through the adjoint
    with pytest.raises(AssertionError, match="of its bound|bars from its reference"):
        cf.check_gradient_alpha(kf, g, dt=0.5, warmup=2)

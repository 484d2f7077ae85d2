"""CPU tier of the status axis (tests/status_cases.py): the inputs keep every expected bit away from rounding, the longdouble
restatement that the expectations come from is pinned to the C oracle, the oracle's objective is not finite for every invalid
instance, the check functions of tests/test_status_gpu.py pass over a CPU engine and FAIL on three built-in mistakes (flags
written at inst % R, flags OR-ed over each aligned group of four instances, an objective that takes log |prod f|), and the GPU
file's parametrisation holds every shape, layout and case.  No deliberately broken kernel is built or run."""
import inspect

import numpy as np
import pytest
import torch

import call_forms as cf
import status_cases as sc
from oracle_engine import OracleEngine
from test_hip_parity import FILT_ATOL, MLE_RTOL

ALL_SHAPES = tuple(dict.fromkeys(sc.SHAPES + sc.GENERIC_SHAPES))
SHAPE_IDS = ["%dx%d" % s for s in ALL_SHAPES]
CPU_SHAPES = ((8, 2), (13, 4))


def test_flags_are_the_headers():
    src = open(sc.cf.__file__.replace("tests/call_forms.py", "include/metran_hip.h")).read()
    for name, bit in (("NONPOSITIVE_F", sc.FLAG_NONPOSITIVE_F), ("NOT_SPD", sc.FLAG_NOT_SPD), ("RANK_DEFICIENT", sc.FLAG_RANK_DEFICIENT)):
        assert "#define MK_FLAG_%s %du" % (name, bit) in src


# ------------------------------------------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
def test_groups_share_wavefronts(shape):
    g = sc.base(*shape)
    assert (g["T"], g["R"]) == (9, 3) and g["B"] == (6 if shape == (70, 3) else 9)
    if shape != (70, 3):
        assert g["B"] % 4 == 1                      # four models per wavefront: the last one holds a single live model
    for name in sc.CASES:
        c = sc.case(shape[0], shape[1], name)
        quads = {i // 4 for i in c["touched"]}
        assert any(i // 4 in quads for i in range(g["B"]) if i not in c["touched"]), name   # a clean neighbour in the wavefront
        if name == "nan_phi":
            assert g["B"] - 1 in c["touched"]       # the tail wavefront
        for k in ("phi", "q", "x0", "P0"):          # the twin differs in the touched instances only
            same = [np.array_equal(c["bad"][k][i], c["twin"][k][i], equal_nan=True) for i in range(g["B"])]
            assert all(s or i in c["touched"] for i, s in enumerate(same)), (name, k)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
def test_record_cases_observe_the_bad_series_where_they_say(shape):
    for name in sc.RECORD_CASES:
        c = sc.case(shape[0], shape[1], name)
        y = c["bad"]["obs"][sc.BAD_RECORD]
        assert np.array_equal(y, c["twin"]["obs"][sc.BAD_RECORD], equal_nan=True)
        seen = np.isfinite(y)
        steps = [sc.STEP_A] if name == "neg_once" else [sc.STEP_A, sc.STEP_B]
        series = [0, 1] if name == "neg_twice_within" else [0]
        for j in series:
            assert list(np.nonzero(seen[:, j])[0]) == steps, name
            assert c["bad"]["obsvar"][sc.BAD_RECORD, j] == sc.BAD_OBSVAR and c["twin"]["obsvar"][sc.BAD_RECORD, j] > 0
        compressed = np.cumsum(seen.any(1)) - 1
        assert all(compressed[t] >= max(sc.WARMUPS) for t in steps), name      # behind the warm-up, in the compressed index
        assert c["touched"] == tuple(i for i in range(c["bad"]["B"]) if i % 3 == 1)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
def test_no_expected_bit_depends_on_rounding(shape):
    """|f| >= 1e-3 or exactly 0 (zero_f: every f of a touched instance); clean pivots >= 1e-6; the intended zero pivot exactly
    0; and the expected bits are the ones the case is about."""
    N, K = shape
    for name in sc.CASES:
        c = sc.case(N, K, name)
        for grp, bad in ((c["bad"], True), (c["twin"], False)):
            for i in range(grp["B"]):
                rs = sc.restate(grp, i)
                f, piv = np.array(rs["f"]), rs["pivots"]
                invalid = bad and i in c["touched"]
                if invalid and name == "zero_f":
                    assert f[0] == 0.0 and not (f[np.isfinite(f)] != 0.0).any(), (name, i)
                elif invalid and name == "nan_phi":
                    assert np.isnan(f).any() and (np.abs(f[np.isfinite(f)]) >= sc.F_MARGIN).all(), (name, i)
                else:
                    assert np.isfinite(f).all() and (np.abs(f) >= sc.F_MARGIN).all(), (name, i, np.abs(f).min())
                if invalid and name in sc.RECORD_CASES:
                    neg = f < 0
                    assert neg.sum() == (1 if name == "neg_once" else 2 if name == "neg_twice_across" else 4), (name, i)
                    assert (piv >= sc.PIVOT_MARGIN).all(), (name, i)      # Pf = P + d d' / |f| stays positive definite
                elif invalid and name == "zero_factor":
                    assert (piv[:, N] == 0.0).all() and (np.delete(piv, N, 1) >= sc.PIVOT_MARGIN).all(), (name, i)
                elif not invalid:
                    assert (piv >= sc.PIVOT_MARGIN).all(), (name, i, piv.min())
        want = {"zero_factor": (0, sc.FLAG_RANK_DEFICIENT)}.get(name)
        for i, (fb, sb) in enumerate(sc.expected_status(c["bad"], "rts")):
            if i not in c["touched"]:
                assert (fb, sb) == (0, 0)
            elif want:
                assert (fb, sb) == want
            else:
                assert fb == sc.FLAG_NONPOSITIVE_F and sb in ((0,) if name in sc.RECORD_CASES else (0, sc.FLAG_RANK_DEFICIENT))
        assert all(e == (0, 0) for e in sc.expected_status(c["twin"], "rts")), name


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
def test_indefinite_moments_have_a_clearly_negative_pivot(shape):
    g, touched = sc.indefinite_group(*shape)
    n = shape[0] + shape[1]
    for i in touched:
        piv = np.diag(-np.diag(g["phi"][i] ** 2) + np.diag(g["q"][i]))
        assert (piv <= sc.NEGATIVE_PIVOT).all() and sc.pivot_bits(piv) == sc.FLAG_NOT_SPD | sc.FLAG_RANK_DEFICIENT
    F, Pf, Xp, Pp = sc.indefinite_moments(g, touched, np.zeros((g["B"], 9, n)), np.tile(np.eye(n), (g["B"], 9, 1, 1)), np.zeros((g["B"], 9, n)),
                                          np.tile(np.eye(n), (g["B"], 9, 1, 1)))
    assert all(np.array_equal(Pf[i, 6], -np.eye(n)) and (np.diag(Pp[i, 7]) <= sc.NEGATIVE_PIVOT).all() for i in touched)
    assert all(np.array_equal(Pf[i], np.tile(np.eye(n), (9, 1, 1))) for i in range(g["B"]) if i not in touched)


# ------------------------------------------------------------------------------------------- the restatement and the oracle
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
def test_restatement_is_the_oracles_filter(shape):
    """Clean instances: filtered moments within FILT_ATOL and the objective within MLE_RTOL of the C oracle at both warm-ups;
    every instance: isfinite(mle) agrees -- the oracle's objective of every invalid instance is NOT finite."""
    for name in sc.CASES:
        c = sc.case(shape[0], shape[1], name)
        g = c["bad"]
        for i in range(g["B"]):
            rs = sc.restate(g, i)
            for w in sc.WARMUPS:
                ref = cf.reference(g, i, w, parts=("state",))
                assert np.isfinite(ref["mle"]) == np.isfinite(rs["mle"][w]), (name, i, w)
                invalid = i in c["touched"] and name != "zero_factor"
                assert np.isfinite(ref["mle"]) != invalid, (name, i, w, ref["mle"])
                if not invalid:
                    assert abs(rs["mle"][w] - ref["mle"]) <= MLE_RTOL * max(1.0, abs(ref["mle"])), (name, i, w)
            if i not in c["touched"]:
                assert np.abs(rs["F"] - ref["F"]).max() <= FILT_ATOL and np.abs(rs["Pf"] - ref["Pf"]).max() <= FILT_ATOL, (name, i)


# --------------------------------------------------------------------------------------------------------- the CPU engine
class StatusEngine(OracleEngine):
    """OracleEngine on a whole group (observation variances and initial moments included): ``loglik`` and ``filter_smooth``
    from the C oracle instance by instance (``call_forms.reference``), ``status`` from the restatement."""

    def __init__(self, g):
        super().__init__(g["obs"], g["loadings"])
        self.g = g

    def _group(self, phi, q, x0, P0):
        return cf.variant(self.g, phi=np.asarray(phi), q=np.asarray(q), x0=x0, P0=P0, B=len(phi))

    def _mle(self, g, i, warmup):
        return cf.reference(g, i, warmup, parts=("state",))["mle"]

    def _status(self, st):
        return st

    def loglik(self, phi, q, warmup=1, x0=None, P0=None):
        g = self._group(phi, q, x0, P0)
        return torch.tensor([self._mle(g, i, warmup) for i in range(g["B"])], dtype=torch.float64)

    def filter_smooth(self, phi, q, warmup=1, x0=None, P0=None):
        g = self._group(phi, q, x0, P0)
        refs = [cf.reference(g, i, warmup, parts=("state",)) for i in range(g["B"])]
        out = {k: torch.from_numpy(np.stack([r[k] for r in refs])) for k in ("F", "Pf", "Xp", "Pp", "S", "Ps")}
        out["mle"] = torch.tensor([self._mle(g, i, warmup) for i in range(g["B"])], dtype=torch.float64)
        st = [fb | sb for fb, sb in sc.expected_status(g, "rts")]
        out["status"] = torch.tensor(self._status(st), dtype=torch.int32)
        return out


class WrongIndexEngine(StatusEngine):
    """Flags written at inst % R instead of inst."""

    def _status(self, st):
        out = [0] * len(st)
        for i, s in enumerate(st):
            out[i % self.R] |= s
        return out


class WavefrontEngine(StatusEngine):
    """Flags OR-ed over each aligned group of four instances."""

    def _status(self, st):
        return [int(np.bitwise_or.reduce(st[i // 4 * 4:i // 4 * 4 + 4])) for i in range(len(st))]


class AbsoluteProductEngine(StatusEngine):
    """An objective that takes log |prod f|: finite for every instance with negative innovation variances."""

    def _mle(self, g, i, warmup):
        ref = cf.reference(g, i, warmup, parts=("state",))
        if np.isfinite(ref["mle"]):
            return ref["mle"]
        y, f = g["obs"][i % g["R"]], iter(sc.restate(g, i)["f"])
        steps = [[next(f) for _ in range(int(m.sum()))] for m in np.isfinite(y) if m.any()]
        with np.errstate(all="ignore"):
            det = sum(np.log(abs(np.prod(s))) for s in steps[warmup:])
        sig = np.nansum(ref["sigmas"][warmup:ref["sigmacount"]])
        return float(np.log(2 * np.pi) * np.isfinite(y[warmup:]).sum() + det + sig)


def _run(engine, c, checks=("flags", "containment", "clean", "objective")):
    bad, twin = engine(c["bad"]), engine(c["twin"])
    a = bad.filter_smooth(c["bad"]["phi"], c["bad"]["q"], **cf.init(c["bad"]))
    b = twin.filter_smooth(c["twin"]["phi"], c["twin"]["q"], **cf.init(c["twin"]))
    if "flags" in checks:
        sc.check_flags(a["status"], c, "rts", "CPU engine")
        sc.check_twin_flags(b["status"], c, "rts", "CPU engine")
    if "containment" in checks:
        sc.check_containment(a, b, c, "CPU engine")
    if "clean" in checks:
        sc.check_clean(a, c, "CPU engine")
    if "objective" in checks:
        for w in sc.WARMUPS:
            sc.check_objective(bad.loglik(c["bad"]["phi"], c["bad"]["q"], warmup=w, **cf.init(c["bad"])), c, w, "CPU engine")


@pytest.mark.parametrize("name", sc.CASES)
@pytest.mark.parametrize("shape", CPU_SHAPES, ids=["8x2", "13x4"])
def test_checks_pass_on_the_cpu_engine(shape, name):
    _run(StatusEngine, sc.case(shape[0], shape[1], name))


@pytest.mark.parametrize("name", sc.CASES)
def test_checks_fail_on_flags_written_at_the_record_index(name):
    with pytest.raises(AssertionError, match="has status"):
        _run(WrongIndexEngine, sc.case(8, 2, name), ("flags",))


@pytest.mark.parametrize("name", sc.CASES)
def test_checks_fail_on_flags_shared_by_a_wavefront(name):
    with pytest.raises(AssertionError, match="has status"):
        _run(WavefrontEngine, sc.case(8, 2, name), ("flags",))


@pytest.mark.parametrize("name", sc.RECORD_CASES)
def test_checks_fail_on_the_objective_of_an_absolute_product(name):
    c = sc.case(8, 2, name)
    kf = AbsoluteProductEngine(c["bad"])
    got = kf.loglik(c["bad"]["phi"], c["bad"]["q"], warmup=1, **cf.init(c["bad"]))
    assert np.isfinite(got.numpy()).all()
    with pytest.raises(AssertionError, match="returned the finite"):
        sc.check_objective(got, c, 1, "absolute product")


def test_containment_check_notices_one_bit():
    c = sc.case(8, 2, "neg_once")
    a = {"F": np.zeros((9, 9, 10)), "status": np.zeros(9)}
    b = {"F": np.zeros((9, 9, 10)), "status": np.zeros(9)}
    b["F"][1] = 1.0                                     # a touched instance may differ
    sc.check_containment(a, b, c, "self-test")
    b["F"][8, 8, 9] = -0.0                              # a clean one may not, not even in the sign of a zero
    with pytest.raises(AssertionError, match="depends on the invalid ones"):
        sc.check_containment(a, b, c, "self-test")


# ----------------------------------------------------------------------------------------------------------- the coverage
def test_gpu_file_holds_every_shape_layout_and_case():
    import test_status_gpu as gpu

    assert sc.SHAPES == ((8, 2), (13, 4), (32, 4), (33, 4), (60, 4)) and sc.GENERIC_SHAPES == ((8, 2), (70, 3))
    assert sc.CASES == ("neg_once", "neg_twice_across", "neg_twice_within", "zero_f", "nan_phi", "zero_factor")
    for fn, shapes in gpu.ROUTE_TESTS.items():
        marks = [m for m in getattr(gpu, fn).pytestmark if m.name == "parametrize"]
        assert len(marks) == 1 and marks[0].args[0] == "shape,layout", fn
        assert list(marks[0].args[1]) == [(s, lay) for s in shapes for lay in sc.LAYOUTS], fn
        src = inspect.getsource(getattr(gpu, fn))
        assert "sc.CASES" in src or "sc.INSTANCE_CASES" in src or "sc.RECORD_CASES" in src or "indefinite" in src, fn
    no_loo = tuple(s for s in sc.SHAPES if s != (60, 4))   # a full wavefront has no leave-one-out walk: its own test says so
    assert all(shapes == (sc.GENERIC_SHAPES if "generic" in fn else ((8, 2),) if "sparse" in fn else no_loo if "loo" in fn else sc.SHAPES)
               for fn, shapes in gpu.ROUTE_TESTS.items())
    assert "test_no_leave_one_out_for_a_full_wavefront" in dir(gpu) and "simulate_unconditional" in inspect.getsource(gpu)
    src = inspect.getsource(gpu)
    for variant in ('"blk"', '"record"', '"v1"', '"mfma"', '"mfma_unfolded"', '"lane_per_state"', '"split"', '"state"', '"observable"', "packed_sym=True",
                    "0xA5A5A5A5", "mk_loglik_grad", "mk_smooth_dense", "mk_smooth", "mk_loo", "mk_filter_smooth", "mk_filter"):
        assert variant in src, variant

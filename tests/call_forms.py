"""Inputs, references and check functions of the CALL-FORM axis (test infrastructure; no GPU, no test functions): batched
calls with more instances than records (B = S * R: instance ``s * R + r`` reads record ``r``) and a warm-up other than 1.

Every batched call has two indices.  An INSTANCE i has its own phi, q, x0, P0 and its own outputs; its RECORD i % R has its
own observations, loadings, observation variances, scale and offset.  With B == R the two coincide and a kernel that mixes
them up passes every comparison, so a group here has

  records     R = 3, all different: drawn with hard_models.draw_model (typical persistence only, redrawn until
              phi.max() < 1 - 1e-3, so the tier's flat bars apply without the conditioning term), with the missingness
              patterns "first", "steps", "single" (, "iid") in turn -- empty steps make the compressed index of observed
              steps differ from the time index, sigmacount differs per record, and the "single" record has sigmacount 1;
              observation variances with about half the series at zero; a scale and an offset per record
  instances   S = 5 parameter sets per record (B = 15: odd, no multiple of the 2, 4 or 16 models the kernels pack per
              wavefront or block): phi and q a perturbation of a few percent of the record's, an x0 and an SPD P0 each
  lengths     T = 9 for n <= 16, T = 7 above; (70,3) -- size-generic kernels only -- has S = 2 (B = 6) and T = 5

tests/test_call_forms.py shows, without a GPU, that every wrong way of pairing the two indices moves every checked quantity
by at least 1000 bars; tests/test_call_forms_gpu.py runs the kernels.  Both use the check functions below, so the checks
themselves run on the CPU (over tests/oracle_engine.py) before a GPU minute is spent.

Bars -- the tier's existing ones, none new:
  mle                    MLE_RTOL (tests/test_hip_parity.py), relative to max(1, |mle|) as hard_models.mle_tolerance has it
  F, Pf, Xp, Pp          FILT_ATOL (tests/test_hip_parity.py)
  S, Ps, state variances SMOOTH_ATOL (tests/test_hip_parity.py)
  sigmas, detfs          rtol 1e-9 + atol 1e-10, atol 1e-10 (tests/test_shape_matrix_gpu.py::_check_filter, the flat part)
  sim_means, sim_vars    2 * SMOOTH_ATOL * max(scale)^2 (tests/test_shape_matrix_gpu.py, projection test, the flat part)
  gphi, gq               rtol 1e-9, atol 1e-9 * max |g| (tests/test_adjoint.py)
  loo means / variances  1e-12 * max(1, largest modulus) against loo_ref.loo_tape (tests/test_loo_gpu.py)
  galpha                 helper_ref.galpha_bound (16 eps of the moduli of its two terms) plus the gradient's bar carried
                         through the chain rule, (bar(gphi) + |2 phi c| bar(gq)) * phi dt / alpha^2: the kernel is handed
                         the device's gphi and gq, which are only that close to the reference's
"""
import functools

import numpy as np

import adjoint_ref
import hard_models
import helper_ref
import loo_ref
import oracle
from metran_amd.params import phi_q_from_alpha
from test_hip_parity import FILT_ATOL, MLE_RTOL, SMOOTH_ATOL

GRAD_RTOL = 1e-9          # tests/test_adjoint.py: rtol = 1e-9, atol = 1e-9 * max |g|
LOO_TOL = 1e-12           # tests/test_loo_gpu.py
SIGMA_RTOL, SIGMA_ATOL, DETF_ATOL = 1e-9, 1e-10, 1e-10   # tests/test_shape_matrix_gpu.py::_check_filter
DRAW_TOL = 1e-9           # tests/test_draws_gpu.py: TOL
FACTOR = 1000.0           # a wrong pairing of the indices moves every quantity by at least this many bars

# one shape per kernel that owns a ``rec`` (all prebuilt: tests/shape_matrix.py MATRIX; (70,3) has no specialised kernels)
SHAPES = ((8, 2), (12, 4), (13, 4), (32, 4), (33, 4), (60, 4), (70, 3))
GENERIC_SHAPES = ((8, 2), (32, 4), (70, 3))   # the size-generic family: 64, 256 and 1024 threads
RECORDS = 3
MISSINGNESS = ("first", "steps", "single", "iid")
GRAD_WARMUPS = (0, 2, 3)
SEEDS = {}                # shape -> seed, where the default draw (0) does not separate right from wrong by FACTOR bars

QUANTITIES = ("mle", "F", "Pf", "S", "Ps", "sim_means", "sim_vars", "gphi", "gq", "loo_means", "loo_vars")


def sizes(N, K):
    """(T, R, S) of the shape's group."""
    if N + K > 64:
        return 5, RECORDS, 2
    return (9 if N + K <= 16 else 7), RECORDS, 5


def loglik_warmups(T):
    return (0, 1, 2, 3, T + 1)


def has_gradient(N, K):
    return N + K <= 64


def has_loo(N, K):
    return N + K <= 63


def quantities(N, K):
    return tuple(k for k in QUANTITIES if (has_gradient(N, K) or k not in ("gphi", "gq")) and (has_loo(N, K) or not k.startswith("loo")))


# ------------------------------------------------------------------------------------------------------------------ inputs
def _usable(pattern, y, taken):
    """A record serves the warm-up checks when its number of observed steps is not one of ``taken`` (the earlier records':
    sigmacount differs per record), its compressed and time indices disagree before the third observed step and, except for
    "single", observed steps are left behind a warm-up of 3 (of 2 for the shortest group, which has no gradient)."""
    seen = np.isfinite(y).any(1)
    if seen.sum() in taken:
        return False
    if pattern == "single":
        return seen.sum() == 1
    if seen.sum() < (4 if len(seen) >= 7 else 3):
        return False
    return pattern == "iid" or not seen[:3].all()


def variant(g, **kw):
    """The group with some entries replaced (and its own cache of references)."""
    out = dict(g, **kw)
    out["_cache"] = {}
    return out


def shared_group(N, K, T, R, S, seed, patterns=MISSINGNESS, usable=_usable):
    """R records and B = S * R instances in the library's order (instance s * R + r reads record r).  dict: obs [R,T,N],
    loadings [R,N,K], obsvar / scale / offset [R,N], patterns [R]; phi / q / x0 [B,n], P0 [B,n,n]; N, K, T, R, S, B.
    ``patterns`` / ``usable``: the missingness patterns taken in turn and the condition a drawn record is redrawn until it
    meets (tests/time_axis.py has its own: it edits the records afterwards).  MILD by construction: a record is redrawn until
    every persistence is below 1 - 1e-3, so that flat bars apply; the hard models (tests/hard_models.py) go through the routes
    that use these groups in tests/test_gpu_property*.py."""
    rng = np.random.default_rng([int(seed), N, K, T, R, S])
    n, B = N + K, S * R
    g = dict(N=N, K=K, T=T, R=R, S=S, B=B, obs=np.empty((R, T, N)), loadings=np.empty((R, N, K)), patterns=[])
    rphi, rq = np.empty((R, n)), np.empty((R, n))
    for r in range(R):
        pat = patterns[r % len(patterns)]
        while True:
            y, phi, q, load = hard_models.draw_model(rng, N, K, T, pat)
            if phi.max() < 1.0 - 1e-3 and usable(pat, y, [int(np.isfinite(o).any(1).sum()) for o in g["obs"][:r]]):
                break
        g["obs"][r], rphi[r], rq[r], g["loadings"][r] = y, phi, q, load
        g["patterns"].append(pat)
    g["obsvar"] = rng.uniform(0.05, 0.5, (R, N)) * (rng.random((R, N)) < 0.5)
    g["scale"], g["offset"] = rng.uniform(0.5, 2.0, (R, N)), rng.normal(size=(R, N))
    rec = np.arange(B) % R
    z = rng.standard_normal((B, n))
    g["phi"] = np.where(rphi[rec] * (1.0 + 0.03 * z) < 1.0 - 1e-3, rphi[rec] * (1.0 + 0.03 * z), rphi[rec] * (1.0 - 0.03 * np.abs(z)))
    g["q"] = rq[rec] * (1.0 + 0.03 * rng.standard_normal((B, n)))
    g["x0"] = rng.normal(size=(B, n))
    A = rng.normal(size=(B, n, n))
    g["P0"] = A @ A.transpose(0, 2, 1) / n + 0.5 * np.eye(n)
    for v in g.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return variant(g)


@functools.lru_cache(maxsize=None)
def group(N, K):
    """The shape's group, drawn once and shared (read-only) by everything that needs it."""
    T, R, S = sizes(N, K)
    return shared_group(N, K, T, R, S, SEEDS.get((N, K), 0))


@functools.lru_cache(maxsize=None)
def group_defaults(N, K):
    """The same records and parameter sets started from the default moments (x0 = P0 = None)."""
    return variant(group(N, K), x0=None, P0=None)


@functools.lru_cache(maxsize=None)
def group_without_obsvar(N, K):
    """The group without observation variances (Metran's own case, the one the state tape serves)."""
    return variant(group(N, K), obsvar=None)


@functools.lru_cache(maxsize=None)
def group_plain(N, K):
    """... and without observation variances or scaling: what tests/oracle_engine.py::OracleEngine serves."""
    return variant(group(N, K), x0=None, P0=None, obsvar=None, scale=None, offset=None)


def take(g, sl):
    """The instances ``sl`` (a slice holding whole parameter sets) of a group, on the same records."""
    return variant(g, B=len(g["phi"][sl]), **{k: (None if g[k] is None else g[k][sl]) for k in ("phi", "q", "x0", "P0")})


def init(g):
    """The initial-moment keywords of a call on the group."""
    return {} if g["x0"] is None else dict(x0=g["x0"], P0=g["P0"])


def alpha_group(g, dt):
    """(alpha [B,n], the group whose phi and q are Metran's map of alpha at step dt, from the default moments): the inputs of
    loglik_grad_alpha, which takes neither x0 nor P0.  alpha = -1 / log(phi): every instance keeps a point of its own."""
    alpha = -1.0 / np.log(g["phi"])
    phi, q = phi_q_from_alpha(alpha, g["loadings"][np.arange(g["B"]) % g["R"]], dt)
    return alpha, variant(g, phi=phi, q=q, x0=None, P0=None)


# -------------------------------------------------------------------------------------------------------------- references
def _opt(g, key, r):
    return None if g[key] is None else g[key][r]


def reference(g, i, warmup, record_of=None, weight_index="compressed", parts=("state", "grad", "loo")):
    """Everything the tier checks, for instance i of a group, from plain restatements:
      state   the oracle's filter and smoother (sigmas, detfs, sigmacount, F, Pf, Xp, Pp, S, Ps), ``mle`` =
              oracle.get_mle(..., warmup), and the projection with the record's scale and offset (sim_means, sim_vars)
      grad    adjoint_ref.gradient(..., warmup=warmup): gmle, gphi, gq (shapes with a gradient)
      loo     loo_ref.loo_tape in the record's units: loo_means, loo_vars (shapes with leave-one-out predictions)
    ``record_of`` (default i % R) and ``weight_index`` exist only so that tests/test_call_forms.py can form deliberately WRONG
    references.  Results are kept with the group."""
    N, K, R = g["N"], g["K"], g["R"]
    n = N + K
    r = int(i % R if record_of is None else record_of(i))
    y, G, Rv = g["obs"][r], g["loadings"][r], _opt(g, "obsvar", r)
    phi, q, x0, P0 = g["phi"][i], g["q"][i], _opt(g, "x0", i), _opt(g, "P0", i)
    cache = g["_cache"]
    out = dict(rec=r)
    if "state" in parts:
        key = ("state", i, r)
        if key not in cache:
            Z = np.concatenate([np.eye(N), G], axis=1)
            o, oi, oc = oracle.set_observations(y)
            sg, df, sc, F, Pf, Xp, Pp = oracle.seqkalmanfilter(o, np.diag(phi), np.diag(q), Z, np.zeros(N) if Rv is None else Rv, oi, oc,
                                                               np.zeros(n) if x0 is None else x0, np.eye(n) if P0 is None else P0)
            S, Ps = oracle.kalmansmoother(F, Pf, Xp, Pp, np.diag(phi))
            scale = np.ones(N) if g["scale"] is None else g["scale"][r]
            offset = np.zeros(N) if g["offset"] is None else g["offset"][r]
            Zs = Z * scale[:, None]
            cache[key] = dict(sigmas=sg, detfs=df, sigmacount=sc, F=F, Pf=Pf, Xp=Xp, Pp=Pp, S=S, Ps=Ps, Z=Z, oc=oc,
                              sim_means=S @ Zs.T + offset, sim_vars=np.maximum(np.einsum("jn,tnm,jm->tj", Zs, Ps, Zs), 0.0),
                              state_vars=np.diagonal(Ps, axis1=1, axis2=2))
        st = cache[key]
        out.update(st)
        sc = st["sigmacount"]
        if weight_index == "compressed":
            out["mle"] = oracle.get_mle(st["sigmas"][:sc], st["detfs"][:sc], st["oc"], warmup)
        else:
            out["mle"] = adjoint_ref.forward(y, phi, q, G, warmup, x0, P0, Rv, weight_index)[0]
    if "grad" in parts and has_gradient(N, K):
        key = ("grad", i, r, warmup, weight_index)
        if key not in cache:
            cache[key] = adjoint_ref.gradient(y, phi, q, G, warmup, x0, P0, Rv, weight_index)
        out["gmle"], out["gphi"], out["gq"] = cache[key]
    if "loo" in parts and has_loo(N, K):
        key = ("loo", i, r)
        if key not in cache:
            m, v = loo_ref.loo_tape(y, phi, q, G, Rv, x0, P0)
            scale = np.ones(N) if g["scale"] is None else g["scale"][r]
            offset = np.zeros(N) if g["offset"] is None else g["offset"][r]
            cache[key] = (m * scale + offset, np.maximum(v, 0.0) * scale ** 2)
        out["loo_means"], out["loo_vars"] = cache[key]
    return out


# -------------------------------------------------------------------------------------------------------------------- bars
def bar(quantity, ref, g, r):
    """The bar of a quantity (scalar or elementwise) around its reference value ``ref``, for an instance of record r."""
    if quantity == "mle":
        return MLE_RTOL * max(1.0, abs(float(ref)))
    if quantity in ("F", "Pf", "Xp", "Pp"):
        return FILT_ATOL
    if quantity in ("S", "Ps", "state_vars"):
        return SMOOTH_ATOL
    if quantity in ("sim_means", "sim_vars"):
        return 2.0 * SMOOTH_ATOL * (1.0 if g["scale"] is None else float(g["scale"][r].max()) ** 2)
    if quantity in ("gphi", "gq"):
        return GRAD_RTOL * np.abs(ref) + GRAD_RTOL * np.abs(ref).max()
    if quantity in ("loo_means", "loo_vars"):
        return LOO_TOL * max(1.0, float(np.nanmax(np.abs(ref))) if np.isfinite(ref).any() else 1.0)
    if quantity == "sigmas":
        return SIGMA_RTOL * np.abs(ref) + SIGMA_ATOL
    if quantity == "detfs":
        return DETF_ATOL
    raise KeyError(quantity)


def bars_apart(quantity, got, ref, g, r):
    """max |got - ref| / bar: at most 1 for a value that passes.  A NaN on one side only counts as infinitely far; where the
    bar is zero (a reference that is exactly zero), any difference does."""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    b = np.broadcast_to(bar(quantity, ref, g, r), ref.shape)
    both = np.isfinite(got) & np.isfinite(ref)
    diff = np.where(both, np.abs(np.where(both, got, 0.0) - np.where(both, ref, 0.0)), np.where(np.isnan(got) == np.isnan(ref), 0.0, np.inf))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(b > 0, diff / np.where(b > 0, b, 1.0), np.where(diff > 0, np.inf, 0.0))
    return float(np.max(ratio)) if ratio.size else 0.0


def assert_close(quantity, got, ref, g, r, what):
    got = np.asarray(got)
    assert got.shape == np.shape(ref), "%s %s: shape %s, expected %s" % (what, quantity, got.shape, np.shape(ref))
    d = bars_apart(quantity, got, ref, g, r)
    assert d <= 1.0, "%s: %s is %.3g bars from its reference" % (what, quantity, d)


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _what(g, i, extra=""):
    return "(%d,%d) instance %d, record %d (%s)%s" % (g["N"], g["K"], i, i % g["R"], g["patterns"][i % g["R"]], extra and " " + extra)


# -------------------------------------------------------------------------------------------------------- check functions
# Each takes an engine that holds the group's records -- metran_amd.engine.BatchedKalman on the GPU,
# tests/oracle_engine.py::OracleEngine on the CPU -- and compares every instance with ``reference``.
def check_objective(kf, g, warmups, tag=""):
    """loglik at every warm-up; at a warm-up beyond the record's length the objective is exactly zero."""
    for w in warmups:
        got = _np(kf.loglik(g["phi"], g["q"], warmup=w, **init(g)))
        assert got.shape == (g["B"],)
        for i in range(g["B"]):
            ref = reference(g, i, w, parts=("state",))
            assert_close("mle", got[i], ref["mle"], g, ref["rec"], _what(g, i, "%s warm-up %d" % (tag, w)))
            if w >= g["T"]:
                assert got[i] == 0.0, _what(g, i, "%s warm-up %d" % (tag, w))


def check_gradient(got, g, warmup, tag=""):
    """(mle, gphi, gq) of loglik_grad at ``warmup``; where the warm-up leaves no observed step (the "single" record from
    warm-up 1 on) the gradient is exactly zero."""
    mle, gphi, gq = (_np(t) for t in got)
    assert mle.shape == (g["B"],) and gphi.shape == gq.shape == g["phi"].shape
    for i in range(g["B"]):
        ref = reference(g, i, warmup, parts=("state", "grad"))
        what = _what(g, i, "%s warm-up %d" % (tag, warmup))
        assert_close("mle", mle[i], ref["mle"], g, ref["rec"], what)
        assert_close("gphi", gphi[i], ref["gphi"], g, ref["rec"], what)
        assert_close("gq", gq[i], ref["gq"], g, ref["rec"], what)
        if warmup >= ref["sigmacount"]:
            assert not gphi[i].any() and not gq[i].any(), what


def check_gradient_alpha(kf, g, dt=0.5, warmup=2):
    """loglik_grad_alpha with B > R against adjoint_ref chained through params.phi_q_from_alpha and the extended-precision
    galpha of tests/helper_ref.py (bar: see the module docstring)."""
    alpha, ga = alpha_group(g, dt)
    mle, galpha = (_np(t) for t in kf.loglik_grad_alpha(alpha, dt=dt, warmup=warmup))
    assert mle.shape == (g["B"],) and galpha.shape == alpha.shape
    for i in range(g["B"]):
        ref = reference(ga, i, warmup, parts=("state", "grad"))
        r, what = ref["rec"], _what(g, i, "galpha, warm-up %d" % warmup)
        assert_close("mle", mle[i], ref["mle"], ga, r, what)
        want, moduli = helper_ref.alpha_grad(alpha[i], g["loadings"][r], dt, ref["gphi"], ref["gq"])
        c = np.concatenate([1.0 - (g["loadings"][r] ** 2).sum(1), np.ones(g["K"])])
        w = ga["phi"][i] * dt / alpha[i] ** 2
        tol = (helper_ref.galpha_bound(alpha[i], dt, ref["gphi"], moduli)
               + (bar("gphi", ref["gphi"], ga, r) + np.abs(2.0 * ga["phi"][i] * c) * bar("gq", ref["gq"], ga, r)) * w)
        err = np.abs(galpha[i] - want)
        assert (err <= tol).all(), "%s: %.3g of its bound" % (what, float((err / np.maximum(tol, 1e-300)).max()))
        if warmup >= ref["sigmacount"]:
            assert not galpha[i].any(), what
    return mle, galpha


def check_two_phase(forward, backward, both, point, decoy, what, same_forward=True):
    """A forward pass at a decoy point, one at the point, then ONE backward walk: bit for bit what the single call gives at
    the point.  ``forward(p) -> mle``, ``backward() -> gradient arrays``, ``both(p) -> (mle, gradient arrays...)``.
    ``same_forward=False``: the CPU engine of tests/oracle_engine.py, whose forward pass is the C oracle and whose single call
    takes the objective from the numpy adjoint -- the pair tests/test_adjoint.py holds to 1e-10 relative."""
    forward(decoy)
    mle = _np(forward(point))
    grads = backward()
    grads = [_np(t) for t in (grads if isinstance(grads, (tuple, list)) else (grads,))]
    ref = [_np(t) for t in both(point)]
    if same_forward:
        assert np.array_equal(mle, ref[0]), what + ": objective"
    else:
        assert (np.abs(mle - ref[0]) <= 1e-10 * np.maximum(1.0, np.abs(ref[0]))).all(), what + ": objective"
    assert len(grads) == len(ref) - 1
    for a, b in zip(grads, ref[1:]):
        assert np.array_equal(a, b), what + ": gradient"


def check_position_independent(fn, g, what):
    """The S * R call equals, bit for bit, the S separate calls with B = R on the same records: ``fn(group) -> {name: array
    [B, ...]}``.  No reference and no tolerance: cross-talk between the models of one wavefront shows however small it is."""
    whole = {k: _np(v).copy() for k, v in fn(g).items()}
    R = g["R"]
    for s in range(g["B"] // R):
        sl = slice(s * R, (s + 1) * R)
        part = fn(take(g, sl))
        assert set(part) == set(whole)
        for k, v in part.items():
            assert np.array_equal(whole[k][sl], _np(v), equal_nan=True), "%s: %s of instances %d..%d depends on their position" % (
                what, k, sl.start, sl.stop - 1)

"""Seeded generator of "hard" dynamic-factor models for the property sweeps (test infrastructure; used by the GPU tier's
tests/test_gpu_property.py and, on the CPU, by tests/test_property_generator.py, which runs the SAME sweep through the oracle
and the numpy restatements so that every tolerance below is known to hold between two independent implementations before
a GPU minute is spent on it; the diagnostic routes -- disturbances, forecasts, observation weights, draws -- take the same
sweep in tests/test_gpu_property_diagnostics.py / tests/test_property_diagnostics.py, the fitting routes -- intervention effects,
window functionals, per-step scores -- in tests/test_gpu_property_fits.py / tests/test_property_fits.py, with the bars at the end of
this file).

A group = B models of one shape (N, K) and one length T (a launch needs a common T), each model drawn independently:
  persistence   phi = exp(-1/alpha), alpha ~ U(2, 60) (Metran's parametrisation, metran.py:246-263); in 30 % of the models one
                or two states (series or factor) get phi = 1 - 10^U(-9, -3) instead -- up to 1 - 1e-9.  (ALL states that
                persistent would make every innovation variance a 1e-9 difference of O(1) covariances: the objective
                is then conditioned like 1e-16 / 1e-9 and no two implementations agree to 1e-9 on it.)
  loadings      random signs, rows scaled to a communality drawn from {0.2, 0.9, 0.999} x U(0.3, 1)
  q             Metran's: (1 - phi^2)(1 - communality) for the series, 1 - phi^2 for the factors (metran.py:310-322)
  data          simulated from the model (prior N(0, I)), for half of the typical models plus noise; then one missingness pattern:
                none | iid 30 % | heavy 95 % | whole steps | never-observed series | a single observation |
                empty first step | empty last step | empty first and last
  group-wide    observation variances R >= 0 (zero for about half of the series) or none; x0 / P0 (SPD) or the defaults
"""
import numpy as np

PATTERNS = ("none", "iid", "heavy", "steps", "series", "single", "first", "last", "both")
AOT_SHAPES = [(8, 2), (5, 1), (2, 1), (3, 1), (4, 1), (6, 2), (14, 3), (32, 4)]
JIT_SHAPES = [(7, 2), (20, 2), (48, 3)]   # all built anyway by tests/test_hip_parity.py::test_runtime_specialised_shapes; (48,3): the
# tape of a model with more than 32 series (round 5) -- appended, so that the groups drawn before it stay what they were


def draw_model(rng, N, K, T, pattern):
    n = N + K
    phi = np.exp(-1.0 / rng.uniform(2.0, 60.0, n))
    if rng.random() < 0.3:   # one or two states (series or factor) with a persistence up to 1 - 1e-9
        idx = rng.choice(n, size=min(n, int(rng.integers(1, 3))), replace=False)
        phi[idx] = 1.0 - 10.0 ** rng.uniform(-9.0, -3.0, idx.size)
    load = rng.uniform(-1.0, 1.0, (N, K))
    comm = rng.choice([0.2, 0.9, 0.999])
    load *= np.sqrt(comm / np.maximum((load ** 2).sum(1), 1e-12))[:, None] * rng.uniform(0.3, 1.0, N)[:, None]
    q = 1.0 - phi ** 2
    q[:N] *= 1.0 - (load ** 2).sum(1)
    # data from the model itself, started from its prior x_{-1} ~ N(0, I) (run_filter's P0, kalmanfilter.py:747-750): with a
    # persistence of 1 - 1e-9 the innovation variances are ~1e-9, and data the model could not have produced would put
    # terms v^2 / f ~ 1e9 into the objective -- a test of cancellation, not of the filter.  A typical-persistence model also
    # gets plain noise on top (off the model's manifold, like real residual series).
    x = rng.standard_normal(n)
    y = np.empty((T, N))
    for t in range(T):
        x = phi * x + np.sqrt(q) * rng.standard_normal(n)
        y[t] = x[:N] + load @ x[N:]
    if rng.random() < 0.5:
        y += 0.3 * rng.standard_normal((T, N))
    if pattern == "iid":
        y[rng.random((T, N)) < 0.3] = np.nan
    elif pattern == "heavy":
        y[rng.random((T, N)) < 0.95] = np.nan
    elif pattern == "steps":
        y[rng.random(T) < 0.5] = np.nan
    elif pattern == "series":
        y[:, rng.random(N) < 0.5] = np.nan
        y[rng.random((T, N)) < 0.2] = np.nan
    elif pattern == "single":
        keep = (rng.integers(T), rng.integers(N))
        v = y[keep]
        y[:] = np.nan
        y[keep] = v
    else:
        if pattern in ("first", "both"):
            y[rng.random((T, N)) < 0.2] = np.nan
            y[0] = np.nan
        if pattern in ("last", "both"):
            y[rng.random((T, N)) < 0.2] = np.nan
            y[-1] = np.nan
    return y, phi, q, load


def draw_group(seed, N, K, T, B):
    """dict: obs [B,T,N], phi / q [B,n], loadings [B,N,K], obsvar [B,N] or None, x0 [B,n] / P0 [B,n,n] or None, patterns."""
    rng = np.random.default_rng([int(seed), N, K, T, B])
    n = N + K
    g = dict(obs=np.empty((B, T, N)), phi=np.empty((B, n)), q=np.empty((B, n)), loadings=np.empty((B, N, K)), patterns=[])
    for b in range(B):
        pat = PATTERNS[(b + int(rng.integers(len(PATTERNS)))) % len(PATTERNS)] if B < len(PATTERNS) else PATTERNS[b % len(PATTERNS)]
        g["obs"][b], g["phi"][b], g["q"][b], g["loadings"][b] = draw_model(rng, N, K, T, pat)
        g["patterns"].append(pat)
    g["obsvar"] = rng.uniform(0.0, 0.5, (B, N)) * (rng.random((B, N)) < 0.5) if rng.random() < 0.4 else None
    if rng.random() < 0.4:
        g["x0"] = rng.normal(size=(B, n))
        A = rng.normal(size=(B, n, n))
        g["P0"] = A @ A.transpose(0, 2, 1) / n + 0.5 * np.eye(n)
    else:
        g["x0"] = g["P0"] = None
    return g


def groups(seed=None, per_shape=32, shapes=None):
    """The sweep: for every shape two groups, a short one (T in 1..12, 12 models) and a longer one (T in 20..56, the rest).
    The default seed is fixed (the tier is deterministic); ``METRAN_SWEEP_SEED=<int>`` draws another sweep of the same classes
    (profiles/r05/gpu_property_other_seeds.log: three more sweeps, 1 056 more models, run once on the final kernels)."""
    import os

    if seed is None:
        seed = int(os.environ.get("METRAN_SWEEP_SEED", "20250922"))
    rng = np.random.default_rng(seed)
    for (N, K) in (shapes or (AOT_SHAPES + JIT_SHAPES)):
        for (tlo, thi, B) in ((1, 13, 12), (20, 57, per_shape - 12)):
            T = int(rng.integers(tlo, thi))
            yield (N, K, T, B), draw_group(seed, N, K, T, B)


def oracle_model(oracle, g, b, smooth=True):
    """The reference algorithm on model b of a group (oracle/: C restatement of kalmanfilter.py:236-476, 550-567) with its
    observation variances and initial moments.  dict: sigmas, detfs, sigmacount, mle, F, Pf, Xp, Pp (, S, Ps)."""
    N, K = g["loadings"].shape[1:]
    n = N + K
    Z = np.concatenate([np.eye(N), g["loadings"][b]], axis=1)
    R = np.zeros(N) if g["obsvar"] is None else g["obsvar"][b]
    x0 = np.zeros(n) if g["x0"] is None else g["x0"][b]
    P0 = np.eye(n) if g["P0"] is None else g["P0"][b]
    o, oi, oc = oracle.set_observations(g["obs"][b])
    sg, df, sc, F, Pf, Xp, Pp = oracle.seqkalmanfilter(o, np.diag(g["phi"][b]), np.diag(g["q"][b]), Z, R, oi, oc, x0, P0)
    out = dict(sigmas=sg, detfs=df, sigmacount=sc, F=F, Pf=Pf, Xp=Xp, Pp=Pp, mle=oracle.get_mle(sg[:sc], df[:sc], oc), Z=Z)
    if smooth:
        out["S"], out["Ps"] = oracle.kalmansmoother(F, Pf, Xp, Pp, np.diag(g["phi"][b]))
    return out


def conditioning(g, b, ref):
    """What the REFERENCE's fp64 filter itself loses on model b: an innovation variance f is a difference of O(scale)
    covariance entries and cannot be smaller than ~min(q), so its relative rounding error is up to eps * scale / min(q) --
    and so is that of everything divided by it (the gain, sigma = v^2 / f).  With a persistence of 1 - 1e-9 (q ~ 2e-9) that is
    ~1e-7: the oracle is 7e-9 (sigmas) / 3e-9 (filtered means) from an extended-precision run of the same recursion on such
    models (tests/test_property_generator.py::test_reference_algorithm_conditioning), and two correct fp64 implementations
    differ from each other by as much.  Returned: 2 eps * scale / min(q); ~1e-15 for an ordinary model."""
    scale = max(1.0, float(np.abs(ref["Pp"]).max()), float(np.abs(ref["F"]).max()))
    return 2.0 * np.finfo(float).eps * scale / float(g["q"][b].min())


def mle_tolerance(g, b, ref, value=None):
    """Absolute tolerance on -2 log L of model b (``value``: the objective under another warm-up, default ref["mle"]): the
    north-star bar (1e-9 relative) plus the reference algorithm's own conditioning -- the objective is a sum of sigmas, so
    it inherits their eps * scale / min(q) (seed 23 of the sweep holds two models whose fp64 oracle is 0.7e-9 / 1.9e-9 from
    the extended-precision objective)."""
    value = ref["mle"] if value is None else value
    return (1e-9 + conditioning(g, b, ref)) * max(1.0, abs(float(value)))


def filter_tolerances(g, b, ref):
    """(atol of the per-step sigmas -- on top of the flat 1e-9 relative bar --, atol of the filtered / predicted moments) for
    model b: the repository's bars (1e-9 relative / 1e-10 for the sigmas, 1e-10 on the scale of the moments) plus the reference
    algorithm's own conditioning (``conditioning``).  The conditioning term of a sigma is ABSOLUTE, on the scale of the model's
    largest sigma: sigma_t = v^2 / f carries the accumulated error of the state mean through v, so a step whose innovation
    happens to be small next to the model's others (sigma_t 5e-6 beside 8e6: seed 88 of the sweep) has NO relative accuracy in
    the reference's own fp64 arithmetic -- the oracle is up to 29 eps scale / min(q) from the extended-precision run on such
    entries relative to themselves (seeds 62, 88, 122, 125: found by METRAN_SWEEP_SEED = 41 .. 70 on the GPU, where both kernel
    families sat 1.1e-6 / 1.5e-7 from the oracle on ONE sigma each, and the oracle 1.4e-6 from the truth on the first) but never
    more than 0.52 of it on the scale of the largest sigma (104 sweeps, 1 800 extreme models:
    tests/test_property_generator.py::test_reference_algorithm_conditioning).  Sigmas are consumed through their sum only."""
    scale = max(1.0, float(np.abs(ref["Pp"]).max()), float(np.abs(ref["F"]).max()))
    c = conditioning(g, b, ref)
    sc = ref["sigmacount"]
    top = max(1.0, float(np.abs(ref["sigmas"][:sc]).max())) if sc else 1.0
    return 1e-10 + c * top, 1e-10 * scale + c


def extended_precision_filter(g, b):
    """The sequential filter of model b in numpy's extended precision (80-bit on x86: eps 1e-19): per-step sigmas of the
    observed steps and the filtered means.  Plain loops; for the handful of extreme models of the sweep."""
    LD = np.longdouble
    y, G = g["obs"][b], g["loadings"][b]
    T, N = y.shape
    K = G.shape[1]
    n = N + K
    Z = np.concatenate([np.eye(N), G], axis=1).astype(LD)
    R = np.zeros(N) if g["obsvar"] is None else g["obsvar"][b]
    x = (np.zeros(n) if g["x0"] is None else g["x0"][b]).astype(LD)
    P = (np.eye(n) if g["P0"] is None else g["P0"][b]).astype(LD)
    phi, q = g["phi"][b].astype(LD), g["q"][b].astype(LD)
    sig, Fs = [], []
    for t in range(T):
        x = phi * x
        P = P * np.outer(phi, phi) + np.diag(q)
        s, seen = LD(0), False
        for j in range(N):
            if np.isfinite(y[t, j]):
                seen = True
                z = Z[j]
                v = LD(y[t, j]) - z @ x
                d = P @ z
                f = LD(R[j]) + z @ d
                k = d / f
                x = x + k * v
                P = P - np.outer(k, k) * f
                s += v * v / f
        if seen:
            sig.append(s)
        Fs.append(x.copy())
    return np.array(sig, dtype=LD), np.array(Fs, dtype=LD)


def smoother_tolerance(g, b, ref):
    """Absolute tolerance on smoothed moments of model b: the repository's smoother bar (1e-9) on the scale of the moments
    in play, plus what the REFERENCE algorithm itself loses in its explicit inverse of the predicted covariance
    (kalmanfilter.py:455-462): eps * cond(Pp) ~ 1e-15 / min(q) -- with persistence close to 1 or a communality close to 1 two
    correct implementations of the reference's formulas differ by that much (tests/test_dk_tape.py, property test)."""
    big = max(1.0, float(np.abs(ref["Pp"]).max()), float(np.abs(ref["F"]).max()))
    return 1e-9 * big + 4e-15 * big * big / float(g["q"][b].min())


# ------------------------------------------------------------------------------------------ the diagnostic routes' bars
# Each bar has the form of filter_tolerances: (the tier's own flat bar + MARGIN * measured * conditioning) * max(1, largest
# modulus of the quantity).  ``measured`` is not chosen: it is the largest (float64 restatement - longdouble restatement) /
# (conditioning * scale) that scripts/measure_diagnostic_bars.py finds over the default sweep and 30 further ones
# (METRAN_SWEEP_SEED = 1 .. 30; 10 912 models); its output is quoted in the docstrings.  MARGIN = 4: the kernels sum in tree order
# with fused multiply-adds -- another sample of the same rounding process -- and the filter's bars leave about 2 x (0.52 measured,
# 1.0 allowed); 4 keeps room for unseen seeds and still rejects the 1e-6-sized error of a dropped term.  ``margin=1`` is what
# tests/test_property_diagnostics.py holds the two restatements to.
MARGIN = 4.0
RAW_TOL = 1e-12         # tests/test_disturbance_gpu.py::RAW_TOL
FORECAST_ATOL_MEAN = 1e-12   # tests/test_forecast_gpu.py::ATOL_MEAN
FORECAST_RTOL_VAR = 1e-12    # tests/test_forecast_gpu.py::RTOL_VAR
WEIGHTS_BAR = 1e-13     # tests/test_weights_gpu.py::BAR
DRAW_TOL = 1e-9         # tests/test_draws_gpu.py::TOL, the smoothed-moment bar: smoother_tolerance's flat part
PERTURB_TOL = 1e-11     # tests/test_draws_gpu.py::PERTURB_TOL
# the last line of scripts/measure_diagnostic_bars.py (31 sweeps, 10 912 models):
MEASURED = {"dist_r": 0.43, "dist_n": 2.1, "forecast_mean": 0.18, "forecast_var": 0.62, "weights_series": 0.47, "weights_states": 0.86}
# ... and of its run with the fitting routes (the same 31 sweeps; those routes on the 279 compared models of the default sweep and,
# for the 30 further seeds, on the compared models of the shapes up to N + K = 22: 7 612 more for the regression, 7 212 for the scores),
# each figure the printed one rounded UP.  The score figures are not of order one: see ``score_tolerances``.
MEASURED.update({"regress_normal": 3.5, "regress_beta": 46.0, "regress_cov": 0.31, "regress_gain": 7.8,
                 "score_score": 4.9e3, "score_grad": 1.7e3, "score_opg": 5.4e4, "score_cusum": 2.1e2})


def _top(a):
    a = np.abs(np.asarray(a, dtype=np.float64))
    return max(1.0, float(np.nanmax(a))) if np.isfinite(a).any() else 1.0


def disturbance_tolerances(g, b, ref, r, ninfo, margin=MARGIN):
    """(atol of r, atol of ninfo) of model b against disturbance_ref.dist_adjoint in longdouble; ``r``, ``ninfo``: that
    reference (their largest moduli are the scales).  Measured, float64 against longdouble restatement in units of
    conditioning * scale: r 0.228 (default sweep) / 0.425, 0.365, 0.266 (seeds 1-10, 11-20, 21-30), the largest at seed 2,
    (7,2) T = 7, "none"; ninfo 1.32 / 2.11, 1.88, 1.50, the largest at seed 4, (6,2) T = 4, "last".  The largest gaps themselves
    are 2.05e-08 (r: seed 6, (5,1) T = 7, "iid", min q 4.3e-9, ratio 0.14) and 1.47e-07 (ninfo: seed 18, (5,1) T = 46, "none", min q
    3.4e-9, ratio 0.56).  ninfo's ratio is about five times r's -- N_t accumulates squares of what r_t accumulates once -- but it
    is the same on ordinary models (min q ~ 0.03: up to 2.1) and on the 2 510 models whose conditioning exceeds 1e-10 (up to 1.3),
    over six orders of magnitude of min q: it scales with the conditioning, and no other scale (the largest 1 / f) is needed."""
    c = conditioning(g, b, ref)
    return (RAW_TOL + margin * MEASURED["dist_r"] * c) * _top(r), (RAW_TOL + margin * MEASURED["dist_n"] * c) * _top(ninfo)


def forecast_tolerances(g, b, ref, means, margin=MARGIN):
    """(atol of a forecast mean, rtol of a forecast variance) of model b against forecast_ref in longdouble; ``means``: the
    reference's means in play (the scale of the mean is max(1, max |y|, max |mean|), as tests/test_forecast_gpu.py's).
    Measured over the whole table (every origin, 14 horizons), in units of conditioning (* scale for the mean): mean 0.0456
    (default sweep) / 0.178, 0.110, 0.178 (seeds 1-10, 11-20, 21-30), the largest at seed 1, (8,2) T = 38, "series"; variance
    0.259 / 0.432, 0.530, 0.622, the largest at seed 30, (2,1) T = 23, "last".  Largest gaps: 5.0e-09 (mean: seed 8, (3,1)
    T = 49, "first", min q 2.3e-9) and 3.6e-08 relative (variance: seed 14, (5,1) T = 33, "steps", min q 2.4e-9)."""
    c = conditioning(g, b, ref)
    return ((FORECAST_ATOL_MEAN + margin * MEASURED["forecast_mean"] * c) * max(_top(g["obs"][b]), _top(means)),
            FORECAST_RTOL_VAR + margin * MEASURED["forecast_var"] * c)


def weights_tolerance(g, b, ref, w, what="series", margin=MARGIN):
    """atol of the weights and the intercept of ONE target of model b against weights_ref.weights in longdouble; ``w``: the
    reference's weights of that target.  Measured over the sweep's targets (tests/diagnostic_sweep.py::targets), relative to
    max(1, max |w|) and in units of conditioning: series 0.384 (default sweep) / 0.472, 0.435, 0.389 (seeds 1-10, 11-20, 21-30),
    states 0.209 / 0.864, 0.306, 0.407, both largest at seed 5, (2,1) T = 39, "last", min q 7.7e-6.  Largest gaps: 1.2e-08
    (series: seed 8, (3,1) T = 49, "first") and 3.0e-08 (states: seed 6, (5,1) T = 7, "iid")."""
    c = conditioning(g, b, ref)
    return (WEIGHTS_BAR + margin * MEASURED["weights_" + what] * c) * _top(w)


def draw_tolerance(g, b, ref_star, xplus, what="series"):
    """atol of one posterior draw of model b against draw_ref.draw_model.  A draw is x+ + E[x | y*]: the unconditional path
    (the perturb tier's PERTURB_TOL on the scale of x+) plus a smoothing pass of the record y* = y - y+, NOT of y -- so the
    smoother's bar is ``smoother_tolerance`` on the oracle's moments of THAT record (``ref_star``: hard_models.oracle_model of
    the group with y* in place of y).  Nothing is measured here: both parts are bars of existing tiers.  A series draw is a
    projection z_j' x: both parts times the largest absolute row sum of Z = [I | loadings] (at most 1 + sqrt(K): a row of the
    loadings has at most unit length)."""
    rows = float((1.0 + np.abs(g["loadings"][b]).sum(1)).max()) if what == "series" else 1.0
    return rows * (smoother_tolerance(g, b, ref_star) + PERTURB_TOL * _top(xplus))


# ------------------------------------------------------------------ the fitting routes' bars (regression, functionals, scores)
REGRESS_BAR_A = max(16 * 1.31e-14, 1e-13)     # tests/test_regression_gpu.py::BAR_A (16 x measured, the floor of 1e-13)
REGRESS_BAR_S = max(16 * 1.07e-13, 1e-13)     # tests/test_regression_gpu.py::BAR_S
FUNCTIONAL_ATOL = 1e-9                        # tests/call_forms.py::SMOOTH_ATOL: smoother_tolerance's flat part
SCORE_SHORT = 2                               # tests/test_scores_gpu.py::SHORT: records of up to two steps have bars of their own
SCORE_BAR = {"score": max(16 * 2.11e-14, 1e-13), "grad": max(16 * 4.96e-15, 1e-13), "opg": max(16 * 8.78e-15, 1e-13),
             "cusum": max(16 * 1.01e-16, 1e-13)}                                     # tests/test_scores_gpu.py::BAR
SCORE_BAR_SHORT = {"score": max(16 * 1.16e-14, 1e-13), "grad": max(16 * 8.75e-14, 1e-13), "opg": max(16 * 9.88e-14, 1e-13),
                   "cusum": max(16 * 2.78e-16, 1e-13)}                               # tests/test_scores_gpu.py::BAR_SHORT


def score_tolerances(g, b, ref, T, margin=MARGIN):
    """{"score", "grad", "opg", "cusum"}: the bar of score_ref.differences -- a difference relative to score_ref's own scale (the
    output's expression with every term replaced by its absolute value) -- of model b against score_ref.scores in longdouble;
    ``T``: the record's length (up to SCORE_SHORT steps the flat part is the short records').  The scales are score_ref's, raised
    where Metran's chain rule makes the prediction's tangent term cancel (tests/diagnostic_sweep.py::_floored).
    Measured, float64 against longdouble restatement in units of conditioning * scale, default sweep / seeds 1-10, 11-20, 21-30:
    score 0.733 / 4.71e3, 4.89e3, 2.5e3 (the largest at seed 20, (3,1) T = 39, "iid", min q 4.9e-9); grad 0.436 / 1.48e3, 1.01e3,
    1.61e3; opg 22.6 / 3.23e4, 3.68e3, 5.38e4; cusum 0.0369 / 83.6, 52.2, 205 (these three largest at seed 23, (3,1) T = 8, "last",
    min q 1.8e-9).  The largest gaps themselves: 1.3e-3 (score: seed 8, (3,1) T = 49, "first", min q 2.3e-9), 5.0e-4 (grad), 1.7e-2
    (opg), 6.3e-5 (cusum: all seed 23).  These are NOT multiples of order one, as every other route's are: on the default sweep the
    tangent filter stays below 0.74 of the conditioning (22.6 for opg, whose scale sum_t scale(s_t) scale(s_t)' is small where the
    large steps of two parameters are different steps -- a "heavy" record), but at models of the further seeds with min q of a few 1e-9
    a correct float64 evaluation of fd / f - v^2 fd / f^2 loses a thousand times more than the filter underneath it
    loses -- the loss grows faster than 1 / min q.  The bar follows the measurement (the form allows nothing else), so on a model
    with q ~ 2e-9 it is about 6e-3 of the scale, while at min q >= 1e-6 (conditioning 1e-9 and below) it stays under 2e-5 (score)
    and every wrong variant is still outside it in every group (tests/test_property_fits.py)."""
    c = conditioning(g, b, ref)
    flat = SCORE_BAR_SHORT if T <= SCORE_SHORT else SCORE_BAR
    return {k: flat[k] + margin * MEASURED["score_" + k] * c for k in flat}


def regression_scales(reg):
    """The scales of a regression result (``reg``: regress_ref.regression in longdouble): ``normal [M+1,M+1]`` sqrt(|A_pp| |A_qq|)
    (1 where it is zero), ``beta [M]`` the standard errors and ``cov [M,M]`` se_i se_j of the kept effects (NaN at a dropped one),
    ``gain`` the gain's own expression sum_i beta_i s_i, s = A[1:,0], with every term replaced by its absolute value (1 where
    nothing is kept), ``cond`` regress_ref.unit_condition of the kept effects."""
    import regress_ref

    A = np.abs(np.asarray(reg["normal"], dtype=np.float64))
    dg = np.sqrt(np.diag(A))
    normal = np.outer(dg, dg)
    normal[normal == 0] = 1.0
    cov = np.asarray(reg["cov"], dtype=np.float64)
    se = np.sqrt(np.diag(cov))
    kept = ~np.asarray(reg["dropped"])
    gain = float((np.abs(np.asarray(reg["beta"], dtype=np.float64)) * A[1:, 0])[kept].sum()) if kept.any() else 0.0
    return dict(normal=normal, beta=se, cov=np.outer(se, se), gain=gain if gain > 0 else 1.0,
                cond=regress_ref.unit_condition(reg["normal"], reg["dropped"]))


def regression_tolerances(g, b, ref, reg, margin=MARGIN):
    """{"normal" [M+1,M+1], "beta" [M], "cov" [M,M], "gain"}: absolute bars of model b against regress_ref.regression in longdouble
    (``reg``: that reference), each (flat + margin * MEASURED * conditioning) * ``regression_scales``; the flat parts are the
    regression tier's BAR_A (normal matrix) and BAR_S (the rest).  For beta and cov the conditioning is multiplied by the condition
    number of the unit-diagonal S of the kept effects (``cond``, up to 9.5e8 on the sweep's effect lists: a level shift and a ramp on
    one series of a two-step record are nearly collinear).
    Measured, float64 against longdouble restatement in units of conditioning * scale (beta, cov: * cond), default sweep / seeds
    1-10, 11-20, 21-30: normal 0.218 / 0.597, 3.5, 0.871 (the largest at seed 17, (7,2) T = 2, "iid"); beta 0.315 / 17.6, 45.3, 10.1
    (seed 12, (2,1) T = 27, "series", min q 5.2e-8); cov 0.0807 / 0.258, 0.302, 0.137 (seed 12, (7,2) T = 2, "series"); gain 0.543 /
    3.72, 7.61, 7.76 (seed 23, (4,1) T = 2, "iid").  Largest gaps: 7.5e-9 (normal), 4.9e-6 of a standard error (beta: seed 8, (3,1)
    T = 49, "first", min q 2.3e-9), 5.1e-9 (cov), 2.6e-8 (gain).  The factor cond is borne out for the ordinary models and not
    needed for the hard ones: WITHOUT it the ratios are 0.65 (beta) and 0.625 (cov) on the default sweep but 2.9e4 and 5.5e4 beyond
    it, both at two-step records of ordinary models whose cond is 1e6 to 1e9 -- among the models whose conditioning exceeds 1e-10
    beta is at most 82 without the factor and 45.3 with it.  So it stays.  All of this holds for the models that meet
    tests/diagnostic_sweep.py::regression_usable (a dropped set that does not hang on rounding); the others leave beta and cov."""
    c = conditioning(g, b, ref)
    sc = regression_scales(reg)
    solve = margin * c * sc["cond"]
    return dict(normal=(REGRESS_BAR_A + margin * MEASURED["regress_normal"] * c) * sc["normal"],
                beta=(REGRESS_BAR_S + MEASURED["regress_beta"] * solve) * sc["beta"],
                cov=(REGRESS_BAR_S + MEASURED["regress_cov"] * solve) * sc["cov"],
                gain=(REGRESS_BAR_S + margin * MEASURED["regress_gain"] * c) * sc["gain"])


def functional_tolerances(g, b, ref, reach):
    """(atol of the mean, atol of the variance) [W,C] of the window functionals of model b against functional_ref.functional_walk
    in longdouble from the ORACLE's records.  The kernel walks its OWN filtered and smoothed records, so its bar is the smoother's
    bar of this model, ``smoother_tolerance`` (flat part FUNCTIONAL_ATOL), carried through the functional as functional_ref.bars
    carries it: times ``reach`` = A zeta for the mean and (A zeta)^2 for the variance (tests/diagnostic_sweep.py::functional_reach).
    Nothing is measured here: two existing bars combined, as ``draw_tolerance``.  What the walk itself loses in float64 is recorded
    by scripts/measure_diagnostic_bars.py: at most 2.7e-7 (mean) and 6.3e-7 (variance) of this bar over the 31 sweeps (7 891 models)."""
    tol = smoother_tolerance(g, b, ref)
    return tol * reach, tol * reach * reach

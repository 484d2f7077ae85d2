"""The property sweep of tests/hard_models.py for the DIAGNOSTIC routes and the FITTING routes -- intervention effects, window
functionals, per-step scores -- (test infrastructure shared by tests/test_property_diagnostics.py and tests/test_property_fits.py
on the CPU, tests/test_gpu_property_diagnostics.py and tests/test_gpu_property_fits.py on the GPU and
scripts/measure_diagnostic_bars.py): which models of a group are compared, the inputs every route derives from the model itself
(weight targets, forecast origins, effect lists, windows and contrasts, Metran's derivatives) and the references -- the numpy restatements in ``np.longdouble`` (the yardstick) or
``np.float64`` (what a correct float64 code does), the oracle's moments, the oracle's draws.  Every reference of a model is
computed once and kept with its group (``g["_cache"]``), read-only, so that the routes share a model's gains, forecast table
and oracle moments.
"""
import numpy as np

import disturbance_ref
import draw_ref
import forecast_ref
import functional_ref
import hard_models
import innov_ref
import oracle
import regress_ref
import score_ref
import time_axis
import weights_ref

HORIZON = 14
T_FIRST = 1
COVERAGE = 0.95
Z95 = 1.959963984540054   # the two-sided normal quantile of COVERAGE (forecast_ref's default)
M_SERIES, M_STATES = 6, 3
GENERIC_SHAPES = [(8, 2), (14, 3), (20, 2)]
DIST_VARIANTS = ("after_phi", "before_updates", "no_rr", "shifted")
FORECAST_VARIANTS = ("origin_shift", "q_once")
WEIGHTS_VARIANTS = ("stop_at_target", "no_c", "descending")
REGRESS_VARIANTS = ("descending", "inclusive", "ramp_from_zero", "late_sums", "skip_before")
FUNCTIONAL_VARIANTS = functional_ref.WRONG
SCORE_VARIANTS = ("half", "no_v2", "filtered_t", "count_before", "uncentred")
M_EFFECTS = 8
UNUSED_EFFECT = (-1, 0, 0, 1)
DUPLICATE = 3             # the effect slot that repeats slot 0: collinear by construction
N_CONTRASTS = 4
DEFINITION_CELLS = 600    # the dense definition of the functionals is computed where T * (N + K) <= this
SCORE_ALL_UP_TO = 16      # the score restatement is compared on every model up to N + K = this ...
SCORE_CAP = 6             # ... and on at most this many models of a group above

GROUPS = list(hard_models.groups())
IDS = ["%dx%d_T%d_B%d" % key for key, _ in GROUPS]


def compared(key, g):
    """The compared models of a group: all of them up to N + K = 16; above, every third plus every model with a state of
    persistence above 1 - 1e-6.  No model is left out for being hard."""
    N, K, T, B = key
    if N + K <= 16:
        return list(range(B))
    return sorted(set(range(0, B, 3)) | {b for b in range(B) if g["phi"][b].max() > 1.0 - 1e-6})


def _opt(g, k, b):
    return None if g[k] is None else g[k][b]


def args(g, b):
    """(obs, phi, q, loadings, obsvar, x0, P0) of model b."""
    return g["obs"][b], g["phi"][b], g["q"][b], g["loadings"][b], _opt(g, "obsvar", b), _opt(g, "x0", b), _opt(g, "P0", b)


def _memo(g, key, make):
    cache = g.setdefault("_cache", {})
    if key not in cache:
        val = make()
        for a in (val.values() if isinstance(val, dict) else val if isinstance(val, (tuple, list)) else (val,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        cache[key] = val
    return cache[key]


def _name(dtype):
    return np.dtype(dtype).name


def oracle_ref(g, b):
    """hard_models.oracle_model of model b (filter and smoother moments of the reference algorithm in fp64)."""
    return _memo(g, ("oracle", b), lambda: hard_models.oracle_model(oracle, g, b))


# ------------------------------------------------------------------------------------------------------- disturbances
def dist(g, b, dtype=np.longdouble, variant=None):
    """(r, ninfo) [T,n] of disturbance_ref.dist_adjoint."""
    return _memo(g, ("dist", b, _name(dtype), variant), lambda: disturbance_ref.dist_adjoint(*args(g, b), variant=variant, dtype=dtype))


def dist_definition(g, b):
    """(mean, var) [T,n] of the smoothed disturbances from the oracle's moments; row 0 NaN."""
    ref = oracle_ref(g, b)
    return _memo(g, ("dist_def", b), lambda: disturbance_ref.dist_definition(g["phi"][b], g["q"][b], ref["F"], ref["Pf"], ref["Xp"],
                                                                             ref["Pp"], ref["S"], ref["Ps"]))


# ---------------------------------------------------------------------------------------------------------- forecasts
def origin(key, b):
    """The fan's origin of record b: runs through -1 .. T - 1 over the records of a group."""
    return (b % (key[2] + 1)) - 1


def track_horizon(key):
    return min(3, key[2])


def ftable(g, b, dtype=np.longdouble, variant=None):
    """(M, S) [T+1,HORIZON,N] of forecast_ref.table; ``variant``: "origin_shift" | "q_once", WRONG on purpose."""
    kw = {} if variant is None else {variant: True}
    return _memo(g, ("ftable", b, _name(dtype), variant), lambda: forecast_ref.table(*args(g, b), hmax=HORIZON, dtype=dtype, **kw))


def forecast(key, g, b, dtype=np.longdouble, variant=None):
    """forecast_ref.forecast of model b as the sweep calls the kernel: HORIZON steps from ``origin``, the track at
    ``track_horizon``, the skill sums from T_FIRST on."""
    tab = ftable(g, b, dtype, variant)
    return _memo(g, ("forecast", b, _name(dtype), variant),
                 lambda: forecast_ref.forecast(*args(g, b), horizon=HORIZON, origin=origin(key, b), track_horizon=track_horizon(key),
                                               t_first=T_FIRST, z=Z95, dtype=dtype, tab=tab))


def truncated_prediction(g, b, o):
    """The second definition of the fan from origin o: the oracle's PREDICTED moments of steps o + 1 .. of the record whose
    steps after o are missing, projected (+ the observation variance).  -> (mean, var [h,N], the oracle's dict), h =
    min(HORIZON, T - 1 - o) rows."""
    T, N = g["obs"][b].shape
    cut = dict(g, obs=g["obs"].copy())
    cut.pop("_cache", None)
    cut["obs"][b, o + 1:] = np.nan
    ref = hard_models.oracle_model(oracle, cut, b, smooth=False)
    Z = ref["Z"]
    R = np.zeros(N) if g["obsvar"] is None else g["obsvar"][b]
    h = min(HORIZON, T - 1 - o)
    Xp, Pp = ref["Xp"][o + 1:o + 1 + h], ref["Pp"][o + 1:o + 1 + h]
    return Xp @ Z.T, np.einsum("jn,tnm,jm->tj", Z, Pp, Z) + R, ref


# ------------------------------------------------------------------------------------------------ observation weights
def targets(g, b, what):
    """The targets of record b, chosen by rule from the record itself so that they differ between records; a rule that finds
    nothing leaves an unused slot (step -1: an all-NaN row).  series [6,2]: an observed cell, a missing cell of a partly
    observed step, a cell of an empty step, t* = 0, t* = T - 1, a never-observed series.  states [3,2]: a common factor, the
    near-unit-root state (persistence above 1 - 1e-6), the last state, each at a step of its own."""
    y, phi = g["obs"][b], g["phi"][b]
    T, N = y.shape
    n = phi.size
    seen = np.isfinite(y)
    unused = (-1, 0)
    if what == "states":
        near = int(np.argmax(phi))
        t = (3 * b + 1) % T
        return np.array([(t, N + b % (n - N)), (min(t + 1, T - 1), near) if phi[near] > 1.0 - 1e-6 else unused, ((5 * b + 2) % T, n - 1)],
                        dtype=np.int64)
    count = seen.sum(1)
    cells = np.argwhere(seen)
    partly = np.argwhere(~seen & ((count > 0) & (count < N))[:, None])
    empty = np.nonzero(count == 0)[0]
    never = np.nonzero(~seen.any(0))[0]
    pick = lambda a: tuple(int(v) for v in a[(7 * b + 3) % len(a)])   # noqa: E731
    tg = [pick(cells) if len(cells) else unused,
          pick(partly) if len(partly) else unused,
          (int(empty[b % len(empty)]), b % N) if len(empty) else unused,
          (0, b % N),
          (T - 1, (b + 1) % N),
          ((2 * b + T // 2) % T, int(never[b % len(never)])) if len(never) else unused]
    return np.array(tg, dtype=np.int64)


def group_targets(g, what):
    """[B,M,2]: the targets of every record of a group."""
    return np.stack([targets(g, b, what) for b in range(g["obs"].shape[0])])


def gains(g, b, dtype=np.longdouble):
    return _memo(g, ("gains", b, _name(dtype)), lambda: weights_ref.gains(*args(g, b), dtype=dtype))


def weights(g, b, what, dtype=np.longdouble, variant=None, record=None):
    """(w [M,T,N], intercept [M]) of weights_ref.weights for the targets of record ``record`` (default: b's own; another one is
    WRONG on purpose, as is ``variant``: "stop_at_target" | "no_c" | "descending")."""
    kw = {} if variant is None else {variant: True}
    tg = targets(g, b if record is None else record, what)
    return _memo(g, ("weights", b, what, _name(dtype), variant, record),
                 lambda: weights_ref.weights(*args(g, b), targets=tg, what=what, dtype=dtype, gain=gains(g, b, dtype), **kw))


def smoothed_at(g, b, what, tg):
    """The oracle's smoothed projection at the targets [M] (NaN at an unused slot): z_j' x_{t*|T} or x_{t*|T,i}."""
    ref = oracle_ref(g, b)
    proj = ref["S"] @ ref["Z"].T if what == "series" else ref["S"]
    return np.array([proj[t, c] if t >= 0 else np.nan for t, c in tg])


def reconstruct(g, b, w, icpt):
    """sum w y + intercept per target, in the arithmetic of (w, intercept)."""
    y = g["obs"][b]
    seen = np.isfinite(y)
    return np.array([(w[m][seen] * y[seen]).sum() + icpt[m] for m in range(w.shape[0])])


# -------------------------------------------------------------------------------------------------------- innovations
def innovations(g, b, dtype=np.longdouble):
    return _memo(g, ("innov", b, _name(dtype)), lambda: innov_ref.innovations(*args(g, b), dtype=dtype))


# -------------------------------------------------------------------------------------------------------------- draws
def draws(g, b, what, first_instance=0):
    """One antithetic pair of draws of model b by draw_ref.draw_model (the oracle's smoother on y* = y - y+), seed
    time_axis.DRAW_SEED, and what its bar is made of: -> dict ``draws [2,T,W]``, ``tol`` = hard_models.draw_tolerance per draw,
    ``ystar [2,T,N]``."""
    def make():
        y, phi, q, G, R, x0, P0 = args(g, b)
        out, parts = draw_ref.draw_model(oracle, y, phi, q, G, 2, time_axis.DRAW_SEED, first_instance + b, what, R, x0, P0,
                                         antithetic=True, parts=True)
        tol = []
        for xp, zx, yp, ystar in parts:
            star = dict(g, obs=g["obs"].copy())
            star.pop("_cache", None)
            star["obs"][b] = ystar
            tol.append(hard_models.draw_tolerance(g, b, hard_models.oracle_model(oracle, star, b, smooth=False), xp, what))
        return dict(draws=out, tol=np.array(tol), ystar=np.array([p[3] for p in parts]))

    return _memo(g, ("draws", b, what, first_instance), make)


# ------------------------------------------------------------------------------------------------ intervention effects
def t_first(b):
    """The first counted step of record b in the regression and the score route: 0 and 1 in turn."""
    return b % 2


def effects(g, b):
    """[8,4] = (series, kind, t0, t1), the effects of record b, chosen by rule from the record itself as ``targets`` chooses (a rule
    that finds nothing leaves an unused slot, series -1): a pulse at an observed cell; a level shift from an observed cell to T; a
    ramp on that series from one step earlier; an exact duplicate of the pulse (slot DUPLICATE: collinear, it must be dropped); a
    level shift on a never-observed series and a pulse at a cell of an empty step (no support); a level shift over the whole
    record on series b % N; a pulse at a missing cell of a partly observed step (no support)."""
    y = g["obs"][b]
    T, N = y.shape
    seen = np.isfinite(y)
    count = seen.sum(1)
    cells = np.argwhere(seen)
    partly = np.argwhere(~seen & ((count > 0) & (count < N))[:, None])
    empty = np.nonzero(count == 0)[0]
    never = np.nonzero(~seen.any(0))[0]
    L, R_ = regress_ref.LEVEL, regress_ref.RAMP
    ef = [UNUSED_EFFECT] * M_EFFECTS
    if len(cells):
        t, j = (int(v) for v in cells[(7 * b + 3) % len(cells)])
        t2, j2 = (int(v) for v in cells[(5 * b + 1) % len(cells)])
        ef[0], ef[1], ef[2], ef[DUPLICATE] = (j, L, t, t + 1), (j2, L, t2, T), (j2, R_, max(t2 - 1, 0), T), (j, L, t, t + 1)
    if len(never):
        ef[4] = (int(never[b % len(never)]), L, 0, T)
    if len(empty):
        e = int(empty[b % len(empty)])
        ef[5] = (b % N, L, e, e + 1)
    ef[6] = (b % N, L, 0, T)
    if len(partly):
        t, j = (int(v) for v in partly[(7 * b + 3) % len(partly)])
        ef[7] = (j, L, t, t + 1)
    return np.array(ef, dtype=np.int64)


def group_effects(g):
    """[B,8,4]: the effects of every record of a group."""
    return np.stack([effects(g, b) for b in range(g["obs"].shape[0])])


def regression(g, b, dtype=np.longdouble, variant=None):
    """regress_ref.regression of model b for ``effects(g, b)`` from ``t_first(b)`` on, over the gains the weights route keeps;
    ``variant``: one of REGRESS_VARIANTS, WRONG on purpose."""
    kw = {} if variant is None else {variant: True}
    return _memo(g, ("regression", b, _name(dtype), variant),
                 lambda: regress_ref.regression(*args(g, b), effects=effects(g, b), t_first=t_first(b), dtype=dtype,
                                                gain=gains(g, b, dtype), **kw))


def regression_usable(g, b):
    """The condition on the INPUTS under which beta and cov of model b are compared: the float64 and the longdouble restatement
    drop the same effects, and no effect that reaches its pivot (the duplicate excepted) has a unit-diagonal pivot within a factor
    100 of regress_ref.MIN_PIVOT -- there the decision itself is a matter of rounding."""
    r64, rl = regression(g, b, np.float64), regression(g, b)
    if not np.array_equal(r64["dropped"], rl["dropped"]):
        return False
    lo, hi = regress_ref.MIN_PIVOT / 100.0, regress_ref.MIN_PIVOT * 100.0
    for r in (r64, rl):
        piv = np.delete(r["pivots"], DUPLICATE)
        if ((piv >= lo) & (piv <= hi)).any():
            return False
    return True


# ---------------------------------------------------------------------------------------------------- window functionals
def windows(key, g, b):
    """[W,4] = (t0, t1, t2, t3) of record b as handed to the kernel; functional_ref.alphas clamps them to [0, T] as the ABI does.
    T >= 4 (W = 9): one step at 0, one at T - 1, the whole record, the first third minus the last third (the gap spans whatever
    empty steps the record has), a range ending at the first observed step, a range starting at the last observed one, a second
    range BEFORE the first, an empty first range (NaN), a range reaching past T.  T <= 3: what fits, as functional_ref.windows."""
    N, K, T, B = key
    if T <= 3:
        w = [(0, 1, 0, 0), (T - 1, T, 0, 0), (0, T, 0, 0), (0, T + 2 + b % 3, 0, 0), (1, 1, 0, 1)]
        if T >= 2:
            w += [(0, 1, 1, 2), (1, 2, 0, 1)] if b % 3 != 1 else [(1, 2, 0, 1), (0, 1, 1, 2)]
        if T >= 3:
            w += [(0, 1, 2, 3), (2, 3, 0, 1 + (b % 2))]
        return np.array(w, dtype=np.int64)
    seen = np.nonzero(np.isfinite(g["obs"][b]).any(1))[0]
    fo, lo = (int(seen[0]), int(seen[-1])) if len(seen) else (0, T - 1)
    h = T // 3
    return np.array([(0, 1, 0, 0), (T - 1, T, 0, 0), (0, T, 0, 0), (0, h, T - h, T), (max(0, fo - 1 - b % 2), fo + 1, 0, 0),
                     (lo, min(T, lo + 2 + b % 2), 0, 0), (T - h, T, b % 2, b % 2 + h), (b % T, b % T, 0, h),
                     (T - 1 - b % 2, T + 5, 0, 0)], dtype=np.int64)


def group_windows(key, g):
    """[B,W,4]: the windows of every record of a group."""
    return np.stack([windows(key, g, b) for b in range(key[3])])


def contrasts(g, b):
    """[4,N] of record b: the unit contrast of series b % N, that of a never-observed series (all zero when every series is
    observed), the group mean 1 / N, a two-series difference."""
    y = g["obs"][b]
    N = y.shape[1]
    never = np.nonzero(~np.isfinite(y).any(0))[0]
    c = np.zeros((N_CONTRASTS, N))
    c[0, b % N] = 1.0
    if len(never):
        c[1, int(never[b % len(never)])] = 1.0
    c[2] = 1.0 / N
    c[3, b % N], c[3, (b + 1) % N] = 1.0, -1.0
    return c


def group_contrasts(g):
    return np.stack([contrasts(g, b) for b in range(g["obs"].shape[0])])


def functional_group(key, g):
    """The hard group as the dict tests/functional_ref.py expects (tests/call_forms.py's: one instance per record, R = B, S = 1,
    no scaling), with a cache of its own; built once per group."""
    cache = g.setdefault("_cache", {})
    if "functional group" not in cache:
        N, K, T, B = key
        cache["functional group"] = dict(N=N, K=K, T=T, R=B, S=1, B=B, scale=None, offset=None, patterns=g["patterns"], _cache={},
                                         **{k: g[k] for k in ("obs", "loadings", "obsvar", "phi", "q", "x0", "P0")})
    return cache["functional group"]


def has_definition(key):
    return key[2] * (key[0] + key[1]) <= DEFINITION_CELLS


def functional_walk(key, g, b, dtype=np.longdouble, variant=None):
    """(mean, var) [W,C] of functional_ref.functional_walk from the oracle's records of model b, for ``group_windows`` and
    ``contrasts``; ``variant``: one of functional_ref.WRONG."""
    def make():
        fg, wins, rows = functional_group(key, g), windows(key, g, b), contrasts(g, b)
        mean, var = np.empty((len(wins), len(rows)), dtype=dtype), np.empty((len(wins), len(rows)), dtype=dtype)
        for w, win in enumerate(wins):
            for k, c in enumerate(rows):
                mean[w, k], var[w, k] = functional_ref.functional_walk(fg, b, win, c, dtype=dtype, wrong=variant)
        return mean, var

    return _memo(g, ("functional walk", b, _name(dtype), variant), make)


def functional_definition(key, g, b):
    """(mean, var) [W,C] in longdouble of functional_ref.functional_definition (dense conditioning of the stacked states, no
    filter and no smoother); only where ``has_definition``."""
    assert has_definition(key)
    return _memo(g, ("functional definition", b),
                 lambda: functional_ref.functional_definition(functional_group(key, g), b, windows(key, g, b), group_contrasts(g)))


def functional_reach(key, g, b):
    """A zeta [W,C] of functional_ref.bars for the windows and contrasts of record b: A = sum_t |alpha_t| (1 or 2; 0 where the
    first range is empty), zeta = || Z'c ||_1 -- what a functional multiplies an error of a smoothed moment by."""
    fg, wins, rows = functional_group(key, g), windows(key, g, b), contrasts(g, b)
    A = np.array([functional_ref.alphas(win, key[2])[1] for win in wins])
    zeta = np.array([float(np.abs(functional_ref.zvector(fg, b, c)).sum()) for c in rows])
    return A[:, None] * zeta[None, :]


def ldl_pivots(g, b):
    """The smallest pivot of the kernel's unpivoted L D L' of Pp_{t+1} = Phi Pf_t Phi + Q over the steps of model b, in float64,
    from the oracle's filtered covariances: what functional_walk_kernel meets (a pivot <= 0 is its MK_FLAG_RANK_DEFICIENT)."""
    def make():
        ref = oracle_ref(g, b)
        phi, q = g["phi"][b], g["q"][b]
        low = np.inf
        for t in range(ref["Pf"].shape[0] - 1):
            A = phi[:, None] * ref["Pf"][t] * phi[None, :] + np.diag(q)
            for j in range(A.shape[0]):
                piv = A[j, j]
                low = min(low, float(piv))
                if piv > 0:
                    l = A[j + 1:, j] / piv
                    A[j + 1:, j + 1:] -= np.outer(l, A[j + 1:, j])
        return low

    return _memo(g, ("ldl pivots", b), make)


# --------------------------------------------------------------------------------------------------------------- scores
def derivs(g, b):
    """(dphi, dq) [n] of model b by Metran's chain rule at dt = 1, as ``scores_alpha``: dphi = phi / alpha^2 with alpha =
    -1 / log(phi), dq = -2 phi dphi c, c = 1 - communality for a series and 1 for a factor -- a near-unit-root state gets its
    true, tiny derivative."""
    phi, G = g["phi"][b], g["loadings"][b]
    alpha = -1.0 / np.log(phi)
    dphi = phi / (alpha * alpha)
    c = np.concatenate([1.0 - (G ** 2).sum(1), np.ones(G.shape[1])])
    return dphi, -2.0 * phi * dphi * c


def group_derivs(g):
    d = [derivs(g, b) for b in range(g["obs"].shape[0])]
    return np.stack([a for a, _ in d]), np.stack([a for _, a in d])


def score_compared(key, g):
    """The models whose scores are compared (the restatement holds [n,n,n] longdouble arrays per cell): every model of
    ``compared`` up to N + K = 16; above, the models with a persistence above 1 - 1e-6, then one model per missingness pattern that
    no model taken so far has (from ``compared`` where it holds one), at most SCORE_CAP per group."""
    N, K, T, B = key
    cmp_ = compared(key, g)
    if N + K <= SCORE_ALL_UP_TO:
        return cmp_
    take = [b for b in range(B) if g["phi"][b].max() > 1.0 - 1e-6][:SCORE_CAP]
    for pat in hard_models.PATTERNS:
        if len(take) >= SCORE_CAP:
            break
        if pat not in {g["patterns"][b] for b in take}:
            cand = [b for b in cmp_ + list(range(B)) if g["patterns"][b] == pat]
            if cand:
                take.append(cand[0])
    return sorted(take)


def score_tape(g, b, dtype=np.longdouble):
    return _memo(g, ("score tape", b, _name(dtype)), lambda: score_ref.base(*args(g, b), dtype=dtype))


def _floored(g, b, res, tape, dtype):
    """``res`` with the scales of score_ref raised to what the prediction's own tangent term contributes.  Under Metran's chain
    rule that term, 2 phi_p dphi_p P_pp + dq_p, CANCELS for a factor whose variance still is the stationary 1 (default P0, no
    observation yet: a "single" record, the first observed step of any record): the score of that parameter is zero in exact
    arithmetic, score_ref's scale -- the absolute values of the terms AFTER the cancellation -- is the rounding noise of the
    arithmetic it ran in (3e-19 in longdouble, exactly 0 in float64), and a difference relative to it means nothing.  The
    expression taken down to its inputs has the two terms apart: per step and parameter
        sum_j z_jp^2 (2 |phi_p dphi_p| P_pp + |dq_p|) (1 / f + v^2 / f^2)   over the cells observed at the step,
    P the filtered covariance of the step before.  A step's scale is the larger of the two, the sums are score_ref.sums' own."""
    dphi, dq = (np.abs(np.asarray(a, dtype=dtype)) for a in derivs(g, b))
    phi = np.abs(np.asarray(g["phi"][b], dtype=dtype))
    Z = weights_ref._Z(np.asarray(g["loadings"][b], dtype=dtype), dtype)
    T = tape["xf"].shape[0]
    steps = np.array(res["scale"]["steps"], dtype=dtype)
    for t in range(T):
        Pd = np.diagonal(tape["P0"] if t == 0 else tape["Pf"][t - 1])
        a = 2 * phi * dphi * np.abs(Pd) + dq
        rf, v = tape["rf"][t], tape["v"][t]
        steps[t] = np.maximum(steps[t], ((Z * Z) * a[None, :] * (rf * (1 + v * v * rf))[:, None]).sum(0))
    _, scale = score_ref.sums(res["score"], steps, res["scale"]["counted"], dtype)
    scale["score"] = np.broadcast_to(steps.max(axis=0) if T else steps.sum(0), steps.shape).copy()
    scale["steps"], scale["counted"] = steps, res["scale"]["counted"]
    return dict(res, scale=scale)


def scores(g, b, dtype=np.longdouble, variant=None):
    """score_ref.scores of model b for ``derivs(g, b)`` from ``t_first(b)`` on, its scales as ``_floored`` has them; ``variant``:
    one of SCORE_VARIANTS."""
    kw = {} if variant is None else {variant: True}
    dphi, dq = derivs(g, b)
    tape = score_tape(g, b, dtype)
    return _memo(g, ("scores", b, _name(dtype), variant),
                 lambda: _floored(g, b, score_ref.scores(*args(g, b), dphi=dphi, dq=dq, t_first=t_first(b), dtype=dtype, tape=tape, **kw),
                                  tape, dtype))


# ----------------------------------------------------- the comparisons of the fitting routes, shared by the CPU and the GPU tier
# Each returns [(name, error, bar)]: the entry of every output that is furthest out in units of its bar; something that must hold
# EXACTLY (a NaN pattern, the support, the dropped set, the count) appears only when it does not, as (name, inf, 0).
def _furthest(diff, bar):
    diff, bar = np.abs(np.asarray(diff, dtype=np.longdouble)).astype(np.float64).ravel(), np.broadcast_to(bar, np.shape(diff)).ravel()
    if diff.size == 0:
        return 0.0, 0.0
    ratio = np.where(bar > 0, diff / np.where(bar > 0, bar, 1.0), np.where(diff > 0, np.inf, 0.0))
    i = int(np.argmax(np.where(np.isnan(ratio), np.inf, ratio)))
    return (float("inf") if np.isnan(diff[i]) else float(diff[i])), float(bar[i])


def regression_checks(got, rl, tol, usable=True):
    """``got``: dict ``normal, support, dropped [M] bool, gain, beta, cov`` of one model; ``rl``: ``regression`` in longdouble;
    ``tol``: hard_models.regression_tolerances; ``usable``: ``regression_usable`` (beta and cov are compared only then)."""
    out = [(k, float("inf"), 0.0) for k in ("support", "dropped") if not np.array_equal(np.asarray(got[k]), rl[k])]
    out.append(("normal",) + _furthest(np.asarray(got["normal"]) - rl["normal"], tol["normal"]))
    out.append(("gain",) + _furthest(got["gain"] - rl["gain"], tol["gain"]))
    if usable and np.array_equal(np.asarray(got["dropped"]), rl["dropped"]):
        kept = ~rl["dropped"]
        for k, sel in (("beta", kept), ("cov", np.outer(kept, kept))):
            gk = np.asarray(got[k])
            if not np.array_equal(np.isnan(gk.astype(np.float64)), ~sel):   # NaN exactly at a dropped effect (its row and column)
                out.append((k + " NaN pattern", float("inf"), 0.0))
            else:
                out.append((k,) + _furthest((gk - rl[k])[sel], tol[k][sel]))
    return out


def functional_checks(got, want, bars):
    """(mean, var) [W,C] of one model against a reference and the pair of bars of hard_models.functional_tolerances; NaN exactly
    where the reference is (an empty first range)."""
    out = []
    for k, a, w, bar in zip(("mean", "var"), got, want, bars):
        a, nan = np.asarray(a), np.isnan(np.asarray(w, dtype=np.float64))
        if not np.array_equal(np.isnan(a.astype(np.float64)), nan):
            out.append((k + " NaN pattern", float("inf"), 0.0))
        else:
            out.append((k,) + _furthest((a - w)[~nan], bar[~nan]))
    return out


def score_checks(got, sl, tol):
    """``got``: dict ``score, grad, count, opg, cusum`` of one model; ``sl``: ``scores`` in longdouble; ``tol``:
    hard_models.score_tolerances, relative to the reference's scales (score_ref.differences)."""
    out = [] if int(got["count"]) == int(sl["count"]) else [("count", float("inf"), 0.0)]
    return out + [(k, v, tol[k]) for k, v in score_ref.differences(got, sl).items()]


# ------------------------------------------------------------------------- float64 against longdouble, per route
def _rel(d, scale):
    scale = np.where(np.asarray(scale, dtype=np.float64) > 0, np.asarray(scale, dtype=np.float64), 1.0)
    d = np.abs(np.asarray(d, dtype=np.longdouble)).astype(np.float64) / scale
    return float(np.nanmax(d)) if np.isfinite(d).any() else 0.0


def fit_gaps(key, g, b, scores_too=True):
    """``restatement_gaps`` of the three fitting routes: {"regress_normal", "regress_beta", "regress_cov", "regress_gain"} relative
    to hard_models.regression_scales (beta and cov also divided by the unit-diagonal condition number of the kept effects, the form
    of their bar; "regress_beta_raw", "regress_cov_raw": not divided, "regress_cond": that number; beta and cov only where
    ``regression_usable``), {"functional_mean", "functional_var"} in units of hard_models.functional_tolerances (nothing is
    measured for that bar: the figure shows what the walk itself loses), and, with ``scores_too``, {"score_score", "score_grad",
    "score_opg", "score_cusum"} relative to score_ref's scales."""
    out = {}
    r64, rl = regression(g, b, np.float64), regression(g, b)
    sc = hard_models.regression_scales(rl)
    out["regress_normal"] = _rel(r64["normal"] - rl["normal"], sc["normal"])
    out["regress_gain"] = _rel(r64["gain"] - rl["gain"], sc["gain"])
    kept = ~rl["dropped"]
    if regression_usable(g, b) and kept.any():
        cond = sc["cond"]
        out["regress_beta_raw"] = _rel((r64["beta"] - rl["beta"])[kept], sc["beta"][kept])
        out["regress_cov_raw"] = _rel((r64["cov"] - rl["cov"])[np.ix_(kept, kept)], sc["cov"][np.ix_(kept, kept)])
        out["regress_beta"], out["regress_cov"] = out["regress_beta_raw"] / cond, out["regress_cov_raw"] / cond
        out["regress_cond"] = cond
    (m64, v64), (ml, vl) = functional_walk(key, g, b, np.float64), functional_walk(key, g, b)
    bm, bv = hard_models.functional_tolerances(g, b, oracle_ref(g, b), functional_reach(key, g, b))
    ok = np.isfinite(ml.astype(np.float64)) & (bm > 0)
    out["functional_mean"] = float((np.abs(m64 - ml).astype(np.float64)[ok] / bm[ok]).max()) if ok.any() else 0.0
    out["functional_var"] = float((np.abs(v64 - vl).astype(np.float64)[ok] / bv[ok]).max()) if ok.any() else 0.0
    if scores_too:
        for k, v in score_ref.differences(scores(g, b, np.float64), scores(g, b)).items():
            out["score_" + k] = v
    return out


def restatement_gaps(key, g, b, fits=False, scores_too=True):
    """What a correct float64 evaluation of each recursion loses on model b: the largest difference between the float64 and
    the longdouble restatement, relative to the scale the route's tolerance function uses -- {"dist_r", "dist_n",
    "forecast_mean", "forecast_var", "weights_series", "weights_states"} and, with ``fits``, those of ``fit_gaps``."""
    top = hard_models._top
    out = {}
    (r64, n64), (rl, nl) = dist(g, b, np.float64), dist(g, b)
    out["dist_r"] = float(np.abs(r64 - rl).max()) / top(rl)
    out["dist_n"] = float(np.abs(n64 - nl).max()) / top(nl)
    (M64, S64), (Ml, Sl) = ftable(g, b, np.float64), ftable(g, b)
    out["forecast_mean"] = float(np.abs(M64 - Ml).max()) / max(top(g["obs"][b]), top(Ml))
    out["forecast_var"] = float(np.abs((S64 - Sl) / Sl).max())
    for what in ("series", "states"):
        (w64, i64), (wl, il) = weights(g, b, what, np.float64), weights(g, b, what)
        worst = 0.0
        for m in range(wl.shape[0]):
            if np.isnan(il[m]):
                continue
            d = abs(float(i64[m] - il[m]))
            if np.isfinite(wl[m]).any():
                d = max(d, float(np.nanmax(np.abs(w64[m] - wl[m]))))
            worst = max(worst, d / top(wl[m]))
        out["weights_" + what] = worst
    if fits:
        out.update(fit_gaps(key, g, b, scores_too))
    return out

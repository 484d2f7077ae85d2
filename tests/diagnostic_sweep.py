"""The property sweep of tests/hard_models.py for the DIAGNOSTIC routes (test infrastructure shared by
tests/test_property_diagnostics.py on the CPU, tests/test_gpu_property_diagnostics.py on the GPU and
scripts/measure_diagnostic_bars.py): which models of a group are compared, the inputs every route derives from the model itself
(weight targets, forecast origins) and the references -- the numpy restatements in ``np.longdouble`` (the yardstick) or
``np.float64`` (what a correct float64 code does), the oracle's moments, the oracle's draws.  Every reference of a model is
computed once and kept with its group (``g["_cache"]``), read-only, so that the routes share a model's gains, forecast table
and oracle moments.
"""
import numpy as np

import disturbance_ref
import draw_ref
import forecast_ref
import hard_models
import innov_ref
import oracle
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


# ------------------------------------------------------------------------- float64 against longdouble, per route
def restatement_gaps(key, g, b):
    """What a correct float64 evaluation of each recursion loses on model b: the largest difference between the float64 and
    the longdouble restatement, relative to the scale the route's tolerance function uses -- {"dist_r", "dist_n",
    "forecast_mean", "forecast_var", "weights_series", "weights_states"}."""
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
    return out

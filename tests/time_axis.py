"""Inputs, mistakes and check functions of the TIME axis (test infrastructure; no GPU, no test functions): record lengths T
chosen for the structure the kernels have along time, not for convenience.

What the kernels tile or pipeline along t (restated below; tests/test_time_axis.py holds each constant to the source text):
  TS = 16      observation tiles through LDS: filter_kernel and filter_wave_kernel (mk_kernels.hip), filter_split_kernel and filter_obs_kernel
               (mk_split.hip).  A tile is loaded one tile ahead with rows clamped to T - 1; the last step of a tile re-reads its
               own row for ``ynext`` and the outer loop supplies the next tile's first row
  PASS = 256   observed_steps_kernel lists the observed steps 256 time steps per pass (four wavefronts' ballots and a prefix)
  TSP = 256    loglik_sparse_kernel (and its record-writing form with fill_gaps_kernel) walks tiles of 256 OBSERVED steps
  WALKERS      the backward walkers and how many steps ahead of use they request their loads: T = 1 is the prologue alone,
               T = 2 one iteration, T = 3 the first iteration that requests as in the steady state

DENSE_LENGTHS follows from TS and the deepest walker: 1, 2, 3; TS - 1, TS, TS + 1; 2 TS, 2 TS + 1.

Dense groups: ``call_forms.shared_group(N, K, T, R=3, S=3, seed)`` -- B = 9 instances (odd: no multiple of the 2, 4 or 16 models
the kernels pack per wavefront or block; (70,3): S = 2) on three records with the patterns "iid", "first", "steps", then EDITED
so that a wrong row at a tile edge cannot hide (``edit_records``):
  * for every tile edge b in {16, 32} with b < T: step b - 1 is fully observed, step b has a mask unlike both neighbours' (an
    alternating one whose parity depends on the record and the edge), and in record (b / 16 - 1) step b is EMPTY -- unless b is
    the last step, which must be observed (next point), so the empty edge step exists at T = 32 and 33 (edge 16) only
  * step T - 1 is observed and step T - 2 has another mask
``MISTAKES`` restates, as edits of the observations, what a kernel with a tile or pipeline bug would read instead;
tests/test_time_axis.py shows that each of them moves every checked quantity of every record by at least call_forms.FACTOR
bars, so tests/test_time_axis_gpu.py would notice.  No bar is new: call_forms.bar for the dense groups,
tests/test_sparse_objective.py's for the sparse records.

Sparse records are built by construction (``SPARSE``): the list of observed steps is given, not drawn."""
import functools
import os

import numpy as np

import call_forms as cf
import oracle
from metran_amd.params import observation_matrix, phi_q_from_alpha
from metran_amd.synthetic import make_dfm

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metran_amd", "csrc")

# ------------------------------------------------------------------------------------------------- restated constants
TS = 16      # observation tile (time steps per LDS refill)
TSP = 256    # tile of observed steps of the sparse walk
PASS = 256   # time steps per pass of observed_steps_kernel

# (what, file, the source line -- matched textually, a comment after it ignored --, how often the file holds it)
SOURCE = (
    ("TS: filter_kernel and filter_wave_kernel", "mk_kernels.hip", "constexpr int TS = %d;" % TS, 2),
    ("TS: filter_split_kernel and filter_obs_kernel", "mk_split.hip", "constexpr int TS = %d;" % TS, 2),
    ("TSP: loglik_sparse_kernel", "mk_kernels.hip", "constexpr int TSP = %d;" % TSP, 1),
    ("PASS: observed_steps_kernel", "mk_kernels.hip", "for (long t0 = 0; t0 < T; t0 += %d) {" % PASS, 1),
)

# backward walker -> (file, loop header, occurrences of the header in the file, steps ahead, the line that requests the load
# furthest ahead (None: the walker loads in the iteration that consumes), occurrences of that line)
_FROM_T2, _FROM_T1 = "for (long t = T - 2; t >= 0; --t) {", "for (long t = T - 1; t >= 0; --t) {"
WALKERS = {
    "smoother_record_kernel": ("mk_kernels.hip", _FROM_T2, 3, 2, "if (t >= 2) issue(xfn);", 2),
    "smoother_blk_kernel": ("mk_kernels.hip", _FROM_T2, 3, 2, "if (t >= 2) issue();", 1),
    "smoother_dense_kernel": ("mk_kernels.hip", _FROM_T2, 3, 1, "if (t >= 1) {", 4),
    "adjoint_kernel (and its LOO mode)": ("mk_kernels.hip", _FROM_T1, 1, 1, "if (t > 0) {", 2),
    "smoother_wave_kernel": ("mk_wide.hip", _FROM_T2, 2, 0, None, 0),
    "smoother_mfma_kernel": ("mk_wide.hip", _FROM_T2, 2, 0, None, 0),
    "smoother_dk_kernel": ("mk_dk.hip", _FROM_T1, 1, 1, "if (t > 0) {", 1),
    "adjoint_wide_kernel": ("mk_split.hip", _FROM_T1, 1, 1, "if (t > 0) load_prev(t - 1);", 1),
    "smoother_generic_kernel": ("mk_generic.hip", _FROM_T2, 1, 0, None, 0),
}


def source_lines(fname):
    return [ln.split("//")[0].strip() for ln in open(os.path.join(CSRC, fname))]


def dense_lengths(ts=TS):
    """Prologue only, one iteration, the first steady-state iteration of the deepest walker; then one step short of a tile, a
    whole tile, one step past it (k TS - 1, k TS, k TS + 1 for k = 1), and two whole tiles and one step past them."""
    depth = max(w[3] for w in WALKERS.values())
    return tuple(range(1, depth + 2)) + (ts - 1, ts, ts + 1, 2 * ts, 2 * ts + 1)


DENSE_LENGTHS = dense_lengths()
EDGES = (TS, 2 * TS)
GENERIC_LENGTHS = (1, 2, TS + 1)
CPU_LENGTHS = (1, 2, TS + 1)   # where the check functions run over the CPU engine

PATTERNS = ("iid", "first", "steps")   # "single" cannot see a tile edge
LOGLIK_WARMUPS = (0, 1)
GRAD_WARMUP = 0                # every step carries weight: a wrong row anywhere reaches the gradient
DRAW_SEED = 29

# shape -> what it exercises
SHAPES = {
    (8, 2): "narrow, even N (16-byte row pieces), four models per wavefront",
    (5, 1): "odd N: scalar row pieces; smoother_blk_kernel",
    (13, 4): "split layout, H = 16, odd N",
    (32, 4): "split layout, H = 32; both tape writers; smoother_dk_kernel; mfma and v1; adjoint_wide_kernel with and without "
             "the update tape; once with wide_filter left at the shipped auto",
    (33, 4): "lane-per-state writer: the WIDE tile path, odd N",
    (60, 4): "a full wavefront",
}
GENERIC_SHAPES = ((8, 2), (70, 3))
LAYOUTS = ("model_major", "time_major")
# route -> the shapes it runs on (every layout, every length of ``lengths``): tests/test_time_axis_gpu.py has one test function
# per route, parametrised with ``params(route)`` and looping over ``lengths(shape, route)``
ROUTES = {
    "filter_smooth": tuple(SHAPES),
    "loglik": tuple(SHAPES),
    "loglik_grad": tuple(SHAPES),
    "simulate_smoothed": tuple(SHAPES),
    "loo_predict": tuple(s for s in SHAPES if cf.has_loo(*s)),
    "draw_smoothed": tuple(SHAPES),
    "generic_family": GENERIC_SHAPES,
}
SEEDS = {}   # (N, K, T) -> seed, where the default draw (0) does not meet tests/test_time_axis.py's sensitivity condition


def lengths(shape, route):
    return GENERIC_LENGTHS if route == "generic_family" else DENSE_LENGTHS


def params(route):
    """(shape, layout) pairs of a route's test function."""
    return [(s, lay) for s in ROUTES[route] for lay in LAYOUTS]


def param_ids(route):
    return ["%dx%d-%s" % (s[0], s[1], lay) for s, lay in params(route)]


# ------------------------------------------------------------------------------------------------------- dense inputs
def _mask(y):
    return np.isfinite(y)


def _edge_mask(N, r, b):
    """Neither full nor empty, and another one per record and per edge."""
    return (np.arange(N) + r + b // TS) % 2 == 0


def _set_mask(y, t, mask, fill):
    y[t] = np.where(mask, np.where(np.isfinite(y[t]), y[t], fill[t]), np.nan)


def edit_records(obs, rng):
    """The edits of the module docstring, on a copy.  ``fill``: values for the cells that become observed."""
    obs = obs.copy()
    R, T, N = obs.shape
    fill = rng.standard_normal(obs.shape)
    for r in range(R):
        y = obs[r]
        if not _mask(y[T - 1]).any():
            _set_mask(y, T - 1, _edge_mask(N, r, 0), fill[r])
        if T >= 2 and np.array_equal(_mask(y[T - 2]), _mask(y[T - 1])):
            _set_mask(y, T - 2, _mask(y[T - 2]) ^ (np.arange(N) == 0), fill[r])
        for b in EDGES:
            if b >= T:
                continue
            _set_mask(y, b - 1, np.ones(N, bool), fill[r])
            empty = r == b // TS - 1 and b < T - 1
            _set_mask(y, b, np.zeros(N, bool) if empty else _edge_mask(N, r, b), fill[r])
            if b + 1 < T:
                m = _mask(y[b + 1])
                if not m.any() or np.array_equal(m, _mask(y[b])):
                    m = ~_edge_mask(N, r, b) | (np.arange(N) == 0)
                    _set_mask(y, b + 1, m, fill[r])
    return obs


def edit_conditions(obs):
    """What ``edit_records`` promises, as a list of violations (empty when all hold)."""
    bad = []
    R, T, N = obs.shape
    for r in range(R):
        m = _mask(obs[r])
        if not m[T - 1].any():
            bad.append((r, "step T-1 is empty"))
        if T >= 2 and np.array_equal(m[T - 2], m[T - 1]):
            bad.append((r, "steps T-2 and T-1 have the same mask"))
        for b in EDGES:
            if b >= T:
                continue
            if not m[b - 1].all():
                bad.append((r, "step %d is not fully observed" % (b - 1)))
            for nb in (b - 1, b + 1):
                if nb < T and np.array_equal(m[nb], m[b]):
                    bad.append((r, "steps %d and %d have the same mask" % (b, nb)))
    for b in EDGES:
        if b < T - 1 and sum(not _mask(obs[r, b]).any() for r in range(R)) != 1:
            bad.append((b, "not exactly one record with an empty step %d" % b))
    return bad


@functools.lru_cache(maxsize=None)
def group(N, K, T):
    """The (shape, length)'s group: drawn once, edited, shared read-only by everything that needs it."""
    S = 2 if N + K > 64 else 3
    seed = SEEDS.get((N, K, T), 0)
    g = cf.shared_group(N, K, T, 3, S, seed, patterns=PATTERNS, usable=lambda pat, y, taken: True)
    obs = edit_records(g["obs"], np.random.default_rng([int(seed), N, K, T, 7]))
    obs.setflags(write=False)
    return cf.variant(g, obs=obs)


@functools.lru_cache(maxsize=None)
def group_plain(N, K, T):
    """... without initial moments, observation variances or scaling: what the CPU engine serves."""
    return cf.variant(group(N, K, T), x0=None, P0=None, obsvar=None, scale=None, offset=None)


# ------------------------------------------------------------------------------------------------------------ mistakes
# name -> f(y [T,N], k) -> (the observations a kernel with that mistake would read, the first affected step) or None where T
# has no such step.  k = 1, 2: the tile edge 16 k.
def _stale_tile(y, k):
    T = len(y)
    if k * TS >= T:
        return None
    out = y.copy()
    out[k * TS:(k + 1) * TS] = y[(k - 1) * TS:(k - 1) * TS + len(out[k * TS:(k + 1) * TS])]
    return out, k * TS


def _edge_row(y, k):
    if k * TS >= len(y):
        return None
    out = y.copy()
    out[k * TS] = y[k * TS - 1]
    return out, k * TS


def _edge_row_back(y, k):
    if k * TS >= len(y):
        return None
    out = y.copy()
    out[k * TS - 1] = y[k * TS]
    return out, k * TS - 1


def _clamp(y, k):
    if k != 1 or len(y) < 2:
        return None
    out = y.copy()
    out[-1] = y[-2]
    return out, len(y) - 1


def _short_walk(y, k):
    if k != 1:
        return None
    out = y.copy()
    out[-1] = np.nan
    return out, len(y) - 1


MISTAKES = {
    "stale tile: tile k reads the rows of tile k-1": _stale_tile,
    "edge row: step 16k reads row 16k-1": _edge_row,
    "edge row, the other way: step 16k-1 reads row 16k": _edge_row_back,
    "clamp: step T-1 reads row T-2": _clamp,
    "short walk: step T-1 is treated as missing": _short_walk,
}


def mistaken(g, name, k):
    """The group with the mistake in every record, or None."""
    made = [MISTAKES[name](y, k) for y in g["obs"]]
    return None if made[0] is None else cf.variant(g, obs=np.stack([m[0] for m in made]))


def sensitivity(g, name, k):
    """{quantity: the smallest distance in bars, over the records, between the reference on the mistaken observations and the
    right one} for every quantity tests/test_time_axis_gpu.py checks; None where T has no such step.  One instance per
    record (the first parameter set): the mistake is in the record."""
    wrong = mistaken(g, name, k)
    if wrong is None:
        return None
    out = {}
    for r in range(g["R"]):
        right, other = cf.reference(g, r, GRAD_WARMUP), cf.reference(wrong, r, GRAD_WARMUP)
        for q in cf.quantities(g["N"], g["K"]):
            d = cf.bars_apart(q, other[q], right[q], g, r)
            out[q] = min(out.get(q, np.inf), d)
    return out


# ----------------------------------------------------------------------------------------------- dense check functions
# Each takes an engine on the group's records: metran_amd.engine.BatchedKalman on the GPU, the CPU engine of
# tests/test_time_axis.py (tests/oracle_engine.py::OracleEngine with the calls it lacks) before that.
def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def check_objective(kf, g, tag=""):
    cf.check_objective(kf, g, LOGLIK_WARMUPS, tag)


def check_gradient(kf, g, tag="", same_forward=True):
    """loglik_grad at GRAD_WARMUP against adjoint_ref, and the two-phase form bit for bit against it."""
    w = GRAD_WARMUP
    got = kf.loglik_grad(g["phi"], g["q"], warmup=w, **cf.init(g))
    cf.check_gradient(got, g, w, tag)
    cf.check_two_phase(lambda p: kf.loglik_forward(p[0], p[1], warmup=w, **cf.init(g)), kf.loglik_backward,
                       lambda p: kf.loglik_grad(p[0], p[1], warmup=w, **cf.init(g)),
                       (g["phi"], g["q"]), (g["phi"] * 0.9, g["q"] * 1.1), "T = %d %s two-phase" % (g["T"], tag), same_forward)
    return got


def check_state(r, g, what, keys=("F", "Pf", "Xp", "Pp", "S", "Ps"), unpack=None):
    """A filter_smooth result: all six records, sigmas, detfs and sigmacount of every instance.  ``unpack``: the engine's
    unpack_sym where the covariances come as packed upper triangles."""
    from metran_amd.engine import FLAG_NONPOSITIVE_F, FLAG_NOT_SPD

    assert not (int(np.bitwise_or.reduce(_np(r["status"]))) & (FLAG_NONPOSITIVE_F | FLAG_NOT_SPD)), what
    got = {k: _np(unpack(r[k]) if unpack is not None and k in ("Pf", "Pp", "Ps") else r[k]) for k in keys + ("mle", "sigmacount", "sigmas", "detfs")}
    for i in range(g["B"]):
        ref = cf.reference(g, i, 1, parts=("state",))
        w, rec, sc = "%s: T = %d, %s" % (what, g["T"], cf._what(g, i)), ref["rec"], ref["sigmacount"]
        cf.assert_close("mle", got["mle"][i], ref["mle"], g, rec, w)
        assert int(got["sigmacount"][i]) == sc, w
        cf.assert_close("sigmas", got["sigmas"][i, :sc], ref["sigmas"][:sc], g, rec, w)
        cf.assert_close("detfs", got["detfs"][i, :sc], ref["detfs"][:sc], g, rec, w)
        if "_rs" in r:   # packed records: the pads of the steps behind the last observed one are zero
            assert not got["sigmas"][i, sc:].any() and not got["detfs"][i, sc:].any(), w
        for k in keys:
            cf.assert_close(k, got[k][i], ref[k], g, rec, w)


def check_projection(outs, g, what):
    """Results of simulate_smoothed / smooth_state_variances: mle, sim_means, sim_vars, S, var of every instance."""
    got = [{k: _np(v) for k, v in o.items() if k in ("mle", "sim_means", "sim_vars", "S", "var")} for o in outs]
    for i in range(g["B"]):
        ref = cf.reference(g, i, 1, parts=("state",))
        w = "%s: T = %d, %s" % (what, g["T"], cf._what(g, i))
        for o in got:
            cf.assert_close("mle", o["mle"][i], ref["mle"], g, ref["rec"], w)
            for k, q in (("sim_means", "sim_means"), ("sim_vars", "sim_vars"), ("S", "S"), ("var", "state_vars")):
                if k in o:
                    cf.assert_close(q, o[k][i], ref[q], g, ref["rec"], w)


def check_loo(r, g, what):
    assert int(np.abs(_np(r["status"]).astype(np.int64)).sum()) == 0, what
    gm, gv = _np(r["loo_means"]), _np(r["loo_vars"])
    for i in range(g["B"]):
        ref = cf.reference(g, i, 0, parts=("loo",))
        seen = np.isfinite(g["obs"][ref["rec"]])
        w = "%s: T = %d, %s" % (what, g["T"], cf._what(g, i))
        assert np.array_equal(np.isnan(gm[i]), ~seen) and np.array_equal(np.isnan(gv[i]), ~seen), w
        cf.assert_close("loo_means", gm[i], ref["loo_means"], g, ref["rec"], w)
        cf.assert_close("loo_vars", gv[i], ref["loo_vars"], g, ref["rec"], w)


def check_draws(kf, g, what_kind, tag=""):
    """draw_smoothed with one antithetic pair against tests/draw_ref.py draw for draw (the draws tier's bar, call_forms.DRAW_TOL).
    T + 1 normals per path: at T = 1 the path is the initial draw and one step."""
    import draw_ref

    out = kf.draw_smoothed(g["phi"], g["q"], 2, seed=DRAW_SEED, what=what_kind, antithetic=True, **cf.init(g))
    assert int(np.abs(_np(out["status"]).astype(np.int64)).sum()) == 0
    got = _np(out["draws"])
    assert got.shape == (2, g["B"], g["T"], g["N"] if what_kind == "series" else g["N"] + g["K"])
    opt = lambda key, j: None if g[key] is None else g[key][j]  # noqa: E731
    for i in range(g["B"]):
        r = i % g["R"]
        want = draw_ref.draw_model(oracle, g["obs"][r], g["phi"][i], g["q"][i], g["loadings"][r], 2, DRAW_SEED, i, what_kind,
                                   opt("obsvar", r), opt("x0", i), opt("P0", i), opt("scale", r), opt("offset", r), antithetic=True)
        err = float(np.abs(got[:, i] - want).max())
        assert err <= cf.DRAW_TOL, "%s draws, T = %d, %s %s: %.3g" % (what_kind, g["T"], cf._what(g, i), tag, err)


# ------------------------------------------------------------------------------------------------------ sparse records
def _all_but(T, dropped):
    keep = np.ones(T, bool)
    keep[list(dropped)] = False
    return np.nonzero(keep)[0]


# name -> (N, K, T, the observed steps); (T, count) pairs around the 256-step pass and the 256-entry tile, observed steps on
# both sides of the wavefront boundary 63|64 and of the pass boundary 255|256
SPARSE = {
    "T256_n255": (5, 1, 256, _all_but(256, [100])),
    "T256_n256": (8, 2, 256, np.arange(256)),
    "T257_n257": (5, 1, 257, np.arange(257)),
    "T513_n256": (8, 2, 513, np.arange(1, 513, 2)),
    "T600_n512": (5, 1, 600, _all_but(600, 5 + 6 * np.arange(88))),
    "T600_n513": (8, 2, 600, _all_but(600, 5 + 6 * np.arange(87))),
    "T300_n257": (5, 1, 300, _all_but(300, 3 + 6 * np.arange(43))),
    # "63, 64, 255, 256 and T - 1" at T = 257: the last step IS step 256
    "T257_straddle": (8, 2, 257, np.array([63, 64, 255, 256])),
    "T40_empty": (5, 1, 40, np.array([], int)),
    "T1": (8, 2, 1, np.array([0])),
}
SPARSE_PAIRS = ((256, 255), (256, 256), (257, 257), (513, 256), (600, 512), (600, 513), (300, 257))
SPARSE_SETS = 13      # parameter sets of the objective (tests/test_sparse_objective.py)
SPARSE_RECORD_SETS = 3


@functools.lru_cache(maxsize=None)
def sparse_record(name):
    """dict: N, K, T, steps, obs [T,N] (a fifth of the cells of the observed steps missing, none of them empty), loadings, and
    the parameter sets of tests/test_sparse_objective.py: phi / q [13,n] (one persistence underflowed to 0), x0, P0, obsvar."""
    N, K, T, steps = SPARSE[name]
    seed = 900 + N + T
    y, alpha, G, _, _ = make_dfm(N, K, T, seed, 0, 0.2, "observed")
    full = make_dfm(N, K, T, seed, 0, 0.0, "observed")[0]
    keep = np.zeros(T, bool)
    keep[steps] = True
    gone = keep & ~np.isfinite(y).any(1)
    y[gone, 0] = full[gone, 0]
    y[~keep] = np.nan
    assert np.array_equal(np.nonzero(np.isfinite(y).any(1))[0], steps)
    rng = np.random.default_rng(T)
    n = N + K
    alphas = alpha[None] * rng.uniform(0.5, 2.0, size=(SPARSE_SETS, n))
    alphas[3, 0] = 1e-5                                     # phi underflows to 0 (Metran's lower bound)
    phi, q = phi_q_from_alpha(alphas, np.repeat(G[None], SPARSE_SETS, 0), 1.0)
    x0 = rng.normal(size=(SPARSE_SETS, n))
    A = rng.normal(size=(SPARSE_SETS, n, n)) * 0.3
    rec = dict(name=name, N=N, K=K, T=T, steps=np.asarray(steps), obs=y, loadings=G, phi=phi, q=q, x0=x0,
               P0=np.eye(n)[None] + A @ A.transpose(0, 2, 1), obsvar=rng.uniform(0.01, 0.3, size=N))
    for v in rec.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return rec


def sparse_reference(rec, s, warmup=1, full=False, obs=None):
    """The oracle's filter of parameter set s on the record (``full``: with x0, P0 and observation variances): dict of sigmas,
    detfs, sigmacount, F, Pf, Xp, Pp, mle."""
    y = rec["obs"] if obs is None else obs
    n = rec["N"] + rec["K"]
    o, oi, oc = oracle.set_observations(y)
    sg, df, sc, F, Pf, Xp, Pp = oracle.seqkalmanfilter(
        o, np.diag(rec["phi"][s]), np.diag(rec["q"][s]), observation_matrix(rec["loadings"]), rec["obsvar"] if full else np.zeros(rec["N"]),
        oi, oc, rec["x0"][s] if full else np.zeros(n), rec["P0"][s] if full else np.eye(n))
    return dict(sigmas=sg, detfs=df, sigmacount=sc, F=F, Pf=Pf, Xp=Xp, Pp=Pp, mle=oracle.get_mle(sg[:sc], df[:sc], oc, warmup))


# the bars of tests/test_sparse_objective.py
def sparse_bar(quantity, ref):
    if quantity == "mle":
        return 1e-10 * max(1.0, abs(float(ref)))
    if quantity in ("F", "Pf", "Xp", "Pp", "detfs"):
        return 1e-10
    if quantity == "sigmas":
        return 1e-10 * np.abs(ref) + 1e-12
    raise KeyError(quantity)


def sparse_bars_apart(quantity, got, ref):
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    return float(np.max(np.abs(got - ref) / sparse_bar(quantity, ref))) if ref.size else 0.0


def _dropped(rec, position):
    """The record without its observed step number ``position``."""
    y = rec["obs"].copy()
    y[rec["steps"][position]] = np.nan
    return y


def _shifted(rec, position):
    """From list position ``position`` on, every observed step reads the row of the NEXT observed step (the last its own)."""
    y, st = rec["obs"].copy(), rec["steps"]
    y[st[position:-1]] = rec["obs"][st[position + 1:]]
    return y


# name -> (applies(rec), the observations a kernel with that mistake would see, the quantities it must move)
SPARSE_MISTAKES = {
    "the 257th observed step dropped": (lambda rec: len(rec["steps"]) >= TSP + 1, lambda rec: _dropped(rec, TSP),
                                        ("mle", "F", "Pf", "Xp", "Pp")),
    "the list shifted by one from position 256 on": (lambda rec: len(rec["steps"]) >= TSP + 2, lambda rec: _shifted(rec, TSP),
                                                     ("mle", "F", "Xp", "sigmas")),
    "step 64 of the straddling record dropped": (lambda rec: rec["name"] == "T257_straddle", lambda rec: _dropped(rec, 1),
                                                 ("mle", "F", "Pf", "Xp", "Pp")),
}


def sparse_sensitivity(rec, name):
    """{quantity: distance in bars between the oracle on the mistaken record and on the right one} (parameter set 0)."""
    applies, form, moved = SPARSE_MISTAKES[name]
    if not applies(rec):
        return None
    right, wrong = sparse_reference(rec, 0, full=True), sparse_reference(rec, 0, full=True, obs=form(rec))
    out = {}
    if "dropped" in name and rec["steps"][TSP if "257th" in name else 1] == rec["T"] - 1:
        moved = tuple(q for q in moved if q not in ("Xp", "Pp"))   # the last step's update reaches no prediction
    for q in moved:
        if q == "sigmas":   # compressed entries: the ones both lists have
            m = min(right["sigmacount"], wrong["sigmacount"])
            out[q] = sparse_bars_apart(q, wrong[q][:m], right[q][:m])
        else:
            out[q] = sparse_bars_apart(q, wrong[q], right[q])
    return out


def check_sparse_objective(kf, rec, full_engine=None):
    """loglik over the 13 parameter sets against the oracle; ``full_engine`` (holding the record WITH observation variances):
    also from given x0 / P0 at warm-up 0, 1 and 3."""
    got = _np(kf.loglik(rec["phi"], rec["q"]))
    assert got.shape == (SPARSE_SETS,)
    for s in range(SPARSE_SETS):
        ref = sparse_reference(rec, s)["mle"]
        assert abs(got[s] - ref) <= 1e-10 * abs(ref) + 1e-10, (rec["name"], s, got[s], ref)
    if full_engine is None:
        return
    for w in (0, 1, 3):
        got = _np(full_engine.loglik(rec["phi"], rec["q"], warmup=w, x0=rec["x0"], P0=rec["P0"]))
        for s in range(SPARSE_SETS):
            ref = sparse_reference(rec, s, w, full=True)["mle"]
            assert abs(got[s] - ref) <= sparse_bar("mle", ref), (rec["name"], "warm-up %d" % w, s, got[s], ref)


def check_sparse_records(results, rec):
    """Results of the record-writing filter (x0, P0, observation variances; the first three parameter sets): all four state
    arrays -- the empty steps' records included --, the compressed entries, sigmacount == the constructed count, zero pads."""
    S, count = SPARSE_RECORD_SETS, len(rec["steps"])
    for s in range(S):
        ref = sparse_reference(rec, s, full=True)
        assert ref["sigmacount"] == count
        for tag, res in results.items():
            what = (rec["name"], tag, s)
            assert int(_np(res["sigmacount"])[s]) == count, what
            for k in ("F", "Pf", "Xp", "Pp"):
                d = sparse_bars_apart(k, _np(res[k])[s], ref[k])
                assert d <= 1.0, what + (k, d)
            sg, df = _np(res["sigmas"])[s], _np(res["detfs"])[s]
            assert sparse_bars_apart("sigmas", sg[:count], ref["sigmas"][:count]) <= 1.0, what
            assert sparse_bars_apart("detfs", df[:count], ref["detfs"][:count]) <= 1.0, what
            assert not sg[count:].any() and not df[count:].any(), what
            assert abs(_np(res["mle"])[s] - ref["mle"]) <= 1e-9 * abs(ref["mle"]), what

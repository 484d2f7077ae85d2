"""References of the window functionals (test infrastructure; no GPU, no test functions): the posterior mean and variance of
``l = sum_t alpha_t c'(scale o Z x_t + offset)``, ``alpha_t = 1/(t1 - t0)`` on ``[t0, t1)`` and ``-1/(t3 - t2)`` on ``[t2, t3)``.

  functional_definition   the DEFINITION: the joint Gaussian of all T states of the record (prior of step 0 = the oracle's
                          Xp[0], Pp[0], later steps from Phi and Q), conditioned on the finite cells with their observation
                          variances by dense linear algebra in numpy longdouble, then a'm and a'Ca.  No filter, no smoother.
  functional_walk         the kernel's recursion from the oracle's F, Pf, S, Ps in a chosen dtype
                              c_t = J_t u_{t+1},  p_t = Ps_t w_t,  var += w_t'(p_t + 2 c_t),  u_t = p_t + c_t,
                          J_t = Pf_t Phi Pp_{t+1}^-1 -- and, by ``wrong=``, the deliberately WRONG variants that
                          tests/test_functionals_host.py shows to be far outside the bars.

Bars (tests/call_forms.py: SMOOTH_ATOL, the tier's 1e-9 on S and Ps): with A = sum_t |alpha_t| (1 or 2) and
zeta = || Z'(c o scale) ||_1,  SMOOTH_ATOL A zeta for the mean and SMOOTH_ATOL (A zeta)^2 for the variance."""
import functools

import numpy as np

import call_forms as cf

LD = np.longdouble
WRONG = ("no_lag", "cross_once", "J_from_Pp_t", "edge_lo", "edge_hi", "no_gap_carry", "second_sign", "scale_once")
# the groups of the GPU tier: (N, K, T); R = 3 records, S = 5 parameter sets (B = 15)
GROUPS = ((5, 1, 33), (8, 2, 1), (8, 2, 2), (8, 2, 3), (8, 2, 17), (13, 4, 17), (32, 4, 3), (60, 4, 3))
EMPTY_STEP = 5      # T >= 17: this step is empty on every record (inside the gap of the difference windows)


@functools.lru_cache(maxsize=None)
def group(N, K, T):
    """``call_forms.shared_group`` with R = 3, S = 5; from T = 17 on step EMPTY_STEP is empty on every record, at T = 3 step 1."""
    g = cf.shared_group(N, K, T, 3, 5, 0, usable=lambda pat, y, taken: True)
    obs = g["obs"].copy()
    if T >= 17:
        obs[:, EMPTY_STEP] = np.nan
    elif T == 3:
        obs[:, 1] = np.nan
    obs.setflags(write=False)
    return cf.variant(g, obs=obs)


def windows(T, R=3):
    """[R,W,4], a different list per record (the edges move with r).  T >= 17: one step at 0, one at T - 1, the whole record, two
    adjacent windows, two overlapping ones, a difference whose gap holds the empty step, one whose ranges touch, one with the
    second range before the first, an empty first range (NaN), a range reaching beyond T (clamped).  T <= 3: what fits."""
    out = []
    for r in range(R):
        if T >= 17:
            w = [(0, 1, 0, 0), (T - 1, T, 0, 0), (0, T, 0, 0), (2 + r, 6, 0, 0), (6, 9 + r, 0, 0), (3, 10 + r, 0, 0), (7 + r, 14, 0, 0),
                 (1 + r, 4, 8, 12 + r), (2, 5 + r, 5 + r, 9), (10 + r, 14, 3, 7), (4, 4, 0, 3), (T - 3 - r, T + 5, 0, 0), (-2, 2 + r, 0, 0)]
        else:
            w = [(0, 1, 0, 0), (T - 1, T, 0, 0), (0, T, 0, 0), (0, T + 2 + r, 0, 0), (1, 1, 0, 1)]
            if T >= 2:
                w += [(0, 1, 1, 2), (1, 2, 0, 1)] if r != 1 else [(1, 2, 0, 1), (0, 1, 1, 2)]
            if T >= 3:
                w += [(0, 1, 2, 3), (2, 3, 0, 1 + (r % 2))]
        out.append(w)
    return np.array(out, dtype=np.int64)


def contrasts(g, kind):
    """[R,C,N] or None: "unit" (None), "one" (C = 1), "mixed" (a two-well difference, an all-zero contrast, a group mean, a random
    one), "full" (C = 64 random)."""
    if kind == "unit":
        return None
    R, N = g["R"], g["N"]
    rng = np.random.default_rng([N, g["K"], 91])
    if kind == "one":
        return rng.normal(size=(R, 1, N))
    if kind == "full":
        return rng.normal(size=(R, 64, N))
    c = np.zeros((R, 4, N))
    for r in range(R):
        c[r, 0, r % N], c[r, 0, (r + 2) % N] = 1.0, -1.0
        c[r, 2, :] = 1.0 / N
        c[r, 3] = rng.normal(size=N)
    return c


# ------------------------------------------------------------------------------------------------------------------ pieces
def alphas(window, T, dtype=np.float64, wrong=None):
    """(alpha [T] or None for an empty first range, A = sum |alpha_t|) of a window, its ranges clamped to [0, T]."""
    t0, t1, t2, t3 = (int(min(max(v, 0), T)) for v in window)
    if t1 <= t0:
        return None, 0.0
    if wrong == "edge_lo":
        t0 = t0 + 1 if t1 - t0 > 1 else max(t0 - 1, 0)
        t1 = max(t1, t0 + 1)
    if wrong == "edge_hi":
        t1 = t1 - 1 if t1 - t0 > 1 else min(t1 + 1, T)
        t0 = min(t0, t1 - 1)
    a = np.zeros(T, dtype=dtype)
    a[t0:t1] += dtype(1) / dtype(t1 - t0)
    if t3 > t2:
        a[t2:t3] += (dtype(1) if wrong == "second_sign" else -dtype(1)) / dtype(t3 - t2)
    return a, (2.0 if t3 > t2 else 1.0)


def _model(g, i, rec=None):
    r = int(i % g["R"] if rec is None else rec)
    N = g["N"]
    Z = np.concatenate([np.eye(N), g["loadings"][r]], axis=1)
    scale = np.ones(N) if g["scale"] is None else g["scale"][r]
    offset = np.zeros(N) if g["offset"] is None else g["offset"][r]
    return r, Z, scale, offset


def zvector(g, i, c, rec=None):
    """Z'(c o scale) of instance i's record."""
    _, Z, scale, _ = _model(g, i, rec)
    return Z.T @ (np.asarray(c, float) * scale)


def bars(g, i, window, c):
    """(bar of the mean, bar of the variance) of a functional."""
    _, A = alphas(window, g["T"])
    zeta = float(np.abs(zvector(g, i, c)).sum())
    return cf.SMOOTH_ATOL * A * zeta, cf.SMOOTH_ATOL * (A * zeta) ** 2


def contrast_rows(g, i, table):
    """The [C,N] contrasts of instance i: its record's rows of ``table``, or the N unit contrasts."""
    return np.eye(g["N"]) if table is None else np.asarray(table)[i % g["R"]]


# -------------------------------------------------------------------------------------------------------------- definition
def _cholesky(S):
    L = np.array(S, dtype=LD)
    m = L.shape[0]
    for j in range(m):
        L[j, j] = np.sqrt(L[j, j])
        L[j + 1:, j] /= L[j, j]
        L[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
    return np.tril(L)


def _chol_solve(L, B):
    X = np.array(B, dtype=LD)
    m = L.shape[0]
    for j in range(m):
        X[j] /= L[j, j]
        X[j + 1:] -= np.outer(L[j + 1:, j], X[j])
    for j in range(m - 1, -1, -1):
        X[j] /= L[j, j]
        X[:j] -= np.outer(L[j, :j], X[j])
    return X


def posterior(g, i):
    """(mean [T*n], covariance [T*n, T*n]) in longdouble of the stacked states of instance i given its record.  Kept with the group."""
    key = ("functional posterior", i)
    if key in g["_cache"]:
        return g["_cache"][key]
    T, n = g["T"], g["N"] + g["K"]
    r, Z, _, _ = _model(g, i)
    ref = cf.reference(g, i, 0, parts=("state",))
    phi, q = g["phi"][i].astype(LD), g["q"][i].astype(LD)
    m = np.empty((T, n), dtype=LD)
    Cd = np.empty((T, n, n), dtype=LD)
    m[0], Cd[0] = ref["Xp"][0].astype(LD), ref["Pp"][0].astype(LD)
    for t in range(1, T):
        m[t] = phi * m[t - 1]
        Cd[t] = phi[:, None] * Cd[t - 1] * phi[None, :] + np.diag(q)
    C = np.empty((T, n, T, n), dtype=LD)
    for t in range(T):
        blk = Cd[t]
        for s in range(t, T):
            C[t, :, s, :] = blk.T        # Cov(x_t, x_s) = C_tt Phi^(s-t)
            C[s, :, t, :] = blk          # Cov(x_s, x_t) = Phi^(s-t) C_tt
            blk = phi[:, None] * blk
    C = C.reshape(T * n, T * n)
    mv = m.reshape(-1)
    y = g["obs"][r]
    cells = [(t, j) for t in range(T) for j in range(g["N"]) if np.isfinite(y[t, j])]
    if cells:
        H = np.zeros((len(cells), T * n), dtype=LD)
        for k, (t, j) in enumerate(cells):
            H[k, t * n:(t + 1) * n] = Z[j]
        Rv = np.zeros(g["N"]) if g["obsvar"] is None else g["obsvar"][r]
        CH = C @ H.T
        S = H @ CH + np.diag(np.array([Rv[j] for _, j in cells], dtype=LD))
        L = _cholesky(S)
        resid = np.array([y[t, j] for t, j in cells], dtype=LD) - H @ mv
        X = _chol_solve(L, np.concatenate([CH.T, resid[:, None]], axis=1))
        mv = mv + CH @ X[:, -1]
        C = C - CH @ X[:, :-1]
    g["_cache"][key] = (mv, C)
    return g["_cache"][key]


def weights_vector(g, i, window, c):
    """The vector a [T*n] (longdouble) with l = a'x + const, and const; None for an empty first range."""
    T = g["T"]
    al, _ = alphas(window, T, dtype=LD)
    if al is None:
        return None, None
    _, Z, scale, offset = _model(g, i)
    z = Z.T.astype(LD) @ (np.asarray(c, dtype=LD) * scale.astype(LD))
    return np.outer(al, z).reshape(-1), al.sum() * (np.asarray(c, dtype=LD) @ offset.astype(LD))


def functional_definition(g, i, wins, table):
    """(mean, var) [W,C] in longdouble of instance i for the windows [W,4] and the contrasts (``contrast_rows``); NaN where the
    first range is empty."""
    mv, C = posterior(g, i)
    rows = contrast_rows(g, i, table)
    mean = np.full((len(wins), len(rows)), np.nan, dtype=LD)
    var = np.full((len(wins), len(rows)), np.nan, dtype=LD)
    for w, win in enumerate(wins):
        for k, c in enumerate(rows):
            a, const = weights_vector(g, i, win, c)
            if a is not None:
                mean[w, k], var[w, k] = a @ mv + const, a @ (C @ a)
    return mean, var


# -------------------------------------------------------------------------------------------------------------------- walk
def _solve(A, b, dtype):
    """A^-1 b by Gaussian elimination with partial pivoting in ``dtype`` (numpy.linalg has no longdouble)."""
    A, b = np.array(A, dtype=dtype), np.array(b, dtype=dtype)
    n = len(b)
    for j in range(n):
        p = j + int(np.argmax(np.abs(A[j:, j])))
        if p != j:
            A[[j, p]], b[[j, p]] = A[[p, j]], b[[p, j]]
        f = A[j + 1:, j] / A[j, j]
        A[j + 1:] -= np.outer(f, A[j])
        b[j + 1:] -= f * b[j]
    for j in range(n - 1, -1, -1):
        b[j] = (b[j] - A[j, j + 1:] @ b[j + 1:]) / A[j, j]
    return b


def functional_walk(g, i, window, c, dtype=np.float64, wrong=None, rec=None, state=None):
    """(mean, var) of one functional by the kernel's recursion from the oracle's records of instance i, in ``dtype``.  ``wrong``:
    one of WRONG.  ``rec`` / ``state``: the record whose loadings, scale and offset are used / the instance whose smoothed and
    filtered records are walked, where they are NOT i % R / i (deliberately wrong pairings)."""
    T = g["T"]
    al, _ = alphas(window, T, dtype=dtype, wrong=wrong)
    if al is None:
        return dtype(np.nan), dtype(np.nan)
    _, Z, scale, offset = _model(g, i, rec)
    st = cf.reference(g, i if state is None else state, 0, parts=("state",))
    F, Pf, S, Ps, Pp = (st[k].astype(dtype) for k in ("F", "Pf", "S", "Ps", "Pp"))
    j = i if state is None else state
    phi, q = g["phi"][j].astype(dtype), g["q"][j].astype(dtype)
    c = np.asarray(c, dtype=dtype)
    z = Z.T.astype(dtype) @ (c * scale.astype(dtype))
    zv = Z.T.astype(dtype) @ c if wrong == "scale_once" else z      # the variance with the scale applied once: z (scaled) x z (not)
    on = np.nonzero(al)[0]
    tlo, thi = int(on.min()), int(on.max()) + 1
    mean = al.sum() * (c @ offset.astype(dtype))
    var = dtype(0)
    u = np.zeros(len(z), dtype=dtype)
    for t in range(thi - 1, tlo - 1, -1):
        w, wv = al[t] * z, al[t] * zv
        mean = mean + w @ S[t]
        ct = np.zeros(len(z), dtype=dtype)
        if t < thi - 1 and wrong != "no_lag":
            P1 = Pp[t] if wrong == "J_from_Pp_t" else phi[:, None] * Pf[t] * phi[None, :] + np.diag(q)
            ct = Pf[t] @ (phi * _solve(P1, u, dtype))
            if wrong == "no_gap_carry" and al[t] == 0:
                ct = np.zeros(len(z), dtype=dtype)
        p = Ps[t] @ wv
        var = var + w @ (p + (1 if wrong == "cross_once" else 2) * ct)
        u = p + ct
    return mean, (var if var > 0 else dtype(0))

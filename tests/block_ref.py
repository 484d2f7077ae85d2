"""References of the leave-block-out predictions (test infrastructure; no GPU, no test functions): for a block I = the observed
cells of one series on the steps [t0, t1), E[y_I | every observation except I], its covariance V, quad = (y_I - E)'V^-1(y_I - E),
log det V and 1'V1.

  definition   the DEFINITION: the joint Gaussian of the observed data vector of the record (the joint prior of the states built as
               ``functional_ref.posterior`` builds it: step 0 from the oracle's Xp[0], Pp[0], later steps from Phi and Q; then
               mu = H m, Sigma = H C H' + diag(obsvar)), conditioned on everything outside the block by dense linear algebra in
               numpy longdouble.  No filter, no smoother, no precision matrix.
  recursion    the kernels' recursion in a chosen dtype: a sequential filter (prediction first, the observed series of the step
               ascending) gives d = P z', 1/f and v per cell; one backward walk of (r, N) with a checkpoint behind every step; per
               block the walk of its steps with the vectors omega_c, then the solve of the unit-diagonal M_II -- and, by ``wrong=``,
               the deliberately WRONG variants that tests/test_block_host.py shows to be far outside the bars.

Both return, per block, a dict: means [L], vars [L] (caller's units, NaN where the cell is not observed or beyond t1), m, quad,
logdet, ovo (= 1'V1 / m^2 * scale^2), kappa (the condition number of the unit-diagonal M_II; definition only) and minpiv (the
smallest pivot of the unit-diagonal Cholesky; recursion only).  An unused slot (series < 0) gives None.

The bar (``bars``): the LOO tier's flat bar -- LOO_TOL * big for the means, LOO_TOL * big^2 for the variances, with big = max(1,
largest modulus of the reference's means), quad and logdet relative to max(1, m) -- plus BAR_SAFETY * MU * kappa * eps * scale
(scale^2 for the variances, 1 for quad and logdet, which carry no units).  MU is measured on the CPU
(tests/test_block_host.py::test_restatement_against_definition prints it): the largest (float64 recursion - definition) /
(kappa * eps * scale) over every group, record and block of the tier; BAR_SAFETY = 4 is the allowance the diagnostics tier gives
the kernels' tree-order fused sums."""
import functools

import numpy as np

import call_forms as cf
import functional_ref as fr

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
MIN_PIVOT = 1e-12          # metran_amd/csrc/regress_kernels.h: regress_min_pivot
MAX_CELLS = 64             # mk_block_max_cells()
MU = 1100.0               # measured: tests/test_block_host.py prints it (the largest value there is 1016)
BAR_SAFETY = 4.0
WRONG = ("omega_gap", "omega_own_cell", "checkpoint_early", "checkpoint_late", "msc_sign", "edge_lo", "edge_hi", "keep_obsvar",
         "scale_once", "record_div", "neighbour_checkpoint")
# the groups of the GPU tier: (N, K, T); R = 3 records, S = 5 parameter sets (B = 15)
GROUPS = ((5, 1, 70), (8, 2, 1), (8, 2, 2), (8, 2, 3), (8, 2, 17), (13, 4, 17), (32, 4, 3), (60, 4, 3))
EMPTY_STEP = 5


@functools.lru_cache(maxsize=None)
def group(N, K, T):
    """``call_forms.shared_group`` with R = 3, S = 5, given x0 / P0, observation variances, scale and offset.  From T = 17 on
    step EMPTY_STEP is empty on every record (at T = 3 step 1) and the last series is never observed; at (5,1), T = 70 record 1
    is fully observed (its block of 64 cells)."""
    g = cf.shared_group(N, K, T, 3, 5, 0, usable=lambda pat, y, taken: True)
    obs = g["obs"].copy()
    if T == 70:
        rng = np.random.default_rng([N, K, T, 7])
        fill = rng.normal(size=obs[1].shape)
        obs[1] = np.where(np.isfinite(obs[1]), obs[1], fill)
    if T >= 17:
        obs[:, EMPTY_STEP] = np.nan
        obs[:, :, N - 1] = np.nan
    elif T == 3:
        obs[:, 1] = np.nan
    if T == 70:
        obs[1, EMPTY_STEP] = fill[EMPTY_STEP]
        obs[1, :, N - 1] = fill[:, N - 1]
    obs.setflags(write=False)
    return cf.variant(g, obs=obs)


def blocks(g):
    """[R,W,3] = (series, t0, t1), a different list per record (the edges and the series move with r): t0 = 0, t1 = T, the whole
    record where T <= 64, a block with the empty step inside, a block without an observed cell, a block on the never-observed
    series, two blocks sharing t1 on different series, overlapping blocks on one series, one-cell blocks, an unused slot; at T = 70
    a block of exactly 64 steps."""
    N, T, R = g["N"], g["T"], g["R"]
    out = []
    for r in range(R):
        a, b = r % N, (r + 2) % N
        if T >= 17:
            w = [(a, 0, 3 + r), (b, T - 4 - r, T), (a, 0, min(T, 64)), (b, 3, 9 + r), (a, EMPTY_STEP, EMPTY_STEP + 1), (N - 1, 2, 12),
                 (a, 6, 11), (b, 8 + r, 11), (a, 8, 14), (-1, 0, 0), (b, 7, 8), (a, T - 1, T), (b, 0, 1)]
            if T == 70:
                w += [((r + 1) % (N - 1), 3, 67), (a, 30, 55 + r)]
        else:
            w = [(a, 0, 1), (b, T - 1, T), (a, 0, T), (-1, 0, 0), (b, 0, T), (N - 1, 0, T)]
            if T >= 2:
                w += [(a, 1, 2), (b, 0, 2)]
            if T >= 3:
                w += [(a, 1, 3), (b, 1, 2)]
        if r == 1:
            w = w[::-1]
        out.append(w)
    return np.array(out, dtype=np.int64)


def _model(g, i, rec=None):
    r, Z, scale, offset = fr._model(g, i, rec)
    Rv = np.zeros(g["N"]) if g["obsvar"] is None else g["obsvar"][r]
    return r, Z, scale, offset, Rv


# -------------------------------------------------------------------------------------------------------------- definition
def joint(g, i):
    """(cells, mu, Sigma) of the observed data vector of instance i in longdouble; cells = [(t, j)] in filter order."""
    key = ("block joint", i)
    if key in g["_cache"]:
        return g["_cache"][key]
    T, n = g["T"], g["N"] + g["K"]
    r, Z, _, _, Rv = _model(g, i)
    ref = cf.reference(g, i, 0, parts=("state",))
    phi, q = g["phi"][i].astype(LD), g["q"][i].astype(LD)
    m = np.empty((T, n), dtype=LD)
    Cd = np.empty((T, n, n), dtype=LD)
    m[0], Cd[0] = ref["Xp"][0].astype(LD), ref["Pp"][0].astype(LD)
    for t in range(1, T):
        m[t] = phi * m[t - 1]
        Cd[t] = phi[:, None] * Cd[t - 1] * phi[None, :] + np.diag(q)
    y = g["obs"][r]
    cells = [(t, j) for t in range(T) for j in range(g["N"]) if np.isfinite(y[t, j])]
    ZL = Z.astype(LD)
    # Cov(y_s, y_c) = z_s Cov(x_ts, x_tc) z_c': Cov(x_t, x_u) = C_tt Phi^(u - t) for u >= t
    steps = sorted({t for t, _ in cells})
    ZC = {}
    for t in steps:
        blk = Cd[t]
        for u in range(t, T):
            ZC[t, u] = ZL @ blk.T @ ZL.T if u == t else ZL @ (blk.T @ ZL.T)    # [N, N]: rows series at t, cols series at u
            blk = phi[:, None] * blk
    M = len(cells)
    Sig = np.zeros((M, M), dtype=LD)
    for a, (t, j) in enumerate(cells):
        for b in range(a, M):
            u, k = cells[b]
            Sig[a, b] = Sig[b, a] = ZC[t, u][j, k]
        Sig[a, a] += LD(Rv[j])
    mu = np.array([ZL[j] @ m[t] for t, j in cells], dtype=LD)
    g["_cache"][key] = (cells, mu, Sig)
    return g["_cache"][key]


def _unit_kappa(Mii):
    sd = np.sqrt(np.diag(Mii))
    A = (Mii / np.outer(sd, sd)).astype(np.float64)
    ev = np.linalg.eigvalsh(A)
    return float(ev[-1] / max(ev[0], 1e-300))


def definition(g, i, blk):
    """The block ``blk`` = (series, t0, t1) of instance i by dense conditioning in longdouble."""
    js, t0, t1 = (int(v) for v in blk)
    if js < 0:
        return None
    key = ("block definition", i, js, t0, t1)
    if key in g["_cache"]:
        return g["_cache"][key]
    r, Z, scale, offset, Rv = _model(g, i)
    cells, mu, Sig = joint(g, i)
    L = t1 - t0
    out = dict(means=np.full(L, np.nan, dtype=LD), vars=np.full(L, np.nan, dtype=LD), m=0, quad=LD(np.nan), logdet=LD(np.nan),
               ovo=LD(np.nan), kappa=1.0, V=None)
    inb = np.array([j == js and t0 <= t < t1 for t, j in cells], dtype=bool)
    m = int(inb.sum())
    out["m"] = m
    if m:
        I, O = np.nonzero(inb)[0], np.nonzero(~inb)[0]
        y = np.array([g["obs"][r][t, j] for t, j in cells], dtype=LD)
        E, V = mu[I].copy(), Sig[np.ix_(I, I)].copy()
        if len(O):
            Lc = fr._cholesky(Sig[np.ix_(O, O)])
            X = fr._chol_solve(Lc, np.concatenate([Sig[np.ix_(O, I)], (y[O] - mu[O])[:, None]], axis=1))
            E = E + Sig[np.ix_(I, O)] @ X[:, -1]
            V = V - Sig[np.ix_(I, O)] @ X[:, :-1]
        Lv = fr._cholesky(V)
        e = y[I] - E
        w = fr._chol_solve(Lv, e[:, None])[:, 0]
        sc, of = LD(scale[js]), LD(offset[js])
        pos = np.array([cells[k][0] - t0 for k in I])
        out["means"][pos] = E * sc + of
        out["vars"][pos] = np.maximum(np.diag(V) - LD(Rv[js]), 0) * sc * sc
        out["quad"] = e @ w
        out["logdet"] = 2 * np.log(np.diag(Lv)).sum()
        out["ovo"] = V.sum() / LD(m) ** 2 * sc * sc
        Mii = fr._chol_solve(Lv, np.eye(m, dtype=LD))
        out["kappa"] = _unit_kappa(Mii)
        out["V"] = V
    g["_cache"][key] = out
    return out


def bars(g, i, blk, ref, safety=BAR_SAFETY):
    """dict of the bars of means, vars, quad, logdet, ovo around the definition ``ref`` of the block."""
    r, _, scale, _, _ = _model(g, i)
    sc = float(scale[int(blk[0])])
    fin = np.isfinite(ref["means"].astype(float))
    big = max(1.0, float(np.abs(ref["means"][fin].astype(float)).max())) if fin.any() else 1.0
    cond = safety * MU * ref["kappa"] * EPS
    mm = max(1, ref["m"])
    return dict(means=cf.LOO_TOL * big + cond * sc, vars=cf.LOO_TOL * big ** 2 + cond * sc ** 2, quad=(cf.LOO_TOL + cond) * mm,
                logdet=(cf.LOO_TOL + cond) * mm, ovo=cf.LOO_TOL * big ** 2 + cond * sc ** 2)


def distance(got, ref, bar):
    """The largest |got - ref| / bar over (means, vars, quad, logdet, ovo); NaN on one side only counts as infinitely far."""
    worst = 0.0
    for k in ("means", "vars", "quad", "logdet", "ovo"):
        a, b = np.atleast_1d(np.asarray(got[k], dtype=LD)), np.atleast_1d(np.asarray(ref[k], dtype=LD))
        if (np.isnan(a) != np.isnan(b)).any():
            return np.inf
        ok = ~np.isnan(b)
        if ok.any():
            worst = max(worst, float(np.abs(a[ok] - b[ok]).max() / bar[k]))
    if got["m"] != ref["m"]:
        return np.inf
    return worst


# --------------------------------------------------------------------------------------------------------------- recursion
def filter_tape(g, i, dtype=np.float64, rec=None):
    """(d [T,N,n], rf [T,N], v [T,N]) of the sequential filter of instance i: zeros at the cells that are not observed."""
    key = ("block tape", i, np.dtype(dtype).name, rec)
    if key in g["_cache"]:
        return g["_cache"][key]
    T, N, n = g["T"], g["N"], g["N"] + g["K"]
    r, Z, _, _, Rv = _model(g, i, rec)
    Z = Z.astype(dtype)
    phi, q = g["phi"][i].astype(dtype), g["q"][i].astype(dtype)
    x = np.zeros(n, dtype) if g["x0"] is None else g["x0"][i].astype(dtype)
    P = np.eye(n, dtype=dtype) if g["P0"] is None else g["P0"][i].astype(dtype)
    d, rf, v = np.zeros((T, N, n), dtype), np.zeros((T, N), dtype), np.zeros((T, N), dtype)
    y = g["obs"][r]
    for t in range(T):
        x = phi * x
        P = phi[:, None] * P * phi[None, :] + np.diag(q)
        for j in range(N):
            if not np.isfinite(y[t, j]):
                continue
            dd = P @ Z[j]
            f = Z[j] @ dd + dtype(Rv[j])
            vv = dtype(y[t, j]) - Z[j] @ x
            d[t, j], rf[t, j], v[t, j] = dd, 1 / f, vv
            k = dd / f
            x = x + k * vv
            P = P - np.outer(k, dd)
    g["_cache"][key] = (d, rf, v)
    return g["_cache"][key]


def _cell(Z, j, d, rf, v, r, Nm):
    """One cell of the backward walk: (k, g, u_s, M_ss, r, N)."""
    k = d * rf
    gg = Nm @ k
    us = v * rf - k @ r
    mss = rf + k @ gg
    z = Z[j]
    r = r + z * us
    Nm = Nm - np.outer(z, gg) - np.outer(gg, z) + mss * np.outer(z, z)
    return k, gg, us, mss, r, Nm


def checkpoints(g, i, dtype=np.float64, rec=None):
    """(r [T+1,n], N [T+1,n,n]): the walk's state behind step t (everything at the steps >= t taken, the pull-back of step t
    included); zeros at t = T."""
    key = ("block checkpoints", i, np.dtype(dtype).name, rec)
    if key in g["_cache"]:
        return g["_cache"][key]
    T, N, n = g["T"], g["N"], g["N"] + g["K"]
    _, Z, _, _, _ = _model(g, i, rec)
    Z = Z.astype(dtype)
    d, rf, v = filter_tape(g, i, dtype, rec)
    phi = g["phi"][i].astype(dtype)
    cr, cN = np.zeros((T + 1, n), dtype), np.zeros((T + 1, n, n), dtype)
    r, Nm = np.zeros(n, dtype), np.zeros((n, n), dtype)
    for t in range(T - 1, -1, -1):
        for j in range(N - 1, -1, -1):
            _, _, _, _, r, Nm = _cell(Z, j, d[t, j], rf[t, j], v[t, j], r, Nm)
        r, Nm = phi * r, phi[:, None] * Nm * phi[None, :]
        cr[t], cN[t] = r, Nm
    g["_cache"][key] = (cr, cN)
    return g["_cache"][key]


def recursion(g, i, blk, dtype=np.float64, wrong=None, neighbour=None):
    """The block ``blk`` of instance i by the kernels' recursion in ``dtype``.  ``wrong``: one of WRONG (``neighbour``: the t1 of
    the block whose checkpoint "neighbour_checkpoint" takes)."""
    js, t0, t1 = (int(v) for v in blk)
    if js < 0:
        return None
    T, N, n = g["T"], g["N"], g["N"] + g["K"]
    rec = (i // g["S"]) % g["R"] if wrong == "record_div" else None
    r_, Z, scale, offset, Rv = _model(g, i, rec)
    Z = Z.astype(dtype)
    d, rf, v = filter_tape(g, i, dtype, rec)
    cr, cN = checkpoints(g, i, dtype, rec)
    phi = g["phi"][i].astype(dtype)
    y = g["obs"][r_]
    L = t1 - t0
    lo, hi = t0, t1
    if wrong == "edge_lo":
        lo = t0 + 1 if L > 1 else max(t0 - 1, 0)
    if wrong == "edge_hi":
        hi = t1 - 1 if L > 1 else min(t1 + 1, T)
    lo, hi = min(lo, hi - 1), max(hi, lo + 1)
    at = hi
    if wrong == "checkpoint_early":
        at = min(hi + 1, T)
    if wrong == "checkpoint_late":
        at = max(hi - 1, 0)
    if wrong == "neighbour_checkpoint" and neighbour is not None:
        at = int(neighbour)
    r, Nm = cr[at].copy(), cN[at].copy()
    om, us_, idx = {}, {}, []              # omega_c, u_c of the block cells passed; their steps, latest first
    Mrow = {}
    for t in range(hi - 1, lo - 1, -1):
        for j in range(N - 1, -1, -1):
            if rf[t, j] == 0:
                continue
            k, gg, us, mss, r, Nm = _cell(Z, j, d[t, j], rf[t, j], v[t, j], r, Nm)
            for c in idx:
                msc = -(k @ om[c])
                if wrong == "msc_sign":
                    msc = -msc
                om[c] = om[c] + Z[j] * msc
                if j == js:
                    Mrow[t, c] = msc
            if j == js:
                om[t] = mss * Z[j] - gg
                if wrong == "omega_own_cell":
                    om[t] = om[t] + Z[j] * (-(k @ om[t]))
                us_[t] = us
                Mrow[t, t] = mss
                idx.append(t)
        seen = np.isfinite(y[t]).any()
        for c in idx:
            if wrong == "omega_gap" and not seen:
                continue
            om[c] = phi * om[c]
        r, Nm = phi * r, phi[:, None] * Nm * phi[None, :]
    steps = sorted(idx)
    m = len(steps)
    Lout = max(L, hi - lo)
    out = dict(means=np.full(Lout, np.nan, dtype=dtype), vars=np.full(Lout, np.nan, dtype=dtype), m=m, quad=dtype(np.nan),
               logdet=dtype(np.nan), ovo=dtype(np.nan), minpiv=np.inf)
    if m:
        Mii = np.empty((m, m), dtype)
        for a, ta in enumerate(steps):
            for b, tb in enumerate(steps):
                Mii[a, b] = Mrow[min(ta, tb), max(ta, tb)]
        u = np.array([us_[t] for t in steps], dtype)
        sd = np.sqrt(np.diag(Mii))
        A = Mii / np.outer(sd, sd)
        Lc = np.zeros((m, m), dtype)
        W = A.copy()
        for c in range(m):
            out["minpiv"] = min(out["minpiv"], float(W[c, c]))
            if not W[c, c] >= MIN_PIVOT:
                out["degenerate"] = True
                out["m"] = m
                out["means"] = out["means"][:L] if Lout > L else out["means"]
                out["vars"] = out["vars"][:L] if Lout > L else out["vars"]
                return out
            Lc[c, c] = np.sqrt(W[c, c])
            Lc[c + 1:, c] = W[c + 1:, c] / Lc[c, c]
            W[c + 1:, c + 1:] -= np.outer(Lc[c + 1:, c], Lc[c + 1:, c])
        Li = np.zeros((m, m), dtype)
        for c in range(m):
            for a in range(c, m):
                Li[a, c] = (dtype(a == c) - Lc[a, c:a] @ Li[c:a, c]) / Lc[a, a]
        w = Li @ (u / sd)
        e = (Li.T @ w) / sd
        Vd = (Li * Li).sum(0) / (sd * sd)
        one = Li @ (1 / sd)
        sc, of = dtype(scale[js]), dtype(offset[js])
        pos = np.array(steps) - lo
        yI = np.array([y[t, js] for t in steps], dtype)
        out["means"][pos] = (yI - e) * sc + of
        keep = dtype(0) if wrong == "keep_obsvar" else dtype(Rv[js])
        out["vars"][pos] = np.maximum(Vd - keep, 0) * sc * (dtype(1) if wrong == "scale_once" else sc)
        out["quad"] = w @ w
        out["logdet"] = -2 * (np.log(sd).sum() + np.log(np.diag(Lc)).sum())
        out["ovo"] = (one @ one) / dtype(m) ** 2 * sc * (dtype(1) if wrong == "scale_once" else sc)
    if lo != t0 or Lout != L:             # a wrong edge: put the rows on the block's own positions
        mm, vv = np.full(L, np.nan, dtype=dtype), np.full(L, np.nan, dtype=dtype)
        for p in range(Lout):
            c = lo + p - t0
            if 0 <= c < L:
                mm[c], vv[c] = out["means"][p], out["vars"][p]
        out["means"], out["vars"] = mm, vv
    return out


# -------------------------------------------------------------------------------------------------------- a degenerate block
DEGENERATE_BLOCKS = np.array([[(0, 4, 6), (1, 7, 12), (2, 6, 9), (3, 10, 12)]], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def degenerate_group():
    """(5,1), T = 12, one record, two instances.  Series 0 has communality 1 (loading 1, no specific variance: q_0 = 0 and a zero
    row of P0) and no observation variance, and is observed at the steps 4 and 5 only; in instance 0 the factor's innovation
    variance is 1e-16, so given the cell at step 4 the one at step 5 is fixed by it to eight digits: the two cells of the block
    (0, 4, 6) have correlation 1 - 1e-15 given the rest, and the second pivot of the unit-diagonal M_II is 1e-15 in exact
    arithmetic.  f stays positive (1e-16 at the second cell): no status bit.  Instance 1 has an ordinary factor: nothing is
    degenerate.  The other blocks lie behind step 5, where the walk has not yet met the two cells."""
    rng = np.random.default_rng(2024)
    N, K, T = 5, 1, 12
    n = N + K
    load = np.array([[1.0], [0.6], [0.5], [-0.7], [0.4]])
    obs = rng.normal(size=(1, T, N))
    obs[0, rng.random((T, N)) < 0.25] = np.nan
    obs[0, :, 0] = np.nan
    obs[0, 4, 0], obs[0, 5, 0] = 0.3, 0.25
    obs[0, 4:6, 1:3] = rng.normal(size=(2, 2))
    phi = np.tile(np.array([0.8, 0.85, 0.9, 0.7, 0.75, 0.9]), (2, 1))
    c = np.concatenate([1.0 - (load ** 2).sum(1), np.ones(K)])
    q = (1.0 - phi ** 2) * c
    q[:, 0] = 0.0
    q[0, N] = 1e-16
    x0 = np.zeros((2, n))
    P0 = np.tile(np.eye(n), (2, 1, 1))
    P0[:, 0, 0] = 0.0
    g = dict(N=N, K=K, T=T, R=1, S=2, B=2, obs=obs, loadings=load[None], patterns=["degenerate"], obsvar=np.zeros((1, N)),
             scale=np.array([[1.5, 0.8, 1.2, 2.0, 0.6]]), offset=np.array([[0.5, -1.0, 2.0, 0.0, 1.0]]), phi=phi, q=q, x0=x0, P0=P0)
    for v in g.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return cf.variant(g)

"""References of the level-shift scan (test infrastructure; no GPU, no test functions): for every observed cell (tau, j) of a
record the regressor x = 1 on the observed cells (t, j) with t >= tau, A = x'u and D = x'Mx with M the precision of the record's
observed data vector and u = M (y - mu): the GLS estimate of the shift is A / D, its standard error 1 / sqrt(D), t = A / sqrt(D).

  definition   the DEFINITION: dense M and u in numpy longdouble from ``block_ref.joint`` (the joint Gaussian of the observed data
               vector; no filter, no smoother, no recursion), A and D per candidate by plain sums -- with the scales of their
               rounding, |x|'|u| and |x|'|M||x|.
  recursion    the kernel's recursion in a chosen dtype: the sequential filter's tape (``block_ref.filter_tape``), one backward
               walk of (r, N) with, per series j, Omega_j, A_j and D_j -- and, by ``wrong=``, the deliberately WRONG variants that
               tests/test_shift_host.py shows to be outside the bar.

Both return ``dict(num [T,N], den [T,N])`` (the definition also ``scale_num``, ``scale_den``), NaN where a cell is not observed.

The bar (``bars``): BAR_SAFETY * MU * eps * scale plus the LOO tier's flat 1e-12.  MU is measured on the CPU
(tests/test_shift_host.py::test_restatement_against_definition prints it): the largest (float64 recursion - definition) /
(eps * scale) over every group, instance and candidate of the tier (MU_EXTRA: of the two groups added to it); BAR_SAFETY = 4 is the allowance tests/block_ref.py gives the
kernels' tree-order fused sums."""
import functools

import numpy as np

import block_ref as br
import call_forms as cf
import functional_ref as fr

LD = np.longdouble
EPS = br.EPS
MU = 1300.0               # measured: tests/test_shift_host.py prints it (the largest value there is 1288)
# ... and over the two groups this tier adds so that Omega is read at n = 64 and at n = 16 (4263 at (15,1), T = 5): a bar of their
# own, so that the other groups keep theirs
MU_EXTRA = {(60, 4, 5): 4300.0, (15, 1, 5): 4300.0}
BAR_SAFETY = 4.0
WRONG = ("omega_gap", "own_cell_first", "m_sign", "d_single", "store_early", "record_div", "neighbour_omega")
# the groups of the GPU tier: (N, K, T); R = 3 records, S = 5 parameter sets (B = 15).  (15,1) and (12,4) have n = 16, the edge of
# the 16-lane group; (60,4) has n = 64 and 60 series lanes; (8,2), T = 33 wraps the kernel's ring of slots with N = 8.  At T = 3
# the groups of (32,4), (60,4) and (15,1) have records with at most one observed step (SINGLE_STEP: no series has two cells, Omega
# is written and never read), so (60,4) and (15,1) are there with T = 5 as well, where two records have series of several cells.
GROUPS = br.GROUPS + ((15, 1, 3), (12, 4, 17), (8, 2, 33), (60, 4, 5), (15, 1, 5))
SINGLE_STEP = ((8, 2, 1), (32, 4, 3), (60, 4, 3), (15, 1, 3))


def group(N, K, T):
    """``block_ref.group``: R = 3, S = 5, given x0 / P0, observation variances, scale and offset; from T = 17 on an empty step
    and a series that is never observed."""
    return br.group(N, K, T)


# -------------------------------------------------------------------------------------------------------------- definition
def definition(g, i):
    """A, D and their rounding scales for every observed cell of instance i, by dense linear algebra in longdouble."""
    key = ("shift definition", i)
    if key in g["_cache"]:
        return g["_cache"][key]
    T, N = g["T"], g["N"]
    r = br._model(g, i)[0]
    cells, mu, Sig = br.joint(g, i)
    out = {k: np.full((T, N), np.nan, dtype=LD) for k in ("num", "den", "scale_num", "scale_den")}
    if cells:
        Lc = fr._cholesky(Sig)
        M = fr._chol_solve(Lc, np.eye(len(cells), dtype=LD))
        M = (M + M.T) / 2
        y = np.array([g["obs"][r][t, j] for t, j in cells], dtype=LD)
        u = M @ (y - mu)
        for j in range(N):
            idx = np.array([a for a, (t, jj) in enumerate(cells) if jj == j], dtype=int)   # in time order
            Mj, uj = M[np.ix_(idx, idx)], u[idx]
            for p, a in enumerate(idx):
                t = cells[a][0]
                out["num"][t, j], out["scale_num"][t, j] = uj[p:].sum(), np.abs(uj[p:]).sum()
                out["den"][t, j], out["scale_den"][t, j] = Mj[p:, p:].sum(), np.abs(Mj[p:, p:]).sum()
    out["mu"] = MU_EXTRA.get((N, g["K"], T), MU)
    g["_cache"][key] = out
    return out


def bars(ref, safety=BAR_SAFETY):
    """dict of the bars of num and den around the definition ``ref`` ([T,N], NaN where not observed)."""
    return dict(num=safety * ref["mu"] * EPS * ref["scale_num"].astype(float) + cf.LOO_TOL,
                den=safety * ref["mu"] * EPS * ref["scale_den"].astype(float) + cf.LOO_TOL)


def distance(got, ref, bar=None):
    """The largest |got - ref| / bar over num and den; NaN on one side only counts as infinitely far."""
    bar = bars(ref) if bar is None else bar
    worst = 0.0
    for k in ("num", "den"):
        a, b = np.asarray(got[k], dtype=LD), ref[k]
        if a.shape != b.shape or (np.isnan(a) != np.isnan(b)).any():
            return np.inf
        ok = ~np.isnan(b)
        if ok.any():
            worst = max(worst, float((np.abs(a[ok] - b[ok]) / bar[k][ok]).max()))
    return worst


def mu_of(got, ref):
    """The largest (got - definition) / (eps * scale) over num and den: what MU is measured as."""
    worst = 0.0
    for k in ("num", "den"):
        ok = ~np.isnan(ref[k])
        if ok.any():
            worst = max(worst, float((np.abs(np.asarray(got[k], dtype=LD)[ok] - ref[k][ok]) / (EPS * ref["scale_" + k][ok])).max()))
    return worst


# --------------------------------------------------------------------------------------------------------------- recursion
def recursion(g, i, dtype=np.float64, wrong=None, _trace=None):
    """The scan of instance i by the kernel's recursion in ``dtype``.  ``wrong``: one of WRONG ("neighbour_omega" takes m from
    the Omega of instance (i + R) % B, the lane group beside it that reads the same record)."""
    key = ("shift recursion", i, np.dtype(dtype).name, wrong)
    if _trace is None and key in g["_cache"]:
        return g["_cache"][key]
    T, N, n = g["T"], g["N"], g["N"] + g["K"]
    rec = (i // g["S"]) % g["R"] if wrong == "record_div" else None
    r_, Z, _, _, _ = br._model(g, i, rec)
    Z = Z.astype(dtype)
    d, rf, v = br.filter_tape(g, i, dtype, rec)
    phi = g["phi"][i].astype(dtype)
    y = g["obs"][r_]
    other = None
    if wrong == "neighbour_omega":
        other = []
        recursion(g, (i + g["R"]) % g["B"], dtype, _trace=other)
        other = iter(other)
    r, Nm = np.zeros(n, dtype), np.zeros((n, n), dtype)
    Om, A, D = np.zeros((N, n), dtype), np.zeros(N, dtype), np.zeros(N, dtype)
    num, den = np.full((T, N), np.nan, dtype), np.full((T, N), np.nan, dtype)

    def store(t):
        seen = rf[t] != 0
        num[t, seen], den[t, seen] = A[seen], D[seen]

    for t in range(T - 1, -1, -1):
        if wrong == "store_early":
            store(t)
        for j in range(N - 1, -1, -1):
            if rf[t, j] == 0:
                continue
            k = d[t, j] * rf[t, j]
            gg = Nm @ k
            us = v[t, j] * rf[t, j] - k @ r
            mss = rf[t, j] + k @ gg
            z = Z[j]
            if _trace is not None:
                _trace.append(Om.copy())
            if wrong == "own_cell_first":
                Om[j] = Om[j] + (mss * z - gg)
            m = -((next(other) if other is not None else Om) @ k)
            if wrong == "m_sign":
                m = -m
            Om = Om + m[:, None] * z[None, :]
            D[j] = D[j] + (mss + (m[j] if wrong == "d_single" else 2 * m[j]))
            A[j] = A[j] + us
            if wrong != "own_cell_first":
                Om[j] = Om[j] + (mss * z - gg)
            r = r + z * us
            Nm = Nm - np.outer(z, gg) - np.outer(gg, z) + mss * np.outer(z, z)
        if wrong != "store_early":
            store(t)
        if not (wrong == "omega_gap" and not np.isfinite(y[t]).any()):
            Om = Om * phi[None, :]
        r, Nm = phi * r, phi[:, None] * Nm * phi[None, :]
    out = dict(num=num, den=den)
    if _trace is None:
        g["_cache"][key] = out
    return out


# --------------------------------------------------------------------------------------------------------- planted shifts
PLANT_SEED = 3
PLANT_T, PLANT_R, PLANT_N, PLANT_K = 120, 5, 4, 1
PLANT_MIN_SEGMENT = 10
PLANTED = ((0, 1, 40), (2, 3, 75), (4, 0, 58))      # (model, series, step); the models 1 and 3 are untouched
PLANT_SIZE = 10.0                                   # in one-step prediction standard deviations of the cell, sqrt(f)


@functools.lru_cache(maxsize=None)
def planted():
    """Records simulated from the model (``metran_amd.synthetic.make_dfm_batch``, fixed seed, a fifth of the cells missing) with
    a level shift of PLANT_SIZE * sqrt(f) of the cell planted in one series of three of the five models, at a step that is
    observed and has PLANT_MIN_SEGMENT observed cells on either side.  dict: obs [R,T,N] (shifted), clean, loadings, alpha,
    phi, q [R,n], planted."""
    from metran_amd.synthetic import make_dfm_batch

    d = make_dfm_batch(PLANT_R, PLANT_N, PLANT_K, PLANT_T, seed=PLANT_SEED, missing=0.2)
    clean = np.array(d["obs"], dtype=np.float64)
    loadings, alpha = np.asarray(d["loadings"], dtype=np.float64), np.asarray(d["alpha"], dtype=np.float64)
    phi = np.exp(-1.0 / alpha)
    c = np.concatenate([1.0 - (loadings ** 2).sum(2), np.ones((PLANT_R, PLANT_K))], axis=1)
    q = (1.0 - phi ** 2) * c
    g = plant_group(clean, loadings, phi, q)
    obs = clean.copy()
    for r, j, t in PLANTED:
        assert np.isfinite(clean[r, t, j])
        assert np.isfinite(clean[r, :t, j]).sum() >= PLANT_MIN_SEGMENT and np.isfinite(clean[r, t:, j]).sum() >= PLANT_MIN_SEGMENT
        f = 1.0 / br.filter_tape(g, r)[1][t, j]
        obs[r, t:, j] += PLANT_SIZE * np.sqrt(f)
    for a in (obs, clean):
        a.setflags(write=False)
    return dict(obs=obs, clean=clean, loadings=loadings, alpha=alpha, phi=phi, q=q, planted=PLANTED)


def plant_group(obs, loadings, phi, q):
    """A group of ``block_ref``'s form over R records with one parameter set each, default initial moments."""
    R, T, N = obs.shape
    return dict(N=N, K=loadings.shape[2], T=T, R=R, S=1, B=R, obs=obs, loadings=loadings, obsvar=None, scale=None, offset=None,
                phi=phi, q=q, x0=None, P0=None, patterns=["planted"] * R, _cache={})

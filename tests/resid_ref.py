"""The numpy restatement of the residual diagnostics (C ABI mk_residual_series / mk_residual_cross, metran_amd/residuals.py) in
``np.longdouble``, straight from ``v`` and ``f`` -- no code shared with the kernels or the package -- the BARS the kernels are
held to, and the inputs of tests/test_residuals_host.py and tests/test_residuals_gpu.py.

Definitions.  A cell (t, j) is valid when v is finite, f is finite and > 0 and t >= t_first; e = v / sqrt(f).  Per series, with
e_1 .. e_m the valid cells in time order: mean = sum e / m, d_i = e_i - mean, S_k = sum d_i^k, h = (m + 1) // 3, ss_first /
ss_last = the sums of e^2 over the first / last h valid cells, C_k = sum_{i<=k} d_i, Q_k = sum_{i<=k} d_i^2, cusum = max |C_k|,
cusq = max |Q_k - (k/m) S2|, each with the step of the first k that attains it.  Across series, e~ = d / sqrt(S2 / m), and for a
calendar lag l: n_ij(l) = #{t: (t, i) and (t - l, j) valid}, s_ij(l) = sum e~[t,i] e~[t-l,j].

The bars are WORST-CASE forward-error bounds of the computation as specified, in double precision with u = 2^-52 (twice the
unit roundoff; first order in u, the second-order terms are covered by the operation counts being rounded up): a sum of P
rounded terms, in ANY order (recursive, tree, scan), is off by at most P u sum|term| plus the errors of its terms.  They get NO
multiplier: a kernel outside them is wrong."""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -52
NSTAT = 12
M, MEAN, S2, S3, S4, H, SS_FIRST, SS_LAST, CUSUM, CUSUM_T, CUSQ, CUSQ_T = range(NSTAT)


def valid_cells(v, f, t_first):
    v, f = np.asarray(v, dtype=np.float64), np.asarray(f, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(v) & np.isfinite(f) & (f > 0) & (np.arange(v.shape[0]) >= t_first)[:, None]


def _e(v, f, ok):
    e = np.zeros(v.shape, dtype=LD)
    e[ok] = np.asarray(v, dtype=LD)[ok] / np.sqrt(np.asarray(f, dtype=LD)[ok])
    return e


def _first_max(x):
    """(max, index of its FIRST occurrence, the largest value strictly below the max or -inf)."""
    k = int(np.argmax(x))        # numpy: the first of equal maxima
    below = x[x < x[k]]
    return x[k], k, (below.max() if below.size else LD(-np.inf))


def series(v, f, t_first=0, variant=None, detail=False):
    """``[N,12]`` longdouble rows of one model (v, f ``[T,N]``).  ``variant`` (WRONG on purpose): 'uncentred' power sums,
    'calendar_thirds' (thirds of the calendar span instead of the compacted sequence), 'h_floor' (h = m // 3), 'last_tie' (the
    LAST step that attains a maximum).  ``detail``: also the bars ``[N,12]`` and, per series, whether the two argmax are
    DECISIVE: the largest excursion exceeds the largest strictly smaller one by more than twice the bar (equal excursions are a
    tie that only exact arithmetic reproduces: the hand-built integer-valued series)."""
    T, N = np.shape(v)
    ok = valid_cells(v, f, t_first)
    E = _e(v, f, ok)
    out = np.full((N, NSTAT), np.nan, dtype=LD)
    bars = np.zeros((N, NSTAT), dtype=LD)
    decisive = np.ones((N, 2), dtype=bool)
    for j in range(N):
        ts = np.nonzero(ok[:, j])[0]
        m = len(ts)
        out[j, M], out[j, H] = m, 0
        if m == 0:
            continue
        e = E[ts, j]
        mean = e.sum() / LD(m)
        d = e - mean if variant != "uncentred" else e.copy()
        h = (m + 1) // 3 if variant != "h_floor" else m // 3
        if variant == "calendar_thirds":
            span = T - t_first
            hc = (span + 1) // 3
            first, last = ts < t_first + hc, ts >= T - hc
        else:
            first, last = np.arange(m) < h, np.arange(m) >= m - h
        C, Q = np.cumsum(d), np.cumsum(d * d)
        s2 = (d * d).sum()
        k = np.arange(1, m + 1).astype(LD)
        xc, xq = np.abs(C), np.abs(Q - k / LD(m) * s2)
        if variant == "last_tie":
            xc, xq = xc[::-1], xq[::-1]
        (cmax, ck, crun), (qmax, qk, qrun) = _first_max(xc), _first_max(xq)
        if variant == "last_tie":
            ck, qk = m - 1 - ck, m - 1 - qk
        out[j] = [m, mean, s2, (d ** 3).sum(), (d ** 4).sum(), h, (e[first] ** 2).sum(), (e[last] ** 2).sum(), cmax, ts[ck], qmax, ts[qk]]
        # ---- the bars.  e = v / sqrt(f): a square root and a division, each rounded once: |de_i| <= u |e_i|.
        # mean: m inputs off by u |e_i|, at most m additions (m u sum|e| in any order), one division: (m + 2) u sum|e| / m.
        # d_i = e_i - mean: |dd_i| <= u |e_i| + bar(mean) + u |d_i|  (its inputs and the rounded subtraction).
        # S_p = sum d_i^p: the propagated p |d_i|^(p-1) dd_i per term, p - 1 rounded products and m additions: (m + p) u sum|d|^p.
        # ss: e_i^2 carries 2 u e_i^2 from e_i and one product, at most h additions: (h + 3) u sum e_i^2.
        # C_k, Q_k: the same over the first k cells -- both grow with k, so the bound at k = m covers max_k; cusq's
        # excursion adds (k/m) bar(S2), the division, product and subtraction (3 u S2) and is at most all of it at k = m.
        ae, ad = np.abs(e), np.abs(d)
        bmean = LD(m + 2) * U * ae.sum() / LD(m)
        dd = U * ae + bmean + U * ad
        bS2 = (2 * ad * dd).sum() + LD(m + 2) * U * (ad ** 2).sum()
        bars[j, MEAN] = bmean
        bars[j, S2] = bS2
        bars[j, S3] = (3 * ad ** 2 * dd).sum() + LD(m + 3) * U * (ad ** 3).sum()
        bars[j, S4] = (4 * ad ** 3 * dd).sum() + LD(m + 4) * U * (ad ** 4).sum()
        bars[j, SS_FIRST] = LD(h + 3) * U * (e[first] ** 2).sum()
        bars[j, SS_LAST] = LD(h + 3) * U * (e[last] ** 2).sum()
        bars[j, CUSUM] = dd.sum() + LD(m) * U * ad.sum()
        bars[j, CUSQ] = 2 * bS2 + 3 * U * s2
        decisive[j] = [cmax - crun > 2 * bars[j, CUSUM], qmax - qrun > 2 * bars[j, CUSQ]]
    return (out, bars, decisive) if detail else out


def cross(v, f, nlags, t_first=0, variant=None, detail=False):
    """``(counts [L+1,N,N] int64, sums [L+1,N,N] longdouble)`` of one model.  ``variant`` (WRONG on purpose): 'lag_sign'
    (e~[t,i] e~[t+l,j]), 'compacted' (lags between the compacted sequences of valid cells instead of calendar steps),
    'no_t_first' (the lagged cell is not held to t_first), 'm_minus_1' (scale sqrt(S2 / (m - 1))).  ``detail``: also the bars."""
    T, N = np.shape(v)
    L = int(nlags)
    ok = valid_cells(v, f, t_first)
    st, sb, _ = series(v, f, t_first, detail=True)
    E = _e(v, f, ok)
    Z, dZ = np.zeros((T, N), dtype=LD), np.zeros((T, N), dtype=LD)
    live = np.zeros(N, dtype=bool)
    for j in range(N):
        m, s2 = int(st[j, M]), st[j, S2]
        live[j] = m > 0 and s2 > 0
        if not live[j]:
            ok[:, j] = False
            continue
        sd = np.sqrt(s2 / LD(m - 1 if variant == "m_minus_1" else m))
        o = ok[:, j]
        Z[o, j] = (E[o, j] - st[j, MEAN]) / sd
        # e~ = d / sd, sd = sqrt(S2 / m) from the statistics row in double: d as in ``series``; S2 off by bar(S2) and rounded, one
        # division and one square root: |dsd| / sd <= bar(S2) / (2 S2) + 2 u; one more division: u |e~|.
        dd = U * np.abs(E[o, j]) + sb[j, MEAN] + U * np.abs(E[o, j] - st[j, MEAN])
        dZ[o, j] = dd / sd + np.abs(Z[o, j]) * (sb[j, S2] / (2 * s2) + 3 * U)
    okl = ok
    if variant == "no_t_first":
        okl = valid_cells(v, f, 0) & live[None, :]
    if variant == "compacted":   # row p of series j: its p-th valid cell
        C, okc = np.zeros((T, N), dtype=LD), np.zeros((T, N), dtype=bool)
        for j in range(N):
            mj = int(ok[:, j].sum())
            C[:mj, j], okc[:mj, j] = Z[ok[:, j], j], True
        Z, ok, okl = C, okc, okc
    counts = np.zeros((L + 1, N, N), dtype=np.int64)
    sums = np.full((L + 1, N, N), np.nan, dtype=LD)
    bars = np.zeros((L + 1, N, N), dtype=LD)
    pair = live[:, None] & live[None, :]
    A, dA = np.abs(Z), dZ
    for l in range(L + 1):
        if l >= T:
            n = np.zeros((N, N), dtype=np.int64)
            s = b = np.zeros((N, N), dtype=LD)
        elif variant == "lag_sign":
            n = ok[:T - l].astype(np.int64).T @ okl[l:].astype(np.int64)
            s, b = Z[:T - l].T @ Z[l:], 0 * Z[:T - l].T @ Z[l:]
        else:
            now, then = slice(l, T), slice(0, T - l)
            n = ok[now].astype(np.int64).T @ okl[then].astype(np.int64)
            s = Z[now].T @ Z[then]
            # s = sum over n products: each carries |e~_i| de~_j + |e~_j| de~_i and its rounding, n additions: (n + 1) u sum|..|
            b = A[now].T @ dA[then] + dA[now].T @ A[then] + (n + 1).astype(LD) * U * (A[now].T @ A[then])
        counts[l] = np.where(pair, n, 0)
        sums[l] = np.where(pair, s, LD(np.nan))
        bars[l] = np.where(pair, b, 0)
    return (counts, sums, bars) if detail else (counts, sums)


# ------------------------------------------------------------------------------------------- the facade's formulas, restated
def normality(row):
    """(nobs, skew, kurtosis, JB, pvalue) of one statistics row."""
    from scipy.stats import chi2

    m, s2 = int(row[M]), row[S2]
    if m < 4 or not s2 > 0:
        return m, np.nan, np.nan, np.nan, np.nan
    var = s2 / LD(m)
    skew, kurt = (row[S3] / LD(m)) / var ** LD(1.5), (row[S4] / LD(m)) / var ** 2
    jb = float(LD(m) / 6 * (skew ** 2 + (kurt - 3) ** 2 / 4))
    return m, float(skew), float(kurt), jb, float(chi2.sf(jb, 2))


def heteroskedasticity(row):
    """(nobs, h, H, pvalue, cusum, cusum step, its pvalue, cusumsq, its step, its pvalue) of one statistics row."""
    from scipy.special import kolmogorov
    from scipy.stats import f as fdist

    m, h = int(row[M]), int(row[H])
    if h == 0 or not row[SS_FIRST] > 0 or not row[S2] > 0:
        return (m, h) + (np.nan,) * 3 + (-1, np.nan, np.nan, -1, np.nan)
    Hs = float(row[SS_LAST] / row[SS_FIRST])
    cs, cq = float(row[CUSUM] / np.sqrt(row[S2])), float(np.sqrt(LD(m) / 2) * row[CUSQ] / row[S2])
    return (m, h, Hs, min(1.0, 2 * min(fdist.cdf(Hs, h, h), fdist.sf(Hs, h, h))), cs, int(row[CUSUM_T]), float(kolmogorov(cs)), cq,
            int(row[CUSQ_T]), float(kolmogorov(cq)))


def cross_test(counts, sums, min_pairs=20):
    """(Q, df, pvalue, worst = (a, b, lag, r, z) or None, |z| of the runner-up) by explicit loops."""
    from scipy.stats import chi2

    L1, N = counts.shape[0], counts.shape[1]
    Q, df, terms = LD(0), 0, []
    for l in range(L1):
        for a in range(N):
            for b in range(N):
                if (a < b if l == 0 else a != b) and counts[l, a, b] >= max(1, min_pairs) and np.isfinite(sums[l, a, b]):
                    n = LD(int(counts[l, a, b]))
                    r = sums[l, a, b] / n
                    Q, df = Q + n * r * r, df + 1
                    terms.append((float(abs(r * np.sqrt(n))), (a, b, l, float(r), float(r * np.sqrt(n)))))
    if df == 0:
        return np.nan, 0, np.nan, None, np.nan
    best = max(range(len(terms)), key=lambda i: terms[i][0])
    rest = [t[0] for i, t in enumerate(terms) if i != best]
    return float(Q), df, float(chi2.sf(float(Q), df)), terms[best][1], (max(rest) if rest else -np.inf)


# ------------------------------------------------------------------------------------------- comparisons at the bars
def inside(got, want, bars, what):
    want = np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want.astype(np.float64))), what
    fin = ~np.isnan(want.astype(np.float64))
    err = np.abs(np.asarray(got, dtype=LD)[fin] - want[fin])
    assert (err <= bars[fin]).all(), (what, float(np.max(err / np.where(bars[fin] > 0, bars[fin], 1))))


EXACT = [M, H]
TIMES = [CUSUM_T, CUSQ_T]


def check_series(got, v, f, t_first, what):
    """One model's rows against the restatement: counts exact, the raw sums at the bars, the time stamps exact where the
    argmax is decisive (tests/resid_ref.py)."""
    want, bars, dec = series(v, f, t_first, detail=True)
    inside(got, want, bars_with_times(bars), what)
    assert np.array_equal(got[:, EXACT], want[:, EXACT].astype(np.float64)), what
    for c, col in enumerate(TIMES):
        rows = dec[:, c] & (want[:, M] > 0)
        assert np.array_equal(got[rows, col], want[rows, col].astype(np.float64)), (what, col)


def bars_with_times(bars):
    b = bars.copy()
    b[:, TIMES] = np.inf     # compared separately, exactly, where decisive
    return b


def check_cross(counts, sums, v, f, nlags, t_first, what):
    """One model's cross sums against the restatement: the counts exact, the sums at the bars, NaN where it has NaN."""
    wc, ws, bars = cross(v, f, nlags, t_first, detail=True)
    assert np.array_equal(counts, wc), what
    inside(sums, ws, bars, what)


# ------------------------------------------------------------------------------------------------------------- test inputs
TILE = 64   # the kernels' time tile


def _cells(B, T, N, seed, missing):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(B, T, N))
    f = rng.uniform(0.5, 2.0, (B, T, N))
    v[rng.random((B, T, N)) < missing] = np.nan
    return v, f


def special_model(T=130, seed=5):
    """One model of 9 series on T = 130 steps: no valid cell; one; m = 2, 3, 4 (h = 1) and m = 5 (h = 2); a constant series
    (e = 1 exactly); valid cells in the last tile only; and f = 0, f < 0, NaN and Inf cells mixed into a full series."""
    rng = np.random.default_rng(seed)
    v = np.full((1, T, 9), np.nan)
    f = np.ones((1, T, 9))
    for j, m in ((1, 1), (2, 2), (3, 3), (4, 4), (5, 5)):
        v[0, np.sort(rng.choice(T, size=m, replace=False)), j] = rng.normal(size=m)
    v[0, :, 6], f[0, :, 6] = 0.5, 0.25
    v[0, 2 * TILE:, 7] = rng.normal(size=T - 2 * TILE)
    v[0, :, 8] = rng.normal(size=T)
    f[0, :, 8] = rng.uniform(0.5, 2.0, T)
    f[0, 3::11, 8], f[0, 5::13, 8], f[0, 7::17, 8], f[0, 9::19, 8], v[0, 10::23, 8] = 0.0, -1.0, np.nan, np.inf, np.inf
    return v, f


def tie_model(T=70):
    """Two integer-valued series whose excursions TIE, with m a power of two so that every operation is exact in every precision:
    e = +1, -1, .. (m = 16, on every second step; |C_k| = 1 at every odd k, first at step 2; Q_k = k is ON its line: all zero) and
    e = +2, -2, 0, 0, +2, -2, 0, 0 (|C_k| = 2 at k = 1 and 5, |Q_k - 2 k| = 4 at k = 2 and 6: the later ones in the second tile)."""
    v = np.full((1, T, 2), np.nan)
    v[0, 2:34:2, 0] = [(-1.0) ** i for i in range(16)]
    v[0, [3, 9, 20, 63, 64, 65, 68, 69], 1] = [2.0, -2.0, 0.0, 0.0, 2.0, -2.0, 0.0, 0.0]
    return v, np.ones_like(v)


def series_cases():
    """``(name, v, f)`` with v, f ``[B,T,N]``: T = 1, 2, 63, 64, 65, 130 x B N = 1, 4, 5, 9 (one wavefront, a full workgroup, and
    one and two workgroups with a replicated tail) x 0 %, 50 %, 95 % missing, the special and the tie model, and the long records
    around step 1024 (``long_cases``)."""
    out = []
    shapes = [(1, 1), (2, 2), (1, 5), (3, 3)]
    for a, T in enumerate((1, 2, 63, 64, 65, 130)):
        for c, missing in enumerate((0.0, 0.5, 0.95)):
            B, N = shapes[(a + c) % 4]
            out.append(("T%d_B%dN%d_miss%d" % (T, B, N, int(100 * missing)),) + _cells(B, T, N, 1000 + 10 * T + c, missing))
    for T in (65, 130):   # every B N at more than one tile
        for B, N in shapes:
            out.append(("T%d_B%dN%d_miss30" % (T, B, N),) + _cells(B, T, N, 7 * T + B + N, 0.3))
    out.append(("special",) + special_model())
    out.append(("tie",) + tie_model())
    return out + long_cases()


KEEP = 16 * TILE   # resid_series_kernel keeps the cells of its first 16 tiles in registers and re-reads v / f beyond step 1024


def late_model(T=1100, seed=9):
    """One model of 5 series on T = 1100 steps, past the 1024 steps the series kernel keeps in registers: 30 % missing; valid cells
    beyond step 1030 only; a FULL series (h = 367: the last third, cells 733 .. 1099, straddles step 1024) whose level and variance
    change at step 1060, so that the largest |C_k| and |Q_k - (k/m) S2| fall after step 1024; 95 % and 50 % missing."""
    v, f = _cells(1, T, 5, seed, 0.3)
    rng = np.random.default_rng(seed + 1)
    v[0, :1030, 1] = np.nan
    v[0, :, 2] = np.where(np.arange(T) < 1060, 0.3 + 0.5 * rng.normal(size=T), -4.0 + 3.0 * rng.normal(size=T))
    f[0, :, 2] = 1.0
    v[0, :, 3] = np.where(rng.random(T) < 0.95, np.nan, rng.normal(size=T))
    v[0, :, 4] = np.where(rng.random(T) < 0.5, np.nan, rng.normal(size=T))
    st = series(v[0], f[0], 0)
    assert st[1, M] > 0 and st[2, M] == T and st[2, CUSUM_T] > KEEP and st[2, CUSQ_T] > KEEP, st[:, [M, CUSUM_T, CUSQ_T]]
    return v, f


def long_cases():
    """``(name, v, f)`` around the end of the kept tiles: T = 1023, 1024, 1025 with missing cells and the late model (T = 1100)."""
    out = []
    for T, (B, N), missing in ((KEEP - 1, (1, 5), 0.3), (KEEP, (2, 2), 0.5), (KEEP + 1, (3, 3), 0.3)):
        out.append(("T%d_B%dN%d_miss%d" % (T, B, N, int(100 * missing)),) + _cells(B, T, N, 3 * T + B, missing))
    out.append(("late",) + late_model())
    return out


def t_firsts(T):
    """0, 1, T and T + 1, and for the long records a first step shortly before and shortly after step 1024."""
    return (0, 1, T, T + 1) + tuple(t for t in (KEEP - 24, KEEP + 6) if t < T)


def check_decisive(cases):
    """Every series of every case, at every t_first the tests use, has decisive time stamps -- but for cusq of a series with
    m <= 2, where every excursion is zero up to rounding by algebra (Q_1 - S2 / 2 = (d_1^2 - d_2^2) / 2 = 0)."""
    for name, v, f in cases:
        for b in range(v.shape[0]):
            for t_first in t_firsts(v.shape[1]):
                st, _, dec = series(v[b], f[b], t_first, detail=True)
                small = st[:, M] <= 2
                assert dec[:, 0].all() and (dec[:, 1] | small).all(), (name, b, t_first, dec)
    return cases


def even_odd_model(T, N, seed):
    """N >= 3 series: A = series 0 observed on even steps only, B = series 1 on odd steps only (n_AB(0) = 0, n_AB(1) > 0), the rest
    30 % missing."""
    v, f = _cells(1, T, N, seed, 0.3)
    rng = np.random.default_rng(seed + 1)
    v[0, :, 0], v[0, :, 1] = rng.normal(size=T), rng.normal(size=T)
    v[0, 1::2, 0] = np.nan
    v[0, 0::2, 1] = np.nan
    return v, f


def cross_cases():
    """``(name, v, f, nlags)``: N = 1, 2, 5, 16, 17, 33, 64 x nlags = 0, 1, 3, 32 (also nlags >= T) x T = 1, 33, 64, 65, 97, 130 (the
    halo crosses no, one and two tile edges), the even/odd pair and a constant series beside live ones."""
    out = []
    for N, T, L, B in ((1, 130, 32, 2), (2, 1, 3, 1), (2, 33, 32, 1), (5, 64, 0, 3), (5, 65, 1, 2), (5, 97, 32, 1), (16, 130, 3, 2),
                       (17, 65, 32, 1), (33, 97, 3, 1), (33, 33, 1, 1), (64, 130, 1, 1), (64, 65, 32, 1), (17, 1, 32, 1)):
        out.append(("N%d_T%d_L%d" % (N, T, L),) + _cells(B, T, N, 50 * N + T + L, 0.3) + (L,))
    v, f = even_odd_model(97, 5, 3)
    out.append(("even_odd", v, f, 3))
    v, f = _cells(1, 130, 4, 77, 0.2)
    v[0, :, 2], f[0, :, 2] = 0.5, 0.25          # S2 = 0
    v[0, :, 3] = np.nan                          # m = 0
    out.append(("dead_series", v, f, 3))
    return out

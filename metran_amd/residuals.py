"""Residual diagnostics from the raw sums of ``BatchedKalman.residual_series`` / ``residual_cross`` (C ABI ``mk_residual_series`` /
``mk_residual_cross``): the test statistics and p-values of ``MetranBatch.test_normality``, ``test_heteroskedasticity`` and
``test_cross_correlation`` as plain numpy functions of the device's output -- no device work here.

The statistics row of a series is ``[m, mean, S2, S3, S4, h, ss_first, ss_last, cusum, cusum_t, cusq, cusq_t]`` over its valid
standardised innovations ``e_1 .. e_m`` (``d_i = e_i - mean``, ``S_k = sum d_i^k``, ``h = (m + 1) // 3``; see the header)."""
import numpy as np

M, MEAN, S2, S3, S4, H, SS_FIRST, SS_LAST, CUSUM, CUSUM_T, CUSQ, CUSQ_T = range(12)


def normality(stats):
    """Jarque-Bera per series from rows ``[..., 12]``: dict of ``nobs``, ``skew = (S3/m) / (S2/m)^1.5``, ``kurtosis = (S4/m) /
    (S2/m)^2``, ``JB = m/6 (skew^2 + (kurtosis - 3)^2 / 4)`` and ``pvalue = chi2.sf(JB, 2)``; NaN for ``m < 4`` or ``S2 = 0``."""
    from scipy.stats import chi2

    s = np.asarray(stats, dtype=np.float64)
    m = s[..., M]
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = (m >= 4) & (s[..., S2] > 0)
        mm = np.where(ok, m, np.nan)
        var = s[..., S2] / mm
        skew = (s[..., S3] / mm) / var ** 1.5
        kurt = (s[..., S4] / mm) / (var * var)
        jb = mm / 6.0 * (skew * skew + (kurt - 3.0) ** 2 / 4.0)
    return {"nobs": m.astype(np.int64), "skew": skew, "kurtosis": kurt, "JB": jb, "pvalue": chi2.sf(jb, 2)}


def heteroskedasticity(stats):
    """Variance-break checks per series from rows ``[..., 12]``: ``H = ss_last / ss_first`` with the two-sided ``pvalue = 2
    min(F.cdf(H, h, h), F.sf(H, h, h))``; ``cusum = max_k |C_k| / sqrt(m s^2)`` and ``cusumsq = sqrt(m / 2) max_k |Q_k - (k/m)
    S2| / S2`` with ``s^2 = S2 / m``, each with the step (``cusum_step`` / ``cusumsq_step``, -1 where undefined) at which it is
    attained and the p-value ``scipy.special.kolmogorov`` of the supremum of a Brownian bridge.  NaN for ``h = 0``,
    ``ss_first = 0`` or ``S2 = 0``."""
    from scipy.special import kolmogorov
    from scipy.stats import f as fdist

    s = np.asarray(stats, dtype=np.float64)
    m, h = s[..., M], s[..., H]
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = (h > 0) & (s[..., SS_FIRST] > 0) & (s[..., S2] > 0)
        nan = np.where(ok, 1.0, np.nan)
        hh = np.where(ok, h, 1.0)
        Hs = s[..., SS_LAST] / s[..., SS_FIRST] * nan
        p = 2.0 * np.minimum(fdist.cdf(Hs, hh, hh), fdist.sf(Hs, hh, hh))
        cusum = s[..., CUSUM] / np.sqrt(s[..., S2]) * nan           # sqrt(m s^2) = sqrt(S2)
        cusq = np.sqrt(m / 2.0) * s[..., CUSQ] / s[..., S2] * nan
    step = lambda col: np.where(ok, np.nan_to_num(s[..., col], nan=-1.0), -1.0).astype(np.int64)  # noqa: E731
    return {"nobs": m.astype(np.int64), "h": h.astype(np.int64), "H": Hs, "pvalue": np.minimum(p, 1.0) * nan,
            "cusum": cusum, "cusum_step": step(CUSUM_T), "cusum_pvalue": kolmogorov(cusum) * nan,
            "cusumsq": cusq, "cusumsq_step": step(CUSQ_T), "cusumsq_pvalue": kolmogorov(cusq) * nan}


def correlations(counts, sums):
    """``r_ij(l) = s / n`` of arrays ``[..., L+1, N, N]``; NaN where ``n < 1``."""
    n = np.asarray(counts, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n >= 1, np.asarray(sums, dtype=np.float64) / np.where(n >= 1, n, 1.0), np.nan)


def cross_correlation(counts, sums, min_pairs=20):
    """The portmanteau statistic of the correlations BETWEEN the series of one model from ``counts``, ``sums`` ``[L+1,N,N]``:
    ``Q = sum n r^2`` over the pairs ``i < j`` at lag 0 and ``i != j`` at every lag ``l >= 1`` with ``n >= min_pairs``, ``df`` the
    number of those terms, ``pvalue = chi2.sf(Q, df)`` (NaN for ``df = 0``), and the term of largest ``|z|``, ``z = r sqrt(n)``:
    ``(a, b, lag, r, z)`` -- the first in (lag, a, b) order among equals; ``None`` for ``df = 0``."""
    from scipy.stats import chi2

    n = np.asarray(counts, dtype=np.float64)
    L1, N = n.shape[0], n.shape[1]
    r = correlations(counts, sums)
    i, j = np.arange(N)[:, None], np.arange(N)[None, :]
    used = np.broadcast_to(i != j, (L1, N, N)).copy()
    used[0] = i < j
    used &= (n >= max(1, int(min_pairs))) & np.isfinite(r)
    df = int(used.sum())
    z = np.where(used, r * np.sqrt(n), 0.0)
    Q = float((z * z).sum())
    if df == 0:
        return {"Q": np.nan, "df": 0, "pvalue": np.nan, "worst": None}
    flat = int(np.argmax(np.where(used, np.abs(z), -1.0)))
    l, a, b = np.unravel_index(flat, used.shape)
    return {"Q": Q, "df": df, "pvalue": float(chi2.sf(Q, df)), "worst": (int(a), int(b), int(l), float(r[l, a, b]), float(z[l, a, b]))}

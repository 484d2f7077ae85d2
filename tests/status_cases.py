"""Inputs, expectations and check functions of the STATUS axis (test infrastructure; no GPU, no test functions): models that
are INVALID, in batches where they share a wavefront with valid ones.

The status word (include/metran_hip.h: MK_FLAG_NONPOSITIVE_F, MK_FLAG_NOT_SPD, MK_FLAG_RANK_DEFICIENT) is the only way a
caller learns that a model's numbers are meaningless; the other tiers run valid inputs and reduce it to "no error bit anywhere".
Here every case is a pair of groups in the style of ``call_forms.shared_group`` -- R = 3 records x S = 3 parameter sets, B = 9,
T = 9: with four models per wavefront the last wavefront holds one live model -- the BAD group and its CLEAN TWIN: the same
arrays with the invalid instances (or the invalid record) replaced by valid ones.

  neg_once           obsvar = -10 on series 0 of record 1 (instances 1, 4, 7), observed at ONE step behind the warm-up
  neg_twice_across   ... observed at TWO such steps: an even number of negative f ACROSS steps (the objective-only product)
  neg_twice_within   obsvar = -10 on series 0 and 1 of record 1, observed at the same steps only: an even number INSIDE a step
  zero_f             P0 = 0 and q = 0 for instances 1 and 6, obsvar = 0 everywhere: every f of theirs is exactly 0
  nan_phi            phi of the first common factor is NaN for instances 1 and 8 (8 sits in the tail wavefront)
  zero_factor        instances 2 and 6: the first common factor has a zero row and column in P0, q = 0, x0 = 0 -- its state and
                     its row of every predicted covariance are exactly 0, the pivot is exactly 0: MK_FLAG_RANK_DEFICIENT alone,
                     from the RTS smoothers alone (the tape walk has no pivot)
  indefinite         smoother entry points only: the filtered covariance of step T - 3 of instances 1 and 6 overwritten with -I
                     (``indefinite_moments``): MK_FLAG_NOT_SPD | MK_FLAG_RANK_DEFICIENT

Expectations come from ``restate`` below -- the sequential filter in numpy longdouble, recording every innovation variance f,
and the LDL' pivots of Pp[t+1] = Phi Pf[t] Phi + Q -- never from the kernels; tests/test_status_cases.py pins it to the C oracle
and asserts the margins that keep every expected bit away from rounding (|f| >= 1e-3 or exactly 0, clean pivots >= 1e-6, the
intended zero pivot exactly 0, the intended negative pivot <= -0.5).

A NaN pivot (met only behind a filter that has ALREADY flagged the instance: its filtered covariances are NaN) sets neither
pivot bit, in every smoother (include/metran_hip.h at MK_FLAG_RANK_DEFICIENT): both comparisons are false.

Check functions (shared by tests/test_status_cases.py over a CPU engine and tests/test_status_gpu.py over the kernels):
  check_flags        the status of every instance equals the expected bit set, bit for bit
  check_containment  every output of every untouched instance is BIT-IDENTICAL to the same call on the clean twin
  check_clean        ... and passes the tier's existing bar against the oracle (tests/call_forms.py: no new tolerance)
  check_objective    oracle mle not finite -> the kernel's is not finite; the kernel's finite -> within MLE_RTOL of the oracle's
"""
import functools

import numpy as np

import call_forms as cf

FLAG_NONPOSITIVE_F, FLAG_NOT_SPD, FLAG_RANK_DEFICIENT = 1, 2, 4   # include/metran_hip.h (tests/test_abi.py holds the engine's to it)
T, R, S = 9, 3, 3
SHAPES = ((8, 2), (13, 4), (32, 4), (33, 4), (60, 4))
GENERIC_SHAPES = ((8, 2), (70, 3))
LAYOUTS = ("model_major", "time_major")
PATTERNS = ("iid", "first", "steps")
BAD_RECORD, BAD_OBSVAR = 1, -10.0
STEP_A, STEP_B = 3, 6               # where the bad series of record 1 is observed
WARMUPS = (0, 1)
RECORD_CASES = ("neg_once", "neg_twice_across", "neg_twice_within")
INSTANCE_CASES = ("zero_f", "nan_phi", "zero_factor")
CASES = RECORD_CASES + INSTANCE_CASES
F_MARGIN, PIVOT_MARGIN, NEGATIVE_PIVOT = 1e-3, 1e-6, -0.5


# ------------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def base(N, K):
    """The shape's valid group, drawn once (read-only)."""
    return cf.shared_group(N, K, T, R, S if N + K <= 64 else 2, 0, patterns=PATTERNS, usable=lambda pat, y, taken: True)


def _record_case(g, name):
    """Record 1 edited (bad group and twin alike): the bad series observed at the chosen steps only, those steps behind the
    warm-up in the compressed index (an observed cell at step 1 sees to that)."""
    N = g["N"]
    series = (0, 1) if name == "neg_twice_within" else (0,)
    steps = (STEP_A,) if name == "neg_once" else (STEP_A, STEP_B)
    rng = np.random.default_rng([N, g["K"], 17])
    obs = g["obs"].copy()
    y = obs[BAD_RECORD]
    fill = rng.standard_normal(y.shape)
    y[:, list(series)] = np.nan
    for t in steps:
        for j in series:
            y[t, j] = fill[t, j]
    if not np.isfinite(y[:STEP_A]).any():
        y[1, N - 1] = fill[1, N - 1]
    obsvar = g["obsvar"].copy()
    obsvar[BAD_RECORD, list(series)] = 0.25
    twin = cf.variant(g, obs=obs, obsvar=obsvar)
    bad_var = obsvar.copy()
    bad_var[BAD_RECORD, list(series)] = BAD_OBSVAR
    touched = tuple(i for i in range(g["B"]) if i % g["R"] == BAD_RECORD)
    return cf.variant(twin, obsvar=bad_var), twin, touched


def _instance_case(g, name):
    N, K, n, B = g["N"], g["K"], g["N"] + g["K"], g["B"]
    phi, q, x0, P0 = (g[k].copy() for k in ("phi", "q", "x0", "P0"))
    twin = g
    if name == "zero_f":
        touched = (1, 6 % B)
        twin = cf.variant(g, obsvar=np.zeros_like(g["obsvar"]))
        for i in touched:
            P0[i], q[i] = 0.0, 0.0
    elif name == "nan_phi":
        touched = (1, B - 1)
        for i in touched:
            phi[i, N] = np.nan
    elif name == "zero_factor":
        touched = (2, 6 % B)
        for i in touched:
            P0[i, N, :], P0[i, :, N], q[i, N], x0[i, N] = 0.0, 0.0, 0.0, 0.0
    else:
        raise KeyError(name)
    return cf.variant(twin, phi=phi, q=q, x0=x0, P0=P0), twin, tuple(sorted(set(touched)))


@functools.lru_cache(maxsize=None)
def case(N, K, name):
    """dict: name, bad, twin (groups), touched (the instances whose inputs differ between the two)."""
    g = base(N, K)
    bad, twin, touched = (_record_case if name in RECORD_CASES else _instance_case)(g, name)
    for grp in (bad, twin):
        for v in grp.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return dict(name=name, bad=bad, twin=twin, touched=touched)


def single_record(c):
    """The case on record 0 alone (R = 1, B = 9 <= 16: the sparse single-record routes); per-instance cases only."""
    assert c["name"] in INSTANCE_CASES
    cut = lambda g: cf.variant(g, R=1, patterns=g["patterns"][:1], **{k: g[k][:1] for k in ("obs", "loadings", "obsvar", "scale", "offset")})  # noqa: E731
    return dict(c, bad=cut(c["bad"]), twin=cut(c["twin"]))


@functools.lru_cache(maxsize=None)
def indefinite_group(N, K):
    """The valid group with a persistence of 0.95 and q = 0.05 for instances 1 and 6, so that Phi (-I) Phi + Q has the pivots
    -0.8525 exactly (a diagonal matrix): the ``indefinite`` case's twin.  touched = (1, 6)."""
    g = base(N, K)
    phi, q = g["phi"].copy(), g["q"].copy()
    touched = (1, 6 % g["B"])
    for i in touched:
        phi[i], q[i] = 0.95, 0.05
    return cf.variant(g, phi=phi, q=q), tuple(sorted(set(touched)))


def indefinite_moments(g, touched, F, Pf, Xp, Pp):
    """Filtered / predicted moments of the clean group ([B,T,...] numpy arrays) -> copies with Pf[T - 3] = -I for the touched
    instances, and the predicted covariance of step T - 2 that goes with it (the 5-argument smoother READS its Pp)."""
    n = g["N"] + g["K"]
    Pf, Pp = np.array(Pf), np.array(Pp)
    for i in touched:
        Pf[i, T - 3] = -np.eye(n)
        Pp[i, T - 2] = -np.diag(g["phi"][i] ** 2) + np.diag(g["q"][i])
    return np.array(F), Pf, np.array(Xp), Pp


# ------------------------------------------------------------------------------------------------------------ restatement
def restate(g, i):
    """Instance i in numpy longdouble: the sequential filter of kalmanfilter.py:315-390 recording every innovation variance, and
    the LDL' pivots of Pp[t+1] = Phi Pf[t] Phi + Q, t = 0 .. T - 2 (a pivot <= 0 is dropped: 1/d := 0).  dict: f (list, in
    order), pivots [T-1,n], F, Pf, mle {warmup: value}.  Kept with the group."""
    key = ("restate", i)
    if key in g["_cache"]:
        return g["_cache"][key]
    ld = np.longdouble
    N, K = g["N"], g["K"]
    n, r = N + K, i % g["R"]
    y = g["obs"][r]
    Z = np.concatenate([np.eye(N), g["loadings"][r]], axis=1).astype(ld)
    Rv = (np.zeros(N) if g["obsvar"] is None else g["obsvar"][r]).astype(ld)
    phi, q = g["phi"][i].astype(ld), g["q"][i].astype(ld)
    x = (np.zeros(n) if g["x0"] is None else g["x0"][i]).astype(ld)
    P = (np.eye(n) if g["P0"] is None else g["P0"][i]).astype(ld)
    fs, sig, det, cnt, F, Pf = [], [], [], [], np.empty((len(y), n)), np.empty((len(y), n, n))
    with np.errstate(all="ignore"):
        for t in range(len(y)):
            x = phi * x
            P = phi[:, None] * P * phi[None, :] + np.diag(q)
            seen = np.nonzero(np.isfinite(y[t]))[0]
            s = d_ = ld(0)
            for j in seen:
                v = ld(y[t, j]) - Z[j] @ x
                d = P @ Z[j]
                f = Rv[j] + Z[j] @ d
                k = d / f
                x = x + k * v
                P = P - np.outer(k, d)
                s, d_ = s + v * v / f, d_ + np.log(f)
                fs.append(float(f))
            if len(seen):
                sig.append(s)
                det.append(d_)
            cnt.append(len(seen))
            F[t], Pf[t] = x, P
        mle = {}
        for w in WARMUPS:
            mle[w] = float(np.log(2 * np.pi) * sum(cnt[w:]) + sum(det[w:], ld(0)) + sum(sig[w:], ld(0)))
        piv = np.empty((len(y) - 1, n))
        for t in range(len(y) - 1):
            A = phi[:, None] * Pf[t].astype(ld) * phi[None, :] + np.diag(q)
            for j in range(n):
                piv[t, j] = A[j, j]
                if A[j, j] > 0:
                    col = A[j + 1:, j] / A[j, j]
                    A[j + 1:, j + 1:] -= np.outer(col, A[j, j + 1:])
    out = dict(f=fs, pivots=piv, F=F, Pf=Pf, mle=mle)
    g["_cache"][key] = out
    return out


def filter_bits(fs):
    return FLAG_NONPOSITIVE_F if any(not f > 0.0 for f in fs) else 0


def pivot_bits(pivots):
    """The smoother's bits of a set of pivots; a NaN pivot sets neither (both comparisons are false)."""
    p = np.asarray(pivots, float)
    return (FLAG_RANK_DEFICIENT if (p <= 0.0).any() else 0) | (FLAG_NOT_SPD if (p < -1e-8).any() else 0)


def expected_status(g, kind):
    """Per instance (filter bits, smoother bits).  kind: "filter" (mk_filter, mk_loglik_grad, mk_loo), "rts"
    (a filter and an RTS smoother), "tape" (a filter and the inverse-free walk, which has no pivot)."""
    out = []
    for i in range(g["B"]):
        rs = restate(g, i)
        out.append((filter_bits(rs["f"]), pivot_bits(rs["pivots"]) if kind == "rts" else 0))
    return out


# -------------------------------------------------------------------------------------------------------- check functions
def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def check_status_values(status, expected, what):
    """``status`` [B] against [(filter bits, smoother bits)] * B, bit for bit."""
    got = _np(status).astype(np.int64) & 0xFFFFFFFF
    assert got.shape == (len(expected),), what
    for i, (fb, sb) in enumerate(expected):
        assert got[i] == fb | sb, "%s: instance %d has status %d, expected %d" % (what, i, got[i], fb | sb)


def check_flags(status, c, kind, what):
    """The bad group's status word.  A [S,B] status (draws) is checked draw by draw: f and the pivots do not depend on the data."""
    st = _np(status)
    exp = expected_status(c["bad"], kind)
    assert any(fb | sb for fb, sb in exp) or (c["name"] == "zero_factor" and kind != "rts"), "the case sets no bit"
    for row in (st if st.ndim == 2 else st[None]):
        check_status_values(row, exp, "%s, %s (%s)" % (what, c["name"], kind))


def check_twin_flags(status, c, kind, what):
    st = _np(status)
    for row in (st if st.ndim == 2 else st[None]):
        check_status_values(row, expected_status(c["twin"], kind), "%s, twin of %s (%s)" % (what, c["name"], kind))


def _arrays(out):
    if isinstance(out, (tuple, list)):
        out = {"out%d" % j: v for j, v in enumerate(out)}
    return {k: _np(v) for k, v in out.items() if not k.startswith("_") and k != "status" and hasattr(v, "shape")}


def check_containment(bad_out, twin_out, c, what, axis=0):
    """Every array of the two results (dicts or tuples; the instance axis is ``axis``): the untouched instances bit-identical."""
    a, b = _arrays(bad_out), _arrays(twin_out)
    assert set(a) == set(b) and a, what
    B = c["bad"]["B"]
    clean = [i for i in range(B) if i not in c["touched"]]
    for k in a:
        assert a[k].shape == b[k].shape and a[k].shape[axis] == B, (what, k)
        x, y = np.take(a[k], clean, axis), np.take(b[k], clean, axis)
        assert x.tobytes() == y.tobytes(), (
            "%s, %s: %s of a clean instance depends on the invalid ones in its batch" % (what, c["name"], k))


_QUANTITY = dict(mle="mle", F="F", Pf="Pf", Xp="Xp", Pp="Pp", S="S", Ps="Ps", sim_means="sim_means", sim_vars="sim_vars", var="state_vars",
                 loo_means="loo_means", loo_vars="loo_vars", gphi="gphi", gq="gq")


def check_clean(out, c, what, warmup=1, keys=None):
    """The untouched instances of a result on the BAD group against ``call_forms.reference``, at the tier's existing bars."""
    g = c["bad"]
    got = {k: _np(v) for k, v in out.items() if k in _QUANTITY and (keys is None or k in keys)}
    assert got, what
    for i in range(g["B"]):
        if i in c["touched"]:
            continue
        parts = ("state",) + (("grad",) if "gphi" in got else ()) + (("loo",) if "loo_means" in got else ())
        ref = cf.reference(g, i, warmup, parts=parts)
        for k, v in got.items():
            if k == "F" and v.shape[-1] != g["N"] + g["K"]:
                continue   # the tape, not filtered means
            cf.assert_close(_QUANTITY[k], v[i], ref[_QUANTITY[k]], g, ref["rec"], "%s, %s: %s" % (what, c["name"], cf._what(g, i)))


def check_objective(mle, c, warmup, what):
    """Every instance of the bad group: a finite number that differs from the reference is never accepted."""
    g, got = c["bad"], _np(mle)
    assert got.shape == (g["B"],), what
    for i in range(g["B"]):
        want = cf.reference(g, i, warmup, parts=("state",))["mle"]
        w = "%s, %s, warm-up %d: %s" % (what, c["name"], warmup, cf._what(g, i))
        if not np.isfinite(want):
            assert not np.isfinite(got[i]), "%s: the reference objective is %r, the kernel returned the finite %r" % (w, want, got[i])
        if np.isfinite(got[i]):
            cf.assert_close("mle", got[i], want, g, i % g["R"], w)

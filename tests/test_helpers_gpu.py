"""GPU: the helper kernels around the filter (mk_standardize, mk_mask_observations, mk_pack_observations, mk_fa_correlation,
the factor analysis at full width, mk_simulate, mk_decompose, mk_params_from_alpha, mk_alpha_grad, mk_sum) against the plain
extended-precision references of tests/helper_ref.py, at the shapes where their hand-written indexing changes path: rows per
pass of the standardise block, the second trip of the correlation's pair loop (N >= 23), counts around one block, shared
records (b % R), the transposed [B,K,T,N] store, null outputs.  Most calls go through the raw C ABI (``kf._L.mk_*``): the
wrappers always pass every output, in place, and turn -1e10 into NaN on the host.  These entry points take run-time sizes
and need no shape module.

Tolerances are those of helper_ref.py, each checked on the CPU first (tests/test_helper_ref.py, fp64 pandas / oracle /
params.py against extended precision); the docstrings below state the derivations."""
import ctypes
import math

import numpy as np
import pytest

import helper_ref as hr
import oracle

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]

MK_ERR_INVALID = -1   # include/metran_hip.h
SENTINEL = -777.25
GUARD = 64


@pytest.fixture(scope="module")
def kf():
    from metran_amd.engine import BatchedKalman

    return BatchedKalman(0)


def _dev(a, dtype=None):
    import torch

    t = torch.from_numpy(np.array(a, order="C"))      # a copy: the shared inputs are read-only
    return t.to("cuda", dtype=dtype) if dtype is not None else t.cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _call(kf, name, *args):
    from metran_amd._lib import check

    kf._bind_stream()
    check(getattr(kf._L, name)(kf._ctx, *args))


def _guarded(shape):
    """An output of ``shape`` prefilled with a sentinel, followed by GUARD sentinel doubles the kernel must leave alone."""
    import torch

    numel = int(np.prod(shape))
    buf = torch.full((numel + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    return buf, buf[:numel].view(*shape) if numel else buf[:0].view(*shape)


def _guard_ok(buf):
    return bool((buf[-GUARD:] == SENTINEL).all())


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# =============================================================================================== standardise
def _layout(y, time_major):
    """Device copy of ``y [R,T,N]`` in the memory order of the layout ([T,R,N] when time-major)."""
    return _dev(y.transpose(1, 0, 2) if time_major else y)


def _unlayout(t, time_major):
    a = _np(t)
    return a.transpose(1, 0, 2) if time_major else a


@pytest.mark.parametrize("time_major", [0, 1], ids=["model_major", "time_major"])
@pytest.mark.parametrize("N", hr.STANDARDIZE_N)
def test_standardize(kf, N, time_major):
    """mk_standardize, R = 3, every T around the block's rows per pass (RP = 256 // N), in each call form: out of place,
    in place, statistics only (d_out NULL) and without d_mean / d_std.  NaN positions and the degenerate series (never
    observed, observed once, constant, one +inf, +inf and -inf) exactly as pandas has them (helper_ref.DEGENERATE, checked
    in test_helper_ref.py); ordinary series within 1e-12 (mean and std relative, standardised values absolute: the bar of
    test_ingest.py, which pandas itself meets against extended precision with a factor 2.5 to spare at N = 63).  The
    input of an out-of-place call is left alone; two calls agree bit for bit.  From N = 7 on every record carries all
    seven kinds; N = 1, 2 and 5 cannot, and run several batches of three records instead (4, 2, 1), each with ordinary
    series of a hundred observations and more next to the degenerate ones (helper_ref.NARROW_KINDS)."""
    import torch

    for T, batch in ((T, b) for T in hr.standardize_lengths(N) for b in range(hr.standardize_batches(N))):
        y, kinds = hr.standardize_case(N, T, batch)
        mean, std, z = hr.standardize_ref(N, T, batch)
        R = y.shape[0]
        src = _layout(y, time_major)
        keep = src.clone()

        def run(inp, out, mu, sd):
            _call(kf, "mk_standardize", R, T, N, time_major, _p(inp), _p(out), _p(mu), _p(sd))

        def check_stats(mu, sd):
            mu, sd = _np(mu), _np(sd)
            for r in range(R):
                for j in range(N):
                    if kinds[r, j] in hr.EXACT_KINDS:
                        want = hr.expected_degenerate(kinds[r, j], T)
                        assert np.array_equal([mu[r, j], sd[r, j]], want, equal_nan=True), (T, r, j, kinds[r, j], mu[r, j], sd[r, j])
                ok = ~np.isin(kinds[r], hr.EXACT_KINDS)
                np.testing.assert_allclose(mu[r, ok], mean[r, ok], rtol=hr.STD_TOL, atol=1e-14, equal_nan=True, err_msg="mean T=%d" % T)
                np.testing.assert_allclose(sd[r, ok], std[r, ok], rtol=hr.STD_TOL, equal_nan=True, err_msg="std T=%d" % T)

        def check_out(out):
            got = _unlayout(out, time_major)
            assert np.array_equal(np.isnan(got), np.isnan(z)), "NaN pattern, T=%d" % T
            assert not np.isinf(got).any()
            np.testing.assert_allclose(got, z, rtol=0, atol=hr.STD_TOL, equal_nan=True, err_msg="T=%d" % T)

        new = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float64, device="cuda")
        # out of place, everything
        out, mu, sd = new(*src.shape), new(R, N), new(R, N)
        run(src, out, mu, sd)
        check_stats(mu, sd)
        check_out(out)
        assert torch.equal(src.view(torch.int64), keep.view(torch.int64))
        # again: bit-identical
        out2, mu2, sd2 = new(*src.shape), new(R, N), new(R, N)
        run(src, out2, mu2, sd2)
        for a, b in ((out, out2), (mu, mu2), (sd, sd2)):
            assert torch.equal(a.view(torch.int64), b.view(torch.int64))
        # statistics only
        mu3, sd3 = new(R, N), new(R, N)
        run(src, None, mu3, sd3)
        assert torch.equal(mu3.view(torch.int64), mu.view(torch.int64)) and torch.equal(sd3.view(torch.int64), sd.view(torch.int64))
        assert torch.equal(src.view(torch.int64), keep.view(torch.int64))
        # no statistics; then one of the two
        out4 = new(*src.shape)
        run(src, out4, None, None)
        assert torch.equal(out4.view(torch.int64), out.view(torch.int64))
        mu5, sd5 = new(R, N), new(R, N)
        run(src, None, mu5, None)
        run(src, None, None, sd5)
        assert torch.equal(mu5.view(torch.int64), mu.view(torch.int64)) and torch.equal(sd5.view(torch.int64), sd.view(torch.int64))
        # in place
        work = src.clone()
        run(work, work, None, None)
        assert torch.equal(work.view(torch.int64), out.view(torch.int64))


@pytest.mark.parametrize("time_major", [0, 1], ids=["model_major", "time_major"])
@pytest.mark.parametrize("N", [5, 64])
def test_standardize_large_offset(kf, N, time_major):
    """Values 1e6 + 1e-2 noise, T = 400, 30 % missing.  Standardised values within C_OFFSET eps (|mean| / std + |z|):
    the mean of such a series carries a rounding of eps |mean| / 2, which the division by std turns into eps |mean| / std
    in z; C_OFFSET = 5 is four times what pandas (fp64, two-pass) needs against extended precision on these records
    (1.20, test_helper_ref.py::test_offset_bound_holds_for_pandas).  The mean within gamma eps mean|y|,
    gamma = ceil(T / RP) + RP: the lengths of the kernel's two summation stages.  The std within 1e-12 relative (pandas:
    4e-16)."""
    import torch

    cols = np.arange(N) % 5
    y = np.stack([hr.offset_record(seed)[:, cols] + 0.0 for seed in (0, 1)])
    y[1, :, N - 1] += 3e6
    R, T = y.shape[0], y.shape[1]
    src = _layout(y, time_major)
    mu = torch.empty((R, N), dtype=torch.float64, device="cuda")
    sd = torch.empty_like(mu)
    _call(kf, "mk_standardize", R, T, N, time_major, _p(src), _p(src), _p(mu), _p(sd))
    got = _unlayout(src, time_major)
    for r in range(R):
        mean, std, z = hr.standardize(y[r])
        err_mean = np.abs(_np(mu)[r] - mean) / hr.mean_bound(y[r], N)
        err_z = np.abs(got[r] - z) / hr.offset_bound(mean, std, z)
        print("N=%d record %d: mean at %.3f of gamma eps mean|y|, z at %.3f of C_OFFSET eps (|mean|/std + |z|), std rel %.1e"
              % (N, r, err_mean.max(), np.nanmax(err_z), np.abs(_np(sd)[r] / std - 1).max()))
        assert np.array_equal(np.isnan(got[r]), np.isnan(z))
        assert err_mean.max() <= 1.0 and np.nanmax(err_z) <= 1.0
        np.testing.assert_allclose(_np(sd)[r], std, rtol=hr.STD_TOL)


def test_standardize_refuses_65_series(kf):
    """N = 65 (the block's shared arrays hold 64 series): MK_ERR_INVALID, and nothing is launched -- the output keeps its
    sentinel."""
    import torch

    src = torch.zeros((1, 4, 65), dtype=torch.float64, device="cuda")
    out = torch.full_like(src, SENTINEL)
    kf._bind_stream()
    rc = kf._L.mk_standardize(kf._ctx, 1, 4, 65, 0, _p(src), _p(out), None, None)
    torch.cuda.synchronize()
    assert rc == MK_ERR_INVALID and b"N <= 64" in kf._L.mk_last_error()
    assert bool((out == SENTINEL).all())
    assert kf._L.mk_fa_correlation(kf._ctx, 1, 4, 65, 0, _p(src), _p(out)) == MK_ERR_INVALID


# =============================================================================================== mask
@pytest.mark.parametrize("count", hr.MASK_COUNTS)
def test_mask(kf, count):
    """mk_mask_observations: mask bytes 0 / 1 / 2 / 255 over NaN, +-inf and -0.0, out of place and in place; bit for
    bit where not masked, NaN where masked, nothing written past the end."""
    y, m = hr.mask_case(count)
    want = hr.mask(y, m)
    hidden = m != 0
    src, md = _dev(y), _dev(m)
    buf, out = _guarded((count,))
    _call(kf, "mk_mask_observations", count, _p(src), _p(md), _p(out))
    got = _np(out)
    assert np.array_equal(_bits(got)[~hidden], _bits(want)[~hidden]) and np.isnan(got[hidden]).all()
    assert _guard_ok(buf) and np.array_equal(_bits(_np(src)), _bits(y))
    _call(kf, "mk_mask_observations", count, _p(src), _p(md), _p(src))
    got = _np(src)
    assert np.array_equal(_bits(got)[~hidden], _bits(want)[~hidden]) and np.isnan(got[hidden]).all()


# =============================================================================================== pack
@pytest.mark.parametrize("R,T,N", hr.PACK_SHAPES)
def test_pack(kf, R, T, N):
    """mk_pack_observations through the raw ABI (the engine's set_observations turns -1e10 into NaN on the host, so only
    this route lets the kernel's own ``v + 1e10 != 0`` decide): -1e10 is dropped, its two fp64 neighbours are kept; all
    three outputs equal helper_ref.pack and oracle.set_observations exactly; each output NULL in turn."""
    import torch

    y = hr.pack_case(R, T, N)
    ref = [hr.pack(y[r]) for r in range(R)]
    for r in range(R):
        for a, b in zip(ref[r], oracle.set_observations(y[r])):
            assert np.array_equal(a, b)
    want = [np.stack([x[i] for x in ref]) for i in range(3)]
    src = _dev(y)

    def outputs():
        bo, o = _guarded((R, T, N))
        bi, ix = _guarded((R, T, N))
        c = torch.full((R * T + GUARD,), -7, dtype=torch.int64, device="cuda")
        return (bo, bi, c), (o, ix, c[: R * T].view(R, T))

    for skip in (None, 0, 1, 2):
        bufs, outs = outputs()
        args = [None if i == skip else outs[i] for i in range(3)]
        _call(kf, "mk_pack_observations", R, T, N, _p(src), _p(args[0]), _p(args[1]), _p(args[2]))
        for i in range(3):
            if i == skip:
                assert bool((bufs[i] == (SENTINEL if i < 2 else -7)).all())
            else:
                assert np.array_equal(_np(outs[i]), want[i]), ("observations", "indices", "count")[i]
        assert _guard_ok(bufs[0]) and _guard_ok(bufs[1]) and bool((bufs[2][-GUARD:] == -7).all())
    assert np.array_equal(_bits(_np(src)), _bits(y))


def test_pack_through_the_engine_time_major():
    """BatchedKalman.pack_observations in the time-major layout (its outputs rely on empty_like keeping the [T,R,N]
    strides): equal to the reference record by record, -1e10 lost on the host as documented."""
    from metran_amd.engine import BatchedKalman

    R, T, N = hr.PACK_SHAPES[1]
    y = hr.pack_case(R, T, N)
    e = BatchedKalman(0, layout="time_major").set_observations(np.array(y))
    assert e.obs.transpose(0, 1).is_contiguous()
    o, ix, c = e.pack_observations()
    assert o.stride() == e.obs.stride() and ix.stride() == e.obs.stride()
    for r in range(R):
        ro, ri, rc = hr.pack(y[r])
        assert np.array_equal(_np(o)[r], ro) and np.array_equal(_np(ix)[r], ri) and np.array_equal(_np(c)[r], rc)


# =============================================================================================== correlation
def _corr(kf, y, time_major):
    import torch

    R, T, N = y.shape
    src = _layout(y, time_major)
    buf, out = _guarded((R, N, N))
    _call(kf, "mk_fa_correlation", R, T, N, time_major, _p(src), _p(out))
    torch.cuda.synchronize()
    assert _guard_ok(buf)
    return _np(out)


@pytest.mark.parametrize("time_major", [0, 1], ids=["model_major", "time_major"])
@pytest.mark.parametrize("N", hr.CORR_N)
def test_correlation(kf, N, time_major):
    """mk_fa_correlation, R = 3, T = 60; N = 22 fills the block's first trip over the pairs (P = 253), N >= 23 needs the
    second (P = 276 .. 2080).  Symmetric bit for bit; NaN exactly where the definition has it (no common row, one common
    row, constant series); diagonal exactly 1 or NaN; off-diagonals within 1e-12 (test_factoranalysis_gpu.py's bar),
    plus C_OFFSET eps |mean| / sd per series for the one with mean 1e6 (helper_ref.corr_bound: a correlation is an average
    of products of standardised values, which carry that error; about 2e-9, of which pandas uses 8e-11)."""
    y, roles = hr.corr_case(N)
    ref = hr.corr_ref(N)
    got = _corr(kf, y, time_major)
    assert not (got == SENTINEL).any()
    for r in range(y.shape[0]):
        assert np.array_equal(_bits(got[r]), _bits(got[r].T))
        assert np.array_equal(np.isnan(got[r]), np.isnan(ref[r]))
        d = np.diag(got[r])
        assert np.array_equal(d, np.diag(ref[r]), equal_nan=True) and np.all((d == 1.0) | np.isnan(d))
        err = np.abs(got[r] - ref[r]) / hr.corr_bound(y[r])
        assert np.nanmax(err, initial=0.0) <= 1.0, (r, np.nanmax(np.abs(got[r] - ref[r])))
    assert np.array_equal(_bits(got), _bits(_corr(kf, y, time_major)))


@pytest.mark.parametrize("time_major", [0, 1], ids=["model_major", "time_major"])
@pytest.mark.parametrize("N", [23, 64])
def test_correlation_with_inf(kf, N, time_major):
    """+-inf in the input -- two +inf in record 0, +inf and -inf in record 1, two -inf in record 2 -- (not compared with
    pandas, whose online algorithm returns an artefact there): every entry that involves the series is NaN, and every
    other entry is bit for bit what the kernel gives with that series removed."""
    y, roles = hr.corr_case(N, with_inf=True)
    ref = hr.corr_ref(N, with_inf=True)
    got = _corr(kf, y, time_major)
    clean = np.array(y)
    for r, s in enumerate(roles["inf"]):
        clean[r, :, s] = np.nan
    base = _corr(kf, clean, time_major)
    for r, s in enumerate(roles["inf"]):
        assert np.isnan(got[r, s]).all() and np.isnan(got[r, :, s]).all()
        keep = np.arange(N) != s
        sub = np.ix_(keep, keep)
        assert np.array_equal(_bits(got[r][sub]), _bits(base[r][sub]))
        assert np.array_equal(np.isnan(got[r]), np.isnan(ref[r]))
        assert np.nanmax(np.abs(got[r] - ref[r]) / hr.corr_bound(clean[r]), initial=0.0) <= 1.0


# =============================================================================================== factor analysis, full width
@pytest.mark.parametrize("R,T,N,K,nf", hr.FACTOR_CASES, ids=["-".join(map(str, c[:4])) for c in hr.FACTOR_CASES])
def test_factor_analysis_at_full_width(R, T, N, K, nf):
    """mk_fa_correlation -> mk_fa_analyse -> mk_fa_minres -> mk_fa_rotate end to end at N = 33 and N = 64 (the 64-lane
    blocks' limit; the suite stopped at 32), against oracle.factor_oracle.solve model by model at the tolerances of
    test_seeded_multi_factor_batch_against_the_oracle: factor count equal, loadings 1e-8 where the minimiser returns its
    start vector and 1e-5 where it iterates; correlations 1e-12, eigenvalues 1e-10.  On the batches with 2 and 3 true
    factors the reference's MAP test keeps one factor, so they reach only the single-column route (no varimax); the
    batches with 4 and 8 true factors settle on two and four (pinned in test_helper_ref.py), and there the count is
    asserted >= 2 as in that test: normalisation, varimax with its K x K eigensolver and polar factor, and the
    scale-back all run at N = 33 and N = 64."""
    from metran_amd.factoranalysis import FactorAnalysisBatch
    from oracle import factor_oracle as fo

    assert nf >= 2 or K < 4            # the added batches reach the rotation, as in the model test
    y = hr.factor_case(R, T, N, K)
    res = FactorAnalysisBatch().solve(obs=np.array(y))
    for r in range(R):
        o = fo.solve(y[r])
        np.testing.assert_allclose(_np(res.corr)[r], o["corr"], atol=1e-12)
        np.testing.assert_allclose(_np(res.eigval)[r], np.sort(np.linalg.eigvalsh(o["corr"]))[::-1].clip(0), atol=1e-10)
        assert int(res.nfactors[r]) == o["nfactors"] == nf and int(res.status[r]) == 0
        np.testing.assert_allclose(_np(res.factors)[r][:, :nf], o["factors"], atol=1e-8 if bool(res.stalled[r]) else 1e-5)
        assert not _np(res.factors)[r][:, nf:].any()


# =============================================================================================== simulate / decompose
@pytest.mark.parametrize("N,n", hr.PROJECTION_SHAPES)
def test_simulate_and_decompose(kf, N, n):
    """mk_simulate / mk_decompose, B = 5 instances sharing RZ = 1, 2 or 5 observation matrices (instance b uses Z[b % RZ]),
    T = 1 and 3, K = n - N from 0 to 4 (cdf is [B,K,T,N]: transposed against the thread order; with K = 0 it is empty and
    must not be written).  Means, variances and sdf within 1e-13 n sum|terms| (n- and n^2-term dot products in index
    order, contraction allowed: each partial sum rounds once, so (n + 1) eps / 2 sum|terms| for the means and twice that
    for the quadratic form bound the error -- 1e-13 n is six times the latter; the fp64 oracle uses < 0.001 of it); cdf, a
    single product, within one rounding.  The projected variance of about -0.3 comes out exactly 0.0; the covariance
    holding a NaN gives NaN, not 0.  Every null-output combination; each output sits in front of guard elements that
    must survive."""
    K = n - N
    for RZ in (1, 2, 5):
        for T in (1, 3):
            Z, x, P = hr.projection_case(N, n, RZ, T)
            ref = hr.projection_ref(N, n, RZ, T)
            B = x.shape[0]
            dZ, dx, dP = _dev(Z), _dev(x), _dev(P)

            def close(got, key):
                want, tol = ref[key], hr.PROJ_TOL * n * ref[key + "_abs"]
                nan = np.isnan(want)
                assert np.array_equal(np.isnan(got), nan), key
                assert (np.abs(got - want)[~nan] <= tol[~nan]).all(), (key, RZ, T, float(np.abs(got - want)[~nan].max()))

            for want_m, want_v, with_covs in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 0, 0)):
                bm, sm = _guarded((B, T, N))
                bv, sv = _guarded((B, T, N))
                _call(kf, "mk_simulate", B, RZ, T, N, n, _p(dZ), _p(dx), _p(dP if with_covs else None),
                      _p(sm if want_m else None), _p(sv if want_v else None))
                assert _guard_ok(bm) and _guard_ok(bv)
                if want_m:
                    close(_np(sm), "sim_means")
                else:
                    assert bool((bm == SENTINEL).all())
                if want_v:
                    v = _np(sv)
                    close(v, "sim_vars")
                    assert np.array_equal(v == 0.0, ref["sim_vars"] == 0.0)          # the clip, exactly
                    nb, nt = hr.SPECIAL_COV["negative"]
                    if T > nt:
                        assert v[nb, nt, 0] == 0.0 and not np.signbit(v[nb, nt, 0])
                    nb, nt = hr.SPECIAL_COV["nan"]
                    if T > nt:
                        assert np.isnan(v[nb, nt]).all()
                else:
                    assert bool((bv == SENTINEL).all())
            for want_s, want_c in ((1, 1), (0, 1), (1, 0)):
                bs, sdf = _guarded((B, T, N))
                bc, cdf = _guarded((B, K, T, N))
                _call(kf, "mk_decompose", B, RZ, T, N, n, _p(dZ), _p(dx), _p(sdf if want_s else None), _p(bc if want_c else None))
                assert _guard_ok(bs) and _guard_ok(bc)
                if want_s:
                    close(_np(sdf), "sdf")
                else:
                    assert bool((bs == SENTINEL).all())
                if want_c and K:
                    c = _np(cdf)
                    assert (np.abs(c - ref["cdf"]) <= hr.EPS * np.abs(ref["cdf"])).all()
                if not want_c or K == 0:
                    assert bool((bc == SENTINEL).all())       # K = 0: a non-null cdf is not touched


# =============================================================================================== parameters
@pytest.mark.parametrize("N,K", hr.PARAM_SHAPES)
def test_params_and_alpha_grad(kf, N, K):
    """mk_params_from_alpha / mk_alpha_grad, B = 7 instances over R = 1, 3, 7 loading records (instance b uses b % R),
    dt = 1 and 7, alpha from 1e-5 (phi underflows: exactly 0) to 1e8 (1 - phi^2 cancels).  phi and q against the
    reference's own fp64 formula, params.phi_q_from_alpha -- not the extended value: at alpha = 1e8 that formula's
    1 - phi^2 has eight digits, and the product must match it, not beat it.  phi within 8 eps absolute (the device's exp
    and libm's differ by 1-2 ulp, <= eps for phi in [1/2, 1)); q within helper_ref.q_bound = eps (8 |c| + K comm + |q|),
    derived there; a communality of exactly 1 gives q exactly 0.  galpha against the extended-precision formula within
    16 eps of the sum of the moduli of its two terms at every alpha: the reference forms dt / alpha in fp64, as the
    kernel must, and does the rest in extended precision, so the rounding of exp's argument is common to both.  One
    deviation from the plain 16 eps, stated here because it loosens a set bound: where phi itself is subnormal
    (alpha = 1 / 720, dt = 1) no fp64 value of it is within eps, and those entries get
    2 * 2^-1074 (|gphi| + 1) dt / alpha^2 + 2^-1074 absolute on top, derived in helper_ref.galpha_bound.  With K = 0 both entry
    points accept loadings = NULL."""
    import torch

    from metran_amd.params import phi_q_from_alpha

    n = N + K
    for R in (1, 3, 7):
        for dt in (1.0, 7.0):
            alpha, loadings, gphi, gq = hr.param_case(N, K, R)
            B = alpha.shape[0]
            lb = hr.tile_loadings(loadings, B)
            phi64, q64 = phi_q_from_alpha(alpha, lb, dt)
            g, moduli = hr.alpha_grad(alpha, lb, dt, gphi, gq)
            da, dg1, dg2 = _dev(alpha), _dev(gphi), _dev(gq)
            dl = _dev(loadings) if K else None
            bp, phi = _guarded((B, n))
            bq, q = _guarded((B, n))
            bg, ga = _guarded((B, n))
            _call(kf, "mk_params_from_alpha", B, R, N, K, _p(da), _p(dl), dt, _p(phi), _p(q))
            _call(kf, "mk_alpha_grad", B, R, N, K, _p(da), _p(dl), dt, _p(dg1), _p(dg2), _p(ga))
            torch.cuda.synchronize()
            assert _guard_ok(bp) and _guard_ok(bq) and _guard_ok(bg)
            phi, q, ga = _np(phi), _np(q), _np(ga)
            assert (phi[phi64 == 0.0] == 0.0).all() and phi[0, 0] == 0.0                    # underflow, exactly
            assert (np.abs(phi - phi64) <= hr.PHI_TOL).all(), float(np.abs(phi - phi64).max() / hr.EPS)
            tol = hr.q_bound(lb, q64)
            assert (np.abs(q - q64) <= tol).all(), float((np.abs(q - q64) / np.maximum(tol, 1e-300)).max())
            if K:
                assert (q[:, 0] == 0.0).all()                                               # communality exactly 1
            assert 0 < q[0, -1] < 4e-8 * dt                                                 # alpha = 1e8: the cancelling end
            err = np.abs(ga - g)
            bound = hr.galpha_bound(alpha, dt, gphi, moduli)
            live = bound > 0
            print("N=%d K=%d R=%d dt=%g: galpha at %.3f of its bound (%.2f eps of the moduli where phi is normal)"
                  % (N, K, R, dt, float((err[live] / bound[live]).max()),
                     float((err / np.maximum(moduli, 1e-300))[phi64 >= hr.SMALLEST_NORMAL].max() / hr.EPS)))
            assert (err <= bound).all(), float((err[live] / bound[live]).max())
            assert (ga[phi64 == 0.0] == 0.0).all()


def test_loadings_stay_required_when_there_are_factors(kf):
    """loadings = NULL is accepted with K = 0 only (test_params_and_alpha_grad runs that at (5, 0)); with K = 1 both entry
    points refuse it and launch nothing."""
    import torch

    B, N, K = 2, 5, 1
    alpha = torch.full((B, N + K), 10.0, dtype=torch.float64, device="cuda")
    g1, g2 = torch.ones_like(alpha), torch.ones_like(alpha)
    outs = [torch.full_like(alpha, SENTINEL) for _ in range(3)]
    kf._bind_stream()
    assert kf._L.mk_alpha_grad(kf._ctx, B, 1, N, K, _p(alpha), None, 1.0, _p(g1), _p(g2), _p(outs[0])) == MK_ERR_INVALID
    assert kf._L.mk_params_from_alpha(kf._ctx, B, 1, N, K, _p(alpha), None, 1.0, _p(outs[1]), _p(outs[2])) == MK_ERR_INVALID
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs)


# =============================================================================================== sum
@pytest.mark.parametrize("count", hr.SUM_COUNTS)
def test_sum(kf, count):
    """mk_sum (one 1024-thread block: a 1024-way strided sum, then a ten-level tree) against math.fsum:
    |got - fsum| <= (ceil(count / 1024) + 10) eps sum|v| -- each value passes through at most ceil(count / 1024)
    additions in its lane and ten in the tree, each rounding at eps / 2 of a partial sum that is at most sum|v|.
    Objective-like values, a cancelling vector, NaN and +inf (which come through as themselves); two calls bit-identical."""
    import torch

    for kind in hr.SUM_KINDS:
        v = hr.sum_case(count, kind)
        want = hr.fsum(v)
        dv = _dev(v)
        out = torch.full((1 + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
        _call(kf, "mk_sum", count, _p(dv), _p(out))
        got = float(out[0])
        assert _guard_ok(out)
        if kind == "nan":
            assert math.isnan(got)
        elif kind == "inf":
            assert got == math.inf
        else:
            assert abs(got - want) <= hr.sum_bound(v), (kind, got, want, abs(got - want) / hr.sum_bound(v))
        again = kf.sum(dv)
        assert np.array_equal(_bits(np.array([got])), _bits(np.array([float(again)])))

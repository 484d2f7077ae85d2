"""GPU tier, the record emission of the 16-lane filter (filter_kernel, OUT = 1 and 3, mk_kernels.hip): the cases only a
DEFERRED pipeline can get wrong.  The kernel puts the filtered record of step t into its LDS image at the end of step t and
stores it during step t + 1 (the last one after the loop), forms the logarithm, the pad (sigma, detf) and the running sums of
step t at the head of step t + 1, and writes a compressed entry whose index is behind its step (an earlier step was empty) with
one scattered store that must follow the chunk stores of the record it lands in.  tests/test_time_axis_gpu.py walks the tile
lengths through the same routes; here:

  shapes    (8,2); (1,1): one update a step, every slot of the schedule collapses into one; (14,2): n = 16, no replica lane
  B         1; 5: a second, partly filled wavefront; 17: a second workgroup
  T         1 (the loop body once, everything leaves after the loop), 2, 3, 17 (a second observation tile)
  patterns  everything observed | step 0 empty | step 1 empty, step 2 observed (the entry of step 2 lands in the record of step 1,
            whose chunks leave in the same step) | the last step empty | two consecutive empty steps in the middle | one model
            of every four with empty steps beside three without (the masked path next to the fast one's data)
  both layouts, full-square and packed-symmetric records, both record sets (``filter_smooth``) and the filtered record alone
  (``simulate_smoothed`` on the records path), warm-up 0 and 2 (alternating over the engines so that every route sees both
  under both layouts and both record forms)

Checks: Xp, Pp, F, Pf, -2 log L, sigmacount and the per-step sigma / detf read from the filtered records' pads -- their zero
tail included -- against the oracle at the bars of tests/call_forms.py (the ones tests/test_time_axis_gpu.py uses).

No bitwise comparison with the dense route (OUT = 2: direct column stores, no LDS image, bookkeeping in its own step): at the
PARENT of the deferred schedule the record route and the dense route of (8,2) already differ in the last bit (measured on
these groups: 220 of 714 arrays, up to 4e-16 in the moments and 7e-15 in -2 log L; the two record routes differ from each
other in 144 arrays) -- the instantiations are compiled separately and contract differently -- so that equality is no
property to hold on to.  What was held instead, once, when the schedule went in: every array of both record routes on every
group of this file at (8,2), both warm-ups, bit for bit equal between the parent's library and the deferred one."""
import functools

import numpy as np
import pytest

import call_forms as cf
import time_axis as ta

pytestmark = pytest.mark.gpu

SHAPES = ((8, 2), (1, 1), (14, 2))
BATCHES = (1, 5, 17)
LENGTHS = (1, 2, 3, 17)
LAYOUTS = ("model_major", "time_major")


def _empty_steps(pattern, T, r):
    """The steps without any observation of record r under a pattern, or None where T has no such case."""
    if pattern == "all":
        return []
    if pattern == "step0":
        return [0] if T >= 2 else None
    if pattern == "step1":                      # step 2 observed: its compressed index is 1 = t - 1
        return [1] if T >= 3 else None
    if pattern == "last":
        return [T - 1] if T >= 2 else None
    if pattern == "two":
        return [T // 2 - 1, T // 2] if T >= 5 else None
    if pattern == "mixed":                      # model 1 of every wavefront's four; T = 1: that model observes nothing at all
        if r % 4 != 1:
            return []
        return sorted({0, T // 2, T - 1}) if T >= 3 else [0]
    raise KeyError(pattern)


PATTERNS = ("all", "step0", "step1", "last", "two", "mixed")


@functools.lru_cache(maxsize=None)
def group(N, K, B, T, pattern):
    """B models on B records of their own (one pattern of empty steps each), every other step fully observed."""
    if _empty_steps(pattern, T, 1) is None:
        return None
    g = cf.shared_group(N, K, T, B, 1, 11, patterns=("iid",), usable=lambda pat, y, taken: True)
    rng = np.random.default_rng([N, K, B, T, PATTERNS.index(pattern)])
    obs = np.where(np.isfinite(g["obs"]), g["obs"], rng.standard_normal(g["obs"].shape))
    for r in range(B):
        obs[r, _empty_steps(pattern, T, r)] = np.nan
    obs.setflags(write=False)
    return cf.variant(g, obs=obs)


@pytest.fixture(scope="module", autouse=True)
def jit_cache(tmp_path_factory):
    import os

    old = os.environ.get("METRAN_HIP_CACHE")
    if old is None:
        os.environ["METRAN_HIP_CACHE"] = str(tmp_path_factory.getbasetemp() / "mkjit")
    yield
    if old is None:
        os.environ.pop("METRAN_HIP_CACHE", None)


def _engine(g, layout, packed_sym):
    from metran_amd.engine import BatchedKalman

    kf = BatchedKalman(0, layout=layout, packed_sym=packed_sym)
    kf.set_observations(g["obs"]).set_loadings(g["loadings"], g["obsvar"])
    kf.set_variant("kernel_family", "specialised")
    kf.set_variant("smoother16", "record")
    kf.projection_path = "records"
    return kf


def _check(res, g, warmup, keys, what, unpack=None):
    """The filter's part of a result against the oracle: the moments in ``keys``, mle at ``warmup``, sigmacount, and the pads."""
    np_ = ta._np
    got = {k: np_(unpack(res[k]) if unpack is not None and k in ("Pf", "Pp") else res[k]) for k in keys + ("mle", "sigmacount", "sigmas", "detfs")}
    assert int(np.abs(np_(res["status"]).astype(np.int64)).sum()) == 0, what
    for i in range(g["B"]):
        ref = cf.reference(g, i, warmup, parts=("state",))
        w, rec, sc = "%s, warm-up %d: T = %d, %s" % (what, warmup, g["T"], cf._what(g, i)), ref["rec"], ref["sigmacount"]
        assert int(got["sigmacount"][i]) == sc, w
        cf.assert_close("mle", got["mle"][i], ref["mle"], g, rec, w)
        cf.assert_close("sigmas", got["sigmas"][i, :sc], ref["sigmas"][:sc], g, rec, w)
        cf.assert_close("detfs", got["detfs"][i, :sc], ref["detfs"][:sc], g, rec, w)
        assert not got["sigmas"][i, sc:].any() and not got["detfs"][i, sc:].any(), w + ": the pads behind the last entry are not zero"
        for k in keys:
            cf.assert_close(k, got[k][i], ref[k], g, rec, w)
    return got


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_deferred_emission(shape, B):
    N, K = shape
    for T in LENGTHS:
        for pattern in PATTERNS:
            g = group(N, K, B, T, pattern)
            if g is None:
                continue
            for li, layout in enumerate(LAYOUTS):
                for si, sym in enumerate((False, True)):
                    kf = _engine(g, layout, sym)
                    unpack = kf.unpack_sym if sym else None
                    w_both, w_filt = ((0, 2), (2, 0))[(li + si) % 2]
                    what = "(%d,%d) B = %d, %s, %s, %s" % (N, K, B, pattern, layout, "packed-symmetric" if sym else "full-square")
                    _check(kf.filter_smooth(g["phi"], g["q"], warmup=w_both, **cf.init(g)), g, w_both, ("F", "Pf", "Xp", "Pp"),
                           what + ", both records", unpack)
                    _check(kf.simulate_smoothed(g["phi"], g["q"], warmup=w_filt, **cf.init(g)), g, w_filt, ("F", "Pf"),
                           what + ", filtered record only", unpack)
                    kf.close()

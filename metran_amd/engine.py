"""Batched MI355X engine: thousands of independent Metran dynamic-factor models per launch.

Host-side plumbing only (device memory and streams come from PyTorch-ROCm); every
number is produced by the HIP kernels behind the C ABI (``include/metran_hip.h``).

Mirrors, batched over a leading axis, the reference call chain
``SPKalmanFilter.set_observations -> set_matrices -> run_filter / run_smoother -> get_mle /
simulate / decompose`` (/root/reference/metran/kalmanfilter.py:520-778) and
``Metran._get_matrices`` (metran/metran.py:386-416).
"""
import ctypes
import logging

import numpy as np

from . import _lib
from ._lib import (BlockRequest, ForecastRequest, FunctionalRequest, MetranHipError, Outputs, Problem, RegressionRequest, ScoresRequest,
                   ShiftRequest, WeightsRequest, check)

logger = logging.getLogger(__name__)

__all__ = ["BatchedKalman", "MetranHipError", "FLAG_NONPOSITIVE_F", "FLAG_NOT_SPD", "FLAG_RANK_DEFICIENT"]

FLAG_NONPOSITIVE_F = 1
FLAG_NOT_SPD = 2
FLAG_RANK_DEFICIENT = 4  # informational: a null direction of Pp was dropped, as the reference's pinv does

_STATE_OUTPUTS = ("F", "Pf", "Xp", "Pp", "S", "Ps")


def _torch():
    import torch

    return torch


class BatchedKalman:
    """One context per (process, GPU).

    Parameters
    ----------
    device : int or torch.device, optional
        CUDA/HIP device index; default ``torch.cuda.current_device()``.

    Typical use::

        kf = BatchedKalman()
        kf.set_observations(obs)            # [R,T,N], NaN = missing; uploaded once
        kf.set_loadings(loadings)           # [R,N,K]
        mle = kf.loglik(phi, q)             # [B] -2 log L, B = k*R instances
        out = kf.filter_smooth(phi, q)      # dict of device tensors F,Pf,Xp,Pp,S,Ps,mle,...
    """

    def __init__(self, device=None, layout="model_major", packed_sym=False):
        """layout: "model_major" -- per-step arrays are ``[B,T,...]`` contiguous (the reference's
        per-model arrays stacked); "time_major" -- the memory is ``[T,B,...]`` (one time step of all
        models contiguous: every wavefront's stores land next to its neighbours', which is what HBM
        wants) and the tensors handed back are ``[B,T,...]`` *views* of it, so indexing is unchanged."""
        torch = _torch()
        if layout not in ("model_major", "time_major"):
            raise ValueError("layout must be 'model_major' or 'time_major'")
        self.time_major = layout == "time_major"
        self.packed_sym = bool(packed_sym)
        # simulate_smoothed of wide models: "auto" = the inverse-free tape path where it applies (MK_OUT_TAPE: 16 < n
        # <= 63), else filtered records + RTS smoother; "tape" insists, "records" never uses it
        self.projection_path = "auto"
        L = _lib.lib()  # raises MetranHipError when the HIP library is not built
        if not torch.cuda.is_available():
            raise MetranHipError("no GPU visible to PyTorch-ROCm; metran_amd has no CPU fallback")
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        self._L = L
        ctx = ctypes.c_void_p()
        check(L.mk_create(self.device.index, ctypes.byref(ctx)))
        self._ctx = ctx
        self.obs = None
        self.loadings = None
        self.obsvar = None
        self.scale = None
        self.offset = None
        self.R = self.T = self.N = self.K = None
        self._timing = False
        for which, name in type(self).default_variants.items():
            self.set_variant(which, name)

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "_ctx", None):
            self._L.mk_destroy(self._ctx)
            self._ctx = None
            self._has_comm = False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ kernel variants (A/B measurements)
    _VARIANTS = {"smoother16": (0, ("record", "blk", "record_general")),
                 "wide_smoother": (1, ("mfma", "v1", "mfma_unfolded")),
                 "wide_filter": (2, ("auto", "lane_per_state", "split")),
                 "single_record": (3, ("sparse", "stepwise")),
                 "kernel_family": (4, ("specialised", "generic")),
                 "tape_filter": (5, ("observable", "state"))}
    # variants every new engine starts with (name -> value); empty = the library's defaults.  The GPU test tier sets
    # {"wide_filter": "split"} so that its small batches keep exercising the split kernels, which "auto" reserves for
    # batches of more than two models per SIMD (tests/conftest.py; tests/test_hip_layouts.py checks "auto" itself)
    default_variants = {}

    def set_variant(self, which, name):
        """Choose between two equivalent kernels of a shape class (``mk_set_kernel_variant``): ``"smoother16"``:
        ``"record"`` (default) | ``"blk"`` | ``"record_general"`` (the record kernel without the rank-K covariance step of
        fully observed steps); ``"wide_smoother"``: ``"mfma"`` (default) | ``"v1"`` (built for N + K <= 51) | ``"mfma_unfolded"``; ``"wide_filter"``: ``"auto"`` (default: the split
        layout for more than two models per SIMD, one state per lane below) | ``"lane_per_state"`` | ``"split"``; ``"tape_filter"``
        (the writer of the backward tape, N <= 32): ``"observable"`` (default: the filter in the observable basis) | ``"state"``.
        Every member is tested against the oracle; there is no environment switch."""
        sel, names = self._VARIANTS[which]
        check(self._L.mk_set_kernel_variant(self._ctx, sel, names.index(name)))
        return self

    def resolved_wide_filter(self, B):
        """The wide-filter kernel ``"auto"`` picks for B instances (``mk_kernels.hip`` dispatch_filter: the split layout above
        two wavefronts per SIMD, one state per lane below)."""
        v = self.get_variant("wide_filter")
        if v != "auto":
            return v
        torch = _torch()
        simds = 4 * torch.cuda.get_device_properties(self.device).multi_processor_count
        return "split" if B > 2 * simds else "lane_per_state"

    def get_variant(self, which):
        sel, names = self._VARIANTS[which]
        v = ctypes.c_int(-1)
        check(self._L.mk_get_kernel_variant(self._ctx, sel, ctypes.byref(v)))
        return names[v.value]

    # ------------------------------------------------------------------ helpers
    def _dev(self, a, shape=None, name="array"):
        """float64 contiguous tensor on this device (accepts numpy / torch)."""
        torch = _torch()
        if a is None:
            return None
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
        a = a.to(device=self.device, dtype=torch.float64).contiguous()
        if shape is not None and tuple(a.shape) != tuple(shape):
            raise ValueError("%s has shape %s, expected %s" % (name, tuple(a.shape), tuple(shape)))
        return a

    def _bind_stream(self):
        torch = _torch()
        s = torch.cuda.current_stream(self.device).cuda_stream
        check(self._L.mk_set_stream(self._ctx, ctypes.c_void_p(s)))

    @staticmethod
    def _p(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    # ------------------------------------------------------------------ inputs
    def set_observations(self, obs):
        """Upload observation records ``[R,T,N]`` (or ``[T,N]``); NaN/inf = missing
        (reference packing: metran/kalmanfilter.py:646-674)."""
        torch = _torch()
        if not isinstance(obs, torch.Tensor):
            obs = np.asarray(obs, dtype=np.float64)
        if obs.ndim == 2:
            obs = obs[None]
        if obs.ndim != 3:
            raise ValueError("observations must be [R,T,N] or [T,N]")
        obs = self._dev(obs)
        # the reference finds valid entries with "(x + 1e10).nonzero()" (kalmanfilter.py:666-667): a finite
        # observation of exactly -1e10 is dropped there, so it is a missing value here too
        obs = torch.where(obs == -1e10, torch.full_like(obs, float("nan")), obs)
        self.obs = self._layout(obs)
        self._obs_unmasked = None
        self._obs_unadjusted = None
        self._grad_pending = self._grad_alpha = None  # a pending forward pass belongs to the previous dataset
        self.R, self.T, self.N = (int(s) for s in self.obs.shape)
        check(self._L.mk_observations_changed(self._ctx))  # a recycled allocation may carry a new record at an old address
        return self

    # ------------------------------------------------------------------ ingestion
    def standardize(self, obs=None):
        """``Metran.standardize`` (metran/metran.py:102-121) for every record on the device: per series,
        subtract the mean and divide by the standard deviation (NaN skipped, ddof = 1).  ``obs`` are raw
        series ``[R,T,N]`` (default: the records already set).  The standardised records become the
        engine's observations and ``(std, mean)`` its scaling (``set_scaling``), so that
        ``simulate_smoothed`` returns values in the original units; returns ``(mean, std)`` ``[R,N]``."""
        torch = _torch()
        if obs is not None:
            self.set_observations(obs)
        if self.obs is None:
            raise MetranHipError("call set_observations first")
        if self.N > 64:
            raise MetranHipError("standardize supports N <= 64 series per model")
        mean = torch.empty((self.R, self.N), dtype=torch.float64, device=self.device)
        std = torch.empty_like(mean)
        self._bind_stream()
        check(self._L.mk_standardize(self._ctx, self.R, self.T, self.N, int(self.time_major), self._p(self.obs),
                                     self._p(self.obs), self._p(mean), self._p(std)))
        self._obs_unmasked = self._obs_unadjusted = None
        self.scale, self.offset = std, mean
        check(self._L.mk_observations_changed(self._ctx))  # standardised in place
        return mean, std

    def mask_observations(self, mask):
        """``Metran.mask_observations`` (metran/metran.py:464-494): hide the observations where ``mask``
        ``[R,T,N]`` is non-zero.  The unmasked records stay on the device; ``unmask_observations`` is free."""
        torch = _torch()
        if self.obs is None:
            raise MetranHipError("call set_observations first")
        base = self._obs_unmasked if getattr(self, "_obs_unmasked", None) is not None else self.obs
        if not isinstance(mask, torch.Tensor):
            mask = torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0).view(np.uint8))
        mask = (mask != 0).to(device=self.device, dtype=torch.uint8)
        if mask.ndim == 2:
            mask = mask[None]
        if tuple(mask.shape) != (self.R, self.T, self.N):
            raise ValueError("Dimensions of mask %s do not equal dimensions of series %s"
                             % (tuple(mask.shape), (self.R, self.T, self.N)))  # metran.py:484-491
        mask = self._layout(mask)
        out = torch.empty_like(base)
        self._bind_stream()
        check(self._L.mk_mask_observations(self._ctx, int(base.numel()), self._p(base), self._p(mask), self._p(out)))
        self._obs_unmasked = base
        self.obs = out
        check(self._L.mk_observations_changed(self._ctx))
        return self

    def unmask_observations(self):
        """``Metran.unmask_observations`` (metran/metran.py:496-506)."""
        if getattr(self, "_obs_unmasked", None) is not None:
            self.obs = self._obs_unmasked
            self._obs_unmasked = None
            check(self._L.mk_observations_changed(self._ctx))
        return self

    def pack_observations(self):
        """``SPKalmanFilter.set_observations`` (metran/kalmanfilter.py:646-674) for every record:
        ``(observations [R,T,N], observation_indices [R,T,N] float64, observation_count [R,T] int64)``."""
        torch = _torch()
        if self.obs is None:
            raise MetranHipError("call set_observations first")
        observations = torch.empty_like(self.obs)
        indices = torch.empty_like(self.obs)
        count = self._empty_bt(self.R, self.T, dtype=torch.int64)
        # the kernel walks the R*T rows in memory order, whichever layout that is
        self._bind_stream()
        check(self._L.mk_pack_observations(self._ctx, self.R * self.T, 1, self.N, self._p(self.obs),
                                           self._p(observations), self._p(indices), self._p(count)))
        return observations, indices, count

    def _layout(self, t):
        """Logical ``[B,T,...]`` tensor whose memory follows the engine's layout."""
        if not self.time_major:
            return t.contiguous()
        if t.transpose(0, 1).is_contiguous():
            return t
        return t.transpose(0, 1).contiguous().transpose(0, 1)

    def _empty_bt(self, B, T, *rest, dtype=None):
        torch = _torch()
        dtype = dtype or torch.float64
        if self.time_major:
            return torch.empty((T, B) + tuple(rest), dtype=dtype, device=self.device).transpose(0, 1)
        return torch.empty((B, T) + tuple(rest), dtype=dtype, device=self.device)

    def set_loadings(self, loadings, obsvar=None):
        """Factor loadings ``[R,N,K]`` (``Z = [I | loadings]``, metran/metran.py:365-370) and
        optional observation variances ``[R,N]`` (zeros in Metran, metran/metran.py:382-384)."""
        torch = _torch()
        if self.obs is None:
            raise MetranHipError("call set_observations first")
        if not isinstance(loadings, torch.Tensor):
            loadings = np.asarray(loadings, dtype=np.float64)
        if loadings.ndim == 2:
            loadings = loadings[None]
        self.loadings = self._dev(loadings)
        self._grad_pending = self._grad_alpha = None  # ... and to the previous loadings
        if tuple(self.loadings.shape[:2]) != (self.R, self.N):
            raise ValueError("loadings must be [R=%d,N=%d,K], got %s" % (self.R, self.N, tuple(self.loadings.shape)))
        self.K = int(self.loadings.shape[2])
        self._ensure_kernels()
        if obsvar is not None:
            if not isinstance(obsvar, torch.Tensor):
                obsvar = np.asarray(obsvar, dtype=np.float64)
            if obsvar.ndim == 1:
                obsvar = obsvar[None]
            self.obsvar = self._dev(obsvar, (self.R, self.N), "obsvar")
        else:
            self.obsvar = None
        return self

    def _ensure_kernels(self):
        """Kernels for this engine's (N, K).  A shape of the ahead-of-time list runs as it is; any other shape with
        N + K <= 64 gets its own specialised module (``metran_amd/jit.py``: prebuilt under ``metran_amd/_shape_cache``, cached
        per user, or compiled now by hipcc); where that is not possible -- no hipcc on the machine, ``METRAN_HIP_JIT=0``,
        or N + K > 64 -- the size-generic kernels serve the shape (``mk_generic.hip``, N + K <= 128: correct for every
        shape, an order of magnitude slower; no packed-symmetric records, tape or adjoint gradient)."""
        if self._L.mk_shape_specialised(self.N, self.K):
            return
        why = None
        if self.n <= 64:
            from . import jit

            try:
                jit.ensure_shape(self.N, self.K)  # builds + registers a specialised kernel module (cached)
                return
            except jit.ShapeUnavailable as e:   # no compiler / METRAN_HIP_JIT=0: the size-generic kernels serve the shape.
                why = str(e).splitlines()[0]    # A FAILED build (hipcc, link, hazard check: jit.ShapeBuildError) propagates --
                                                # it must not hide behind kernels ten times slower (round-5 advice)
        if not self._L.mk_shape_supported(self.N, self.K):
            raise MetranHipError("a model of N=%d series and K=%d factors has %d states; the library serves N + K <= %d"
                                 % (self.N, self.K, self.n, int(self._L.mk_generic_max_states())))
        if self.packed_sym:
            raise MetranHipError("packed-symmetric records need specialised kernels; (N=%d, K=%d) runs the size-generic ones%s"
                                 % (self.N, self.K, " (%s)" % why if why else ""))
        logger.warning("(N=%d, K=%d) runs the size-generic kernels%s -- correct, about an order of magnitude slower, no adjoint "
                       "gradient / tape / packed-symmetric records", self.N, self.K, ": " + why if why else " (N + K > 64)")

    def specialised(self):
        """True when this engine's shape runs the specialised (unrolled, one-state-per-lane) kernels, False for the size-generic ones."""
        return bool(self._L.mk_shape_specialised(self.N, self.K))

    def subset(self, index):
        """A new engine holding the records ``index`` (1-D integer tensor / array of record numbers) of this one: the
        observations, loadings and observation variances are gathered on the device (what ``calibrate_batch`` does when
        most of its models have converged: the remaining iterations run on the still-active records only)."""
        torch = _torch()
        index = torch.as_tensor(index, dtype=torch.long, device=self.device)
        sub = BatchedKalman(self.device.index, layout="time_major" if self.time_major else "model_major",
                            packed_sym=self.packed_sym)
        # the sub-engine runs the SAME kernels as its parent: the user's variants and projection path carry over, and
        # "auto" (a rule on the batch size) is pinned to what it resolves to for the parent's record count -- so a model
        # sees bit-identical results whether or not calibrate_batch compacted the flight around it
        sub.projection_path = self.projection_path
        for which in self._VARIANTS:
            sub.set_variant(which, self.get_variant(which))
        if self.get_variant("wide_filter") == "auto" and self.R is not None:
            sub.set_variant("wide_filter", self.resolved_wide_filter(self.R))
        sub.set_observations(self.obs[index])
        sub.set_loadings(self.loadings[index], None if self.obsvar is None else self.obsvar[index])
        if self.scale is not None:
            sub.scale, sub.offset = self.scale[index].contiguous(), self.offset[index].contiguous()
        # the sub-engine takes over the parent's adjoint workspace (a subset never needs more of it; at 8192 x (8,2), T = 1000 it is
        # 7.3 GB, and a fresh 3 GB allocation for the first compacted flight was the largest single item of a calibration's wall
        # time).  The two are used one after the other (calibrate_batch returns to the parent when the flight has finished); a
        # forward pass still waiting for its backward pass on the parent is void from here on.  Interleaved use is not supported:
        # The buffer carries an OWNER token shared by everybody who holds it (round-5 advice): whoever starts a forward pass
        # takes the token, and a backward pass whose engine no longer holds it raises instead of walking somebody else's records.
        work = getattr(self, "_grad_work", None)
        if work is not None:
            sub._grad_work = work
            sub._grad_share = self._grad_share = getattr(self, "_grad_share", None) or {"owner": None}
            self._grad_pending = None
        sub.adjoint_updates = self.adjoint_updates
        if getattr(self, "_grad_upd", None) is not None:   # ... and so does the update tape of the wide adjoint gradient
            sub._grad_upd = self._grad_upd
        return sub

    @property
    def n(self):
        return self.N + self.K

    def params_from_alpha(self, alpha, dt=1.0):
        """``alpha [B,n] -> (phi, q)`` on device (Metran._get_matrices diagonals, metran.py:246-322)."""
        torch = _torch()
        alpha = self._dev(alpha)
        if alpha.ndim == 1:
            alpha = alpha[None]
        B = int(alpha.shape[0])
        if alpha.shape[1] != self.n:
            raise ValueError("alpha must be [B,%d]" % self.n)
        phi = torch.empty_like(alpha)
        q = torch.empty_like(alpha)
        self._bind_stream()
        check(self._L.mk_params_from_alpha(self._ctx, B, self.R, self.N, self.K, self._p(alpha),
                                           self._p(self.loadings), float(dt), self._p(phi), self._p(q)))
        return phi, q

    def _problem(self, phi, q, warmup, x0, P0):
        if self.obs is None or self.loadings is None:
            raise MetranHipError("set_observations and set_loadings must be called before running the filter")
        phi = self._dev(phi)
        q = self._dev(q)
        if phi.ndim == 1:
            phi = phi[None]
        if q.ndim == 1:
            q = q[None]
        B = int(phi.shape[0])
        if tuple(phi.shape) != (B, self.n) or tuple(q.shape) != (B, self.n):
            raise ValueError("phi and q must be [B,%d]; got %s, %s" % (self.n, tuple(phi.shape), tuple(q.shape)))
        if B % self.R != 0:
            raise ValueError("number of instances B=%d must be a multiple of the number of records R=%d" % (B, self.R))
        x0 = self._dev(x0, (B, self.n), "x0") if x0 is not None else None
        P0 = self._dev(P0, (B, self.n, self.n), "P0") if P0 is not None else None
        prob = Problem(B, self.R, self.T, self.N, self.K, int(warmup), self._p(self.obs), self._p(phi), self._p(q),
                       self._p(self.loadings), self._p(self.obsvar), self._p(x0), self._p(P0),
                       1 if self.time_major else 0, self._p(self.scale), self._p(self.offset))
        keep = (phi, q, x0, P0)
        return prob, keep, B

    # ------------------------------------------------------------------ hot path
    def loglik(self, phi, q, warmup=1, x0=None, P0=None, out=None):
        """-2 log L per instance (``Metran.get_mle`` objective, metran/metran.py:605-622)."""
        torch = _torch()
        prob, keep, B = self._problem(phi, q, warmup, x0, P0)
        mle = out if out is not None else torch.empty(B, dtype=torch.float64, device=self.device)
        self._bind_stream()
        check(self._L.mk_loglik(self._ctx, ctypes.byref(prob), self._p(mle)))
        return mle

    def loglik_grad(self, phi, q, warmup=1, x0=None, P0=None):
        """Objective and its ADJOINT gradient: ``(mle [B], gphi [B,n], gq [B,n])`` with
        ``gphi = d(-2 log L)/d phi``, ``gq = d(-2 log L)/d q`` in two launches (forward filter writing the
        filtered records into a workspace that is kept between calls, then the backward adjoint kernel).
        The reference has no gradient (metran/solver.py:248-255 leaves scipy to difference P+1 runs).
        Any supported shape: four models per wavefront for n <= 16, one per wavefront for 16 < n <= 64."""
        torch = _torch()
        prob, keep, B = self._problem(phi, q, warmup, x0, P0)
        self._grad_pending = None  # the shared workspace is about to be overwritten: a forward pass waiting for its backward is void
        need = B * self.T * self.record_stride()
        work = self._take_grad_work(need)
        self._ensure_grad_updates(B)
        mle = torch.empty(B, dtype=torch.float64, device=self.device)
        sc = torch.empty(B, dtype=torch.int64, device=self.device)
        gphi = torch.empty((B, self.n), dtype=torch.float64, device=self.device)
        gq = torch.empty_like(gphi)
        self._bind_stream()
        check(self._L.mk_loglik_grad(self._ctx, ctypes.byref(prob), self._p(work), 1 if self.time_major else 0,
                                     self._p(mle), self._p(sc), self._p(gphi), self._p(gq), None))
        return mle, gphi, gq

    # the update tape of the wide adjoint gradient (C ABI mk_set_adjoint_updates; round 6): True = allocate and use it where the
    # shape has one (16 < N + K <= 64) and it fits in 40 % of the free memory, False = the backward walk recomputes every step
    adjoint_updates = True

    def _ensure_grad_updates(self, B):
        torch = _torch()
        us = int(self._L.mk_adjoint_update_stride(self.N, self.K)) if self.adjoint_updates else 0
        buf = getattr(self, "_grad_upd", None)
        need = B * self.T * us
        if us and (buf is None or buf.numel() < need):
            free = float(torch.cuda.mem_get_info(self.device)[0])
            buf = torch.empty(need, dtype=torch.float64, device=self.device) if 8.0 * need <= 0.4 * free else None
            self._grad_upd = buf
            self._grad_upd_set = None
        if not us:
            buf = None
        key = None if buf is None else (buf.data_ptr(), buf.numel())
        if getattr(self, "_grad_upd_set", "unset") != key:   # (the context keeps the pointer: tell it only when it changes)
            check(self._L.mk_set_adjoint_updates(self._ctx, self._p(buf), 0 if buf is None else int(buf.numel())))
            self._grad_upd_set = key

    def _take_grad_work(self, need):
        """The adjoint workspace (at least ``need`` doubles), with this engine as the owner of its contents from now on: an
        engine sharing the buffer (``subset``) that still waits for a backward pass will refuse to run it."""
        torch = _torch()
        work = getattr(self, "_grad_work", None)
        if work is None or work.numel() < need:
            self._grad_work = work = torch.empty(need, dtype=torch.float64, device=self.device)
            self._grad_share = None          # a fresh buffer is nobody else's
        self._grad_token = object()
        if getattr(self, "_grad_share", None) is not None:
            self._grad_share["owner"] = self._grad_token
        return work

    def loglik_forward(self, phi, q, warmup=1, x0=None, P0=None):
        """The forward half of ``loglik_grad`` alone (``mk_loglik_grad_phases``, MK_GRAD_FORWARD): ``mle [B]``, with the
        filtered records left in the workspace.  ``loglik_backward()`` then returns the gradient AT THESE parameters
        without filtering them again -- a line search evaluates several trial points and wants the gradient of the last
        one only."""
        torch = _torch()
        prob, keep, B = self._problem(phi, q, warmup, x0, P0)
        need = B * self.T * self.record_stride()
        work = self._take_grad_work(need)
        self._ensure_grad_updates(B)
        mle = torch.empty(B, dtype=torch.float64, device=self.device)
        sc = torch.empty(B, dtype=torch.int64, device=self.device)
        self._bind_stream()
        check(self._L.mk_loglik_grad_phases(self._ctx, ctypes.byref(prob), self._p(work), 1 if self.time_major else 0,
                                            self._p(mle), self._p(sc), None, None, None, 1))
        # everything the backward launch dereferences stays alive with the pending record (the parameter tensors in `keep`,
        # the observation / loadings / variance tensors the problem struct points at); set_observations, set_loadings and
        # loglik_grad void it (round-3 advice: a backward pass over records of another parameter set or dataset returned a
        # wrong gradient without an error)
        self._grad_pending = (prob, keep + (self.obs, self.loadings, self.obsvar), B, sc, work)
        self._grad_alpha = None
        return mle

    def loglik_backward(self):
        """``(gphi [B,n], gq [B,n])`` at the parameters of the last ``loglik_forward`` (MK_GRAD_BACKWARD)."""
        torch = _torch()
        pending = getattr(self, "_grad_pending", None)
        if pending is None:
            raise MetranHipError("loglik_backward without a preceding loglik_forward")
        share = getattr(self, "_grad_share", None)
        if share is not None and share["owner"] is not self._grad_token:
            self._grad_pending = None
            raise MetranHipError("the records of this engine's forward pass have been overwritten: the adjoint workspace is shared with "
                                 "another engine (BatchedKalman.subset) that ran a forward pass since -- use the two one after the other")
        prob, keep, B, sc, work = pending
        gphi = torch.empty((B, self.n), dtype=torch.float64, device=self.device)
        gq = torch.empty_like(gphi)
        self._bind_stream()
        check(self._L.mk_loglik_grad_phases(self._ctx, ctypes.byref(prob), self._p(work), 1 if self.time_major else 0,
                                            None, self._p(sc), self._p(gphi), self._p(gq), None, 2))
        self._grad_pending = None  # one backward pass per forward pass
        return gphi, gq

    def loglik_forward_alpha(self, alpha, dt=1.0, warmup=1):
        """``loglik_forward`` in Metran's parametrisation; ``loglik_backward_alpha()`` completes it."""
        alpha = self._dev(alpha)
        if alpha.ndim == 1:
            alpha = alpha[None]
        phi, q = self.params_from_alpha(alpha, dt=dt)
        mle = self.loglik_forward(phi, q, warmup=warmup)
        self._grad_alpha = (alpha, float(dt))
        return mle

    def loglik_backward_alpha(self):
        """``d mle / d alpha [B,n]`` at the point of the last ``loglik_forward_alpha``."""
        torch = _torch()
        if getattr(self, "_grad_alpha", None) is None:
            raise MetranHipError("loglik_backward_alpha without a preceding loglik_forward_alpha")
        alpha, dt = self._grad_alpha
        gphi, gq = self.loglik_backward()
        self._grad_alpha = None
        galpha = torch.empty_like(gphi)
        check(self._L.mk_alpha_grad(self._ctx, int(alpha.shape[0]), self.R, self.N, self.K, self._p(alpha),
                                    self._p(self.loadings), dt, self._p(gphi), self._p(gq), self._p(galpha)))
        return galpha

    def has_adjoint(self):
        """Whether ``loglik_grad`` (``mk_loglik_grad``) serves this engine's shape: ``adjoint_kernel`` for n <= 16 (four
        models per wavefront), ``adjoint_wide_kernel`` for 16 < n <= 64 (one model per wavefront)."""
        return self.N is not None and self.n <= 64 and self.specialised() and self.get_variant("kernel_family") == "specialised"

    def loglik_grad_alpha(self, alpha, dt=1.0, warmup=1):
        """``(mle [B], d mle / d alpha [B,n])`` for Metran's parametrisation (``params_from_alpha`` forward,
        ``mk_alpha_grad`` chain rule backward)."""
        torch = _torch()
        alpha = self._dev(alpha)
        if alpha.ndim == 1:
            alpha = alpha[None]
        phi, q = self.params_from_alpha(alpha, dt=dt)
        mle, gphi, gq = self.loglik_grad(phi, q, warmup=warmup)
        galpha = torch.empty_like(gphi)
        check(self._L.mk_alpha_grad(self._ctx, int(alpha.shape[0]), self.R, self.N, self.K, self._p(alpha),
                                    self._p(self.loadings), float(dt), self._p(gphi), self._p(gq), self._p(galpha)))
        return mle, galpha

    def record_stride(self):
        """Doubles per packed (model, step) record for this state dimension (C ABI ``mk_record_stride``, or
        ``mk_record_stride_sym`` for an engine created with ``packed_sym=True``)."""
        if self.packed_sym:
            return int(self._L.mk_record_stride_sym(self.n))
        return int(self._L.mk_record_stride(self.n))

    def unpack_sym(self, packed):
        """Packed upper triangle ``[..., n(n+1)/2]`` (what the covariance entries of a ``packed_sym`` engine's results
        are) -> full symmetric ``[..., n, n]``.  Lazy by design: the packed records are what moves through HBM."""
        torch = _torch()
        n = self.n
        idx = getattr(self, "_sym_index", None)
        if idx is None or idx.shape[0] != n:
            r = torch.arange(n, device=self.device)
            lo, hi = torch.minimum(r[:, None], r[None, :]), torch.maximum(r[:, None], r[None, :])
            idx = self._sym_index = lo * n - (lo * (lo - 1)) // 2 + (hi - lo)
        return packed[..., idx]

    def _alloc_records(self, B):
        """One record array ``[B,T,RS]`` (logical; memory follows the engine layout) and its views
        ``(mean [B,T,n], cov [B,T,n,n], pad0 [B,T], pad1 [B,T])``."""
        T, n = self.T, self.n
        RS = self.record_stride()
        rec = self._empty_bt(B, T, RS)
        if self.packed_sym:  # covariance entry = the packed upper triangle [B,T,n(n+1)/2]; see unpack_sym
            nv = n + n * (n + 1) // 2
            return rec, rec[..., :n], rec[..., n:nv], rec[..., nv], rec[..., nv + 1]
        nv = n + n * n
        return rec, rec[..., :n], rec[..., n:nv].unflatten(-1, (n, n)), rec[..., nv], rec[..., nv + 1]

    def _alloc_outputs(self, B, want, bookkeeping=True):
        """Output tensors for one launch.  When the predicted and filtered moments (and, if any, both
        smoothed moments) are all requested, they are allocated as PACKED RECORDS (the kernels' fast
        path, see ``mk_outputs.record_stride``) and the entries of the returned dict are views."""
        torch = _torch()
        T, n = self.T, self.n
        f64 = dict(dtype=torch.float64, device=self.device)
        want = list(want)
        for k in want:
            if k not in _STATE_OUTPUTS:
                raise ValueError("unknown output %r (choose from %s)" % (k, _STATE_OUTPUTS))
        res = {"mle": torch.empty(B, **f64)}
        res["status"] = torch.zeros(B, dtype=torch.int32, device=self.device)
        if bookkeeping:
            res["sigmacount"] = torch.empty(B, dtype=torch.int64, device=self.device)
        smooth_pair = ("S" in want) + ("Ps" in want)
        records = all(k in want for k in ("F", "Pf", "Xp", "Pp")) and smooth_pair in (0, 2)
        if self.packed_sym and not records:
            raise MetranHipError("a packed_sym engine writes record outputs only: ask for F, Pf, Xp, Pp (and S, Ps), "
                                 "or use simulate_smoothed / smooth_state_variances")
        if records:
            res["_rs"] = self.record_stride()
            res["_rec_pred"], res["Xp"], res["Pp"], _, _ = self._alloc_records(B)
            res["_rec_filt"], res["F"], res["Pf"], sig, det = self._alloc_records(B)
            if bookkeeping:
                res["sigmas"], res["detfs"] = sig, det
            if smooth_pair:
                res["_rec_smooth"], res["S"], res["Ps"], _, _ = self._alloc_records(B)
            return res
        if bookkeeping:
            res["sigmas"] = self._empty_bt(B, T)
            res["detfs"] = self._empty_bt(B, T)
        for k in want:
            res[k] = self._empty_bt(B, T, n) if k in ("F", "Xp", "S") else self._empty_bt(B, T, n, n)
        return res

    def _outputs_struct(self, res):
        g = res.get
        return Outputs(self._p(g("mle")), self._p(g("sigmas")), self._p(g("detfs")), self._p(g("sigmacount")),
                       self._p(g("F")), self._p(g("Pf")), self._p(g("Xp")), self._p(g("Pp")), self._p(g("S")),
                       self._p(g("Ps")), self._p(g("status")), 1 if self.time_major else 0,
                       self._p(g("sim_means")), self._p(g("sim_vars")), int(g("_rs", 0)),
                       (1 if (self.packed_sym and g("_rs", 0) and not g("_tape")) else 0) | (2 if g("_var_only") else 0)
                       | (4 if g("_tape") else 0))

    def filter(self, phi, q, warmup=1, x0=None, P0=None, outputs=("F", "Pf", "Xp", "Pp"), buffers=None):
        """``run_filter`` for B instances (kalmanfilter.py:696-778).  Returns a dict of device tensors."""
        prob, keep, B = self._problem(phi, q, warmup, x0, P0)
        res = buffers if buffers is not None else self._alloc_outputs(B, [o for o in outputs if o not in ("S", "Ps")])
        o = self._outputs_struct(res)
        self._bind_stream()
        check(self._L.mk_filter(self._ctx, ctypes.byref(prob), ctypes.byref(o)))
        return res

    def filter_smooth(self, phi, q, warmup=1, x0=None, P0=None, outputs=_STATE_OUTPUTS, buffers=None):
        """``run_smoother`` for B instances (kalmanfilter.py:676-694): filter, then RTS smoother."""
        want = set(outputs) | {"F", "Pf"}  # the backward pass re-reads the filtered moments
        if {"Xp", "Pp"} <= want:
            want |= {"S", "Ps"}  # full output set -> packed records for all three moment sets
        prob, keep, B = self._problem(phi, q, warmup, x0, P0)
        res = buffers if buffers is not None else self._alloc_outputs(B, [k for k in _STATE_OUTPUTS if k in want])
        o = self._outputs_struct(res)
        self._bind_stream()
        check(self._L.mk_filter_smooth(self._ctx, ctypes.byref(prob), ctypes.byref(o)))
        return res

    def set_scaling(self, scale=None, offset=None):
        """Series standard deviations / means ``[R,N]`` for the fused projection (``Metran.oseries_std`` /
        ``oseries_mean``; the scaled observation matrix of metran/metran.py:944-961).  None = 1 / 0."""
        def prep(a):
            if a is None:
                return None
            torch = _torch()
            if not isinstance(a, torch.Tensor):
                a = np.asarray(a, dtype=np.float64)
            if a.ndim == 1:
                a = a[None]
            return self._dev(a, (self.R, self.N), "scale/offset")
        self.scale, self.offset = prep(scale), prep(offset)
        return self

    def tape_path(self):
        """True when ``simulate_smoothed`` runs the inverse-free backward pass over the filter's tape (``MK_OUT_TAPE``:
        ``mk_split.hip`` OUT = 4 + ``mk_dk.hip``) instead of filtered records + the RTS smoother: wide models served by the
        split filter -- with more than 32 series: by the lane-per-state filter, same tape -- (16 < n <= 63), full-square engine,
        ``projection_path`` not "records"."""
        ok = (self.loadings is not None and not self.packed_sym and bool(self._L.mk_tape_supported(self.N, self.K))
              and self.get_variant("kernel_family") == "specialised")
        if self.projection_path == "tape" and not ok:
            raise MetranHipError("projection_path='tape' needs a model with 16 < N + K <= 63 and a full-square engine "
                                 "(got N=%s, K=%s)" % (self.N, getattr(self, "K", None)))
        return ok and self.projection_path != "records"

    def alloc_projection(self, B):
        """Buffers of ``simulate_smoothed`` for B instances (filtered record array -- or the backward tape, see
        ``tape_path`` -- + projected moments), for callers that run it repeatedly (pass them back as ``buffers=``)."""
        torch = _torch()
        res = {"mle": torch.empty(B, dtype=torch.float64, device=self.device),
               "status": torch.zeros(B, dtype=torch.int32, device=self.device),
               "sigmacount": torch.empty(B, dtype=torch.int64, device=self.device), "_rs": self.record_stride()}
        if self.tape_path():
            res["_rs"] = int(self._L.mk_tape_stride(self.N, self.K))
            res["_tape"] = True
            res["F"] = res["_rec_filt"] = self._empty_bt(B, self.T, res["_rs"])  # d_F = the tape
            res["sim_means"] = self._empty_bt(B, self.T, self.N)
            res["sim_vars"] = self._empty_bt(B, self.T, self.N)
            return res
        res["_rec_filt"], res["F"], res["Pf"], res["sigmas"], res["detfs"] = self._alloc_records(B)
        res["sim_means"] = self._empty_bt(B, self.T, self.N)
        res["sim_vars"] = self._empty_bt(B, self.T, self.N)
        return res

    def simulate_smoothed(self, phi, q, warmup=1, x0=None, P0=None, buffers=None):
        """``Metran.get_simulated_means/variances(method="smoother")`` for B instances in two launches
        WITHOUT materialising the smoothed states: the filter writes only the filtered records, the
        smoother reads them and writes the projected means/variances ``[B,T,N]`` (fused epilogue,
        kalmanfilter.py:569-603 with the scaling set by ``set_scaling``).  Returns a dict with
        ``sim_means, sim_vars, mle, sigmacount, status`` (and the filtered views ``F, Pf``; on the tape path of wide
        models -- ``tape_path`` -- ``F`` is the tape and there is no ``Pf``)."""
        prob, keep, B = self._problem(phi, q, warmup, x0, P0)
        res = buffers if buffers is not None else self.alloc_projection(B)
        o = self._outputs_struct(res)
        self._bind_stream()
        check(self._L.mk_filter_smooth(self._ctx, ctypes.byref(prob), ctypes.byref(o)))
        return res

    # ------------------------------------------------------------------ the record readers: one scaffold
    # loo_predict, disturbances, innovations, forecast, observation_weights, regression, scores, block_predict, level_shifts and functionals (which also runs
    # the smoother) run the recording forward pass into a workspace ("_work") and kernels that read its filtered records.  What a
    # reader keeps to itself is the validation of its request, its shapes and its request struct; the table, _reader_stride,
    # _reader_shapes, _reader_buffers and _reader_call are the rest.
    # reader -> (stride function of the C ABI, specialised kernels only, who reads full-square records only (None: packed-symmetric
    # engines are served too), what the refusal of a shape says is served, allocator)
    _READERS = {
        "loo": ("mk_loo_work_stride", True, None, "leave-one-out predictions serve specialised shapes with N + K <= 63", "alloc_loo"),
        "disturbances": ("mk_disturbance_work_stride", True, None, "state disturbances serve specialised shapes with N + K <= 64",
                         "alloc_disturbances"),
        "innovations": ("mk_innovations_work_stride", False, None, "innovations serve shapes with N + K <= 64", "alloc_innovations"),
        "forecast": ("mk_forecast_work_stride", False, None, "forecasts serve shapes with N + K <= 64", "alloc_forecast"),
        "weights": ("mk_weights_work_stride", False, None, "observation weights serve shapes with N + K <= 64",
                    "alloc_observation_weights"),
        "regression": ("mk_regression_work_stride", False, None, "intervention effects serve shapes with N + K <= 64", "alloc_regression"),
        "scores": ("mk_scores_work_stride", False, "the scores", "per-step scores serve shapes with N + K <= 64", "alloc_scores"),
        "blocks": ("mk_block_work_stride", False, "leave-block-out predictions", "leave-block-out predictions serve shapes with N + K <= 64",
                   "alloc_block_predict"),
        "shifts": ("mk_shift_work_stride", False, "the level-shift scan", "the level-shift scan serves shapes with N + K <= 64",
                   "alloc_level_shifts"),
        "functionals": ("mk_functionals_work_stride", False, "window functionals", "window functionals serve shapes with N + K <= 64",
                        "alloc_functionals"),
    }

    # NOTE: loo_supported() and disturbances_supported() are methods, innovations_supported, forecast_supported,
    # observation_weights_supported, regression_supported, scores_supported, block_predict_supported, level_shifts_supported and functionals_supported properties -- an
    # inconsistency of the public API that is kept.
    def _reader_stride(self, name, refuse=False):
        """Doubles per (instance, step) of the workspace of the record reader ``name``; where the engine is not served 0, or with
        ``refuse`` a MetranHipError."""
        fn, specialised_only, full_square, serves, _ = self._READERS[name]
        if full_square and self.packed_sym:
            if refuse:
                raise MetranHipError("libmetran_hip error -2 (MK_ERR_SHAPE): %s read full-square records; this engine was "
                                     "created with packed_sym=True" % full_square)
            return 0
        served = self.loadings is not None and (not specialised_only or self.get_variant("kernel_family") == "specialised")
        stride = int(getattr(self._L, fn)(self.N, self.K)) if served else 0
        if not stride and refuse:
            raise MetranHipError("%s; (N=%s, K=%s) is not one" % (serves, self.N, getattr(self, "K", None)))
        return stride

    def _reader_shapes(self, B, bt=None, ints=None, **plain):
        """name -> (logical shape, follows the engine's layout, dtype) of a record reader's outputs: the float64 ``[B,T,tail]``
        buffers ``bt`` (key -> tail), the contiguous float64 buffers ``plain`` (key -> shape), the contiguous integer buffers
        ``ints`` (key -> (shape, dtype)) and ``status``."""
        torch = _torch()
        shapes = {key: ((B, self.T, tail), True, torch.float64) for key, tail in (bt or {}).items()}
        for key, shape in plain.items():
            shapes[key] = (shape, False, torch.float64)
        for key, (shape, dtype) in (ints or {}).items():
            shapes[key] = (shape, False, dtype)
        shapes["status"] = ((B,), False, torch.int32)
        return shapes

    def _reader_buffers(self, name, buffers, shapes, stride=None):
        """The buffers of the record reader ``name``: its workspace of ``stride`` doubles per (instance, step) (None: asked for
        here) and what ``shapes`` lists (``_reader_shapes``; the workspace is added to it) -- allocated with a zeroed ``status``,
        or the caller's ``buffers``, every one of them checked before anything is bound or launched."""
        torch = _torch()
        B = shapes["status"][0][0]
        shapes["_work"] = ((B, self.T, stride or self._reader_stride(name, refuse=True)), True, torch.float64)
        if buffers is None:
            return {key: self._empty_bt(*shape, dtype=dtype) if bt else
                    (torch.zeros if key == "status" else torch.empty)(shape, dtype=dtype, device=self.device)
                    for key, (shape, bt, dtype) in shapes.items()}
        for key, (shape, bt, dtype) in shapes.items():
            t = buffers.get(key)
            if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == self.device and t.shape == shape
                    and (t.transpose(0, 1) if bt and self.time_major else t).is_contiguous()):
                raise ValueError("buffers[%r] must be a %s [%s] tensor on %s%s (%s)" % (
                    key, str(dtype).replace("torch.", ""), ", ".join("%d" % d for d in shape), self.device,
                    " in the engine's layout" if bt else ", contiguous", self._READERS[name][-1]))
        return buffers

    def _reader_call(self, entry, prob, res, *specific, mask=()):
        """The tail of every record reader: the C ABI's ``entry(ctx, prob, work, time_major, *specific, status)`` on the current
        stream, then NaN in every row of ``mask`` of the instances whose status carries ``FLAG_NONPOSITIVE_F``."""
        self._bind_stream()
        check(getattr(self._L, entry)(self._ctx, ctypes.byref(prob), self._p(res["_work"]), 1 if self.time_major else 0, *specific,
                                      self._p(res["status"])))
        if mask:
            bad = (res["status"] & FLAG_NONPOSITIVE_F) != 0
            for key in mask:
                res[key].masked_fill_(bad.view((-1,) + (1,) * (res[key].ndim - 1)), float("nan"))
        return res

    # ------------------------------------------------------------------ leave-one-out predictions
    def loo_supported(self):
        """True when ``loo_predict`` serves this engine's shape (C ABI ``mk_loo_work_stride`` > 0): specialised kernels and
        N + K <= 63 -- the adjoint walk over filtered records for N + K <= 16, the tape walk above."""
        return self._reader_stride("loo") > 0

    def _loo_shapes(self, B):
        return self._reader_shapes(B, bt=dict(loo_means=self.N, loo_vars=self.N))

    def alloc_loo(self, B):
        """Buffers of ``loo_predict`` for B instances (the forward pass's workspace + the two outputs), for callers that run
        it repeatedly (pass them back as ``buffers=``)."""
        return self._reader_buffers("loo", None, self._loo_shapes(B))

    def loo_predict(self, phi, q, x0=None, P0=None, buffers=None):
        """LEAVE-ONE-OUT predictions of every observed cell for B instances (C ABI ``mk_loo``): ``loo_means[b,t,j]`` is the
        prediction of observation (t, j) from every OTHER observation of the record and ``loo_vars[b,t,j]`` the variance of
        the projected state z_j x_t under it -- what masking that one cell, smoothing again and reading ``simulate`` at the
        cell gives (Metran's outlier screen, metran.py:464-506 + 831-883), parameters held fixed -- for all cells in two
        launches.  Units as set by ``set_scaling`` (scale / offset of the projection); NaN where a cell is not observed.
        Returns a dict with ``loo_means, loo_vars`` ``[B,T,N]`` and ``status`` (the filter's MK_FLAG_* bits)."""
        stride = self._reader_stride("loo", refuse=True)
        prob, keep, B = self._problem(phi, q, 0, x0, P0)
        res = self._reader_buffers("loo", buffers, self._loo_shapes(B), stride)
        return self._reader_call("mk_loo", prob, res, self._p(res["loo_means"]), self._p(res["loo_vars"]))

    # ------------------------------------------------------------------ smoothed state disturbances
    def disturbances_supported(self):
        """True when ``disturbances`` serves this engine's shape (C ABI ``mk_disturbance_work_stride`` > 0): specialised
        kernels and N + K <= 64 -- ``adjoint_kernel`` for N + K <= 16, ``adjoint_wide_kernel`` above, in their disturbance mode."""
        return self._reader_stride("disturbances") > 0

    def _disturbance_shapes(self, B):
        return self._reader_shapes(B, bt=dict(r=self.n, ninfo=self.n))

    def alloc_disturbances(self, B):
        """Buffers of ``disturbances`` for B instances (the forward pass's workspace + the two outputs), for callers that run
        it repeatedly (pass them back as ``buffers=``)."""
        return self._reader_buffers("disturbances", None, self._disturbance_shapes(B))

    def disturbances(self, phi, q, x0=None, P0=None, buffers=None):
        """Smoothed STATE DISTURBANCES for B instances (C ABI ``mk_disturbances``): the Durbin-Koopman backward pair of the
        state equation x_t = phi o x_{t-1} + eta_t, ``r[b,t,i]`` and ``ninfo[b,t,i]`` = N_t,ii, for every state of every step
        (t = 0: between the initial state and the first prediction), from which
        ``E[eta | Y] = q r``, ``Var[eta | Y] = q - q^2 ninfo`` and the auxiliary residual ``u = r / sqrt(ninfo)`` (Harvey &
        Koopman 1992; unit spread under the model, large where the state equation failed).  The raw pair is returned so that
        ``u`` is never formed from a difference.  Two launches: the recording forward pass and one backward walk.
        Returns a dict with ``r, ninfo`` ``[B,T,n]`` and ``status`` (the filter's MK_FLAG_* bits)."""
        stride = self._reader_stride("disturbances", refuse=True)
        prob, keep, B = self._problem(phi, q, 0, x0, P0)
        res = self._reader_buffers("disturbances", buffers, self._disturbance_shapes(B), stride)
        return self._reader_call("mk_disturbances", prob, res, self._p(res["r"]), self._p(res["ninfo"]))

    # ------------------------------------------------------------------ one-step-ahead innovations
    _INNOVATION_OUTPUTS = ("v", "f", "pred_mean", "pred_var")

    @property
    def innovations_supported(self):
        """True when ``innovations`` serves this engine's shape (C ABI ``mk_innovations_work_stride`` > 0): N + K <= 64,
        specialised or size-generic kernels alike."""
        return self._reader_stride("innovations") > 0

    def _innovations_shapes(self, B, outputs):
        return self._reader_shapes(B, bt={key: self.N for key in outputs})

    def alloc_innovations(self, B, outputs=_INNOVATION_OUTPUTS):
        """Buffers of ``innovations`` for B instances (the forward pass's workspace + the outputs asked for), for callers that
        run it repeatedly (pass them back as ``buffers=``)."""
        return self._reader_buffers("innovations", None, self._innovations_shapes(B, outputs))

    def innovations(self, phi, q, x0=None, P0=None, buffers=None, outputs=_INNOVATION_OUTPUTS):
        """ONE-STEP-AHEAD innovations for B instances (C ABI ``mk_innovations``): ``v[b,t,j]`` and ``f[b,t,j]`` are the innovation
        and its variance of the scalar update of the observed cell (t, j) -- the cell predicted from the past and from the series
        < j of the same step, so they depend on the order of the series; ``e = v / sqrt(f)`` is independent N(0,1) under the
        model -- NaN where a cell is not observed; ``pred_mean[b,t,j]`` / ``pred_var[b,t,j]`` are the forecast of EVERY series from
        the past alone (which does not depend on the order), in the units of ``set_scaling`` and with the observation variance
        included.  ``outputs``: which of the four to compute.  Returns a dict with those ``[B,T,N]`` tensors and ``status`` (the
        filter's MK_FLAG_* bits); the rows of an instance whose status carries ``FLAG_NONPOSITIVE_F`` are NaN."""
        outputs = tuple(outputs)
        if not outputs or any(k not in self._INNOVATION_OUTPUTS for k in outputs):
            raise ValueError("outputs must be a non-empty subset of %s" % (self._INNOVATION_OUTPUTS,))
        stride = self._reader_stride("innovations", refuse=True)
        prob, keep, B = self._problem(phi, q, 0, x0, P0)
        res = self._reader_buffers("innovations", buffers, self._innovations_shapes(B, outputs), stride)
        ptr = [self._p(res[k]) if k in outputs else None for k in self._INNOVATION_OUTPUTS]
        return self._reader_call("mk_innovations", prob, res, *ptr, mask=outputs)

    def innovation_stats(self, v, f, nlags=10, t_first=0):
        """Whiteness statistics of the standardised innovations ``e = v / sqrt(f)`` per (instance, series) (C ABI
        ``mk_innovation_stats``): over the cells with finite ``v``, finite ``f > 0`` and ``t >= t_first``, in time order, the
        count ``m``, the mean, the variance ``c_0`` (divisor m), the autocorrelations ``r_1 .. r_nlags`` at lags counted in
        successive VALID cells (not calendar steps) and the Ljung-Box statistic ``Q = m (m + 2) sum r_l^2 / (m - l)``.  ``v``,
        ``f``: ``[B,T,N]`` tensors in the engine's layout (as ``innovations`` returns them).  Returns ``[B,N,4+nlags]`` =
        ``[m, mean, c_0, Q, r_1 .. r_nlags]``; ``r_l`` and ``Q`` are NaN when ``m <= nlags`` or ``c_0 = 0``."""
        torch = _torch()
        nlags, t_first = int(nlags), int(t_first)
        if not 1 <= nlags <= 32:
            raise ValueError("nlags must be in 1..32")
        if t_first < 0:
            raise ValueError("t_first must be >= 0")
        if v.ndim != 3 or tuple(v.shape) != tuple(f.shape):
            raise ValueError("v and f must be [B,T,N] tensors of one shape")
        for name, t in (("v", v), ("f", f)):
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.device == self.device and self._layout(t) is t):
                raise ValueError("%s must be a float64 tensor on %s in the engine's layout" % (name, self.device))
        B, T, N = (int(s) for s in v.shape)
        stats = torch.empty((B, N, 4 + nlags), dtype=torch.float64, device=self.device)
        self._bind_stream()
        check(self._L.mk_innovation_stats(self._ctx, B, T, N, 1 if self.time_major else 0, t_first, nlags, self._p(v), self._p(f),
                                          self._p(stats)))
        return stats

    def _residual_cells(self, v, f, t_first):
        """The checks ``innovation_stats`` makes of ``v``, ``f`` and ``t_first`` -> ``(B, T, N, t_first)``."""
        torch = _torch()
        t_first = int(t_first)
        if t_first < 0:
            raise ValueError("t_first must be >= 0")
        if v.ndim != 3 or tuple(v.shape) != tuple(f.shape):
            raise ValueError("v and f must be [B,T,N] tensors of one shape")
        for name, t in (("v", v), ("f", f)):
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.device == self.device and self._layout(t) is t):
                raise ValueError("%s must be a float64 tensor on %s in the engine's layout" % (name, self.device))
        B, T, N = (int(s) for s in v.shape)
        return B, T, N, t_first

    def residual_series(self, v, f, t_first=0):
        """Moments, variance thirds and CUSUM excursions of the standardised innovations ``e = v / sqrt(f)`` per (instance,
        series) (C ABI ``mk_residual_series``).  Over the valid cells (finite ``v``, finite ``f > 0``, ``t >= t_first``)
        ``e_1 .. e_m`` in time order, with ``d_i = e_i - mean``: returns ``[B,N,12]`` = ``[m, mean, S2, S3, S4, h, ss_first,
        ss_last, cusum, cusum_t, cusq, cusq_t]`` -- ``S_k = sum d_i^k`` (not divided); ``h = (m + 1) // 3`` and the sums of
        ``e^2`` over the first and the last ``h`` valid cells; ``cusum = max_k |sum_{i<=k} d_i|`` and ``cusq = max_k
        |sum_{i<=k} d_i^2 - (k / m) S2|``, each with the calendar step of the first ``k`` that attains it.  ``m = 0``: NaN but for
        ``m = h = 0``.  ``v``, ``f``: ``[B,T,N]`` tensors in the engine's layout (as ``innovations`` returns them)."""
        torch = _torch()
        B, T, N, t_first = self._residual_cells(v, f, t_first)
        stats = torch.empty((B, N, 12), dtype=torch.float64, device=self.device)
        self._bind_stream()
        check(self._L.mk_residual_series(self._ctx, B, T, N, 1 if self.time_major else 0, t_first, self._p(v), self._p(f), self._p(stats)))
        return stats

    def residual_cross(self, v, f, stats, nlags=10, t_first=0):
        """Lagged sums of products BETWEEN the series of an instance (C ABI ``mk_residual_cross``): with ``e~ = d / sqrt(S2 / m)``
        from ``stats`` (``residual_series`` of the same ``v``, ``f``, ``t_first``), for the lags ``l = 0 .. nlags`` in CALENDAR
        steps and all ordered pairs, ``counts[b,l,i,j]`` = the number of steps t at which (t, i) and (t - l, j) are both valid
        (int64) and ``sums[b,l,i,j] = sum e~[t,i] e~[t-l,j]`` over them, both ``[B,nlags+1,N,N]``; a pair with a series that has no
        valid cell or does not vary gets 0 and NaN.  ``N <= 64``, ``0 <= nlags <= 32``.  Returns ``(counts, sums)``."""
        torch = _torch()
        nlags = int(nlags)
        if not 0 <= nlags <= 32:
            raise ValueError("nlags must be in 0..32")
        B, T, N, t_first = self._residual_cells(v, f, t_first)
        if N > 64:
            raise ValueError("residual_cross serves N <= 64 series")
        if not (isinstance(stats, torch.Tensor) and stats.dtype == torch.float64 and stats.device == self.device
                and tuple(stats.shape) == (B, N, 12) and stats.is_contiguous()):
            raise ValueError("stats must be the contiguous float64 [B,N,12] tensor of residual_series on %s" % (self.device,))
        counts = torch.empty((B, nlags + 1, N, N), dtype=torch.int64, device=self.device)
        sums = torch.empty((B, nlags + 1, N, N), dtype=torch.float64, device=self.device)
        self._bind_stream()
        check(self._L.mk_residual_cross(self._ctx, B, T, N, 1 if self.time_major else 0, t_first, nlags, self._p(v), self._p(f),
                                        self._p(stats), self._p(counts), self._p(sums)))
        return counts, sums

    # ------------------------------------------------------------------ multi-step-ahead forecasts and forecast skill
    _FORECAST_OUTPUTS = ("fan", "track", "skill")

    @property
    def forecast_supported(self):
        """True when ``forecast`` serves this engine's shape (C ABI ``mk_forecast_work_stride`` > 0): N + K <= 64,
        specialised or size-generic kernels alike."""
        return self._reader_stride("forecast") > 0

    def _forecast_shapes(self, B, horizon, outputs):
        plain = {}
        if "fan" in outputs:
            plain["fan_mean"] = plain["fan_var"] = (B, horizon, self.N)
        if "skill" in outputs:
            plain["skill"] = (B, self.N, horizon, 6)
        return self._reader_shapes(B, bt=dict(track_mean=self.N, track_var=self.N) if "track" in outputs else None, **plain)

    def _forecast_request(self, horizon, outputs):
        outputs = tuple(outputs)
        if not outputs or any(k not in self._FORECAST_OUTPUTS for k in outputs):
            raise ValueError("outputs must be a non-empty subset of %s" % (self._FORECAST_OUTPUTS,))
        horizon = int(horizon)
        if not 1 <= horizon <= int(self._L.mk_forecast_max_horizon()):
            raise ValueError("horizon must be in 1..%d" % int(self._L.mk_forecast_max_horizon()))
        return horizon, outputs

    def alloc_forecast(self, B, horizon=14, outputs=("fan", "skill")):
        """Buffers of ``forecast`` for B instances (the forward pass's workspace + the outputs asked for), for callers that run
        it repeatedly (pass them back as ``buffers=``)."""
        horizon, outputs = self._forecast_request(horizon, outputs)
        return self._reader_buffers("forecast", None, self._forecast_shapes(B, horizon, outputs))

    def forecast(self, phi, q, x0=None, P0=None, horizon=14, outputs=("fan", "skill"), origins=None, track_horizon=1, t_first=1,
                 coverage=0.95, buffers=None):
        """MULTI-STEP-AHEAD forecasts and forecast skill for B instances (C ABI ``mk_forecast``).  From an ORIGIN o -- the
        filtered moments of step o, or the initial moments for o = -1 -- the filter's prediction applied h times gives the
        forecast of every series h steps ahead, mean and variance (observation variance included).  ``outputs``:

        ``"fan"``    ``fan_mean, fan_var [B,horizon,N]``: h = 1 .. horizon from the origin of the instance's record, ``origins``
                     (``[R]`` integers in -1 .. T-1; None = T - 1, the out-of-sample forecast), in the units of ``set_scaling``;
        ``"track"``  ``track_mean, track_var [B,T,N]``: at every step t the forecast made ``track_horizon`` steps earlier (from the
                     initial moments where t < track_horizon), in the units of ``set_scaling``; ``track_horizon=1`` is
                     ``innovations``' ``pred_mean / pred_var``;
        ``"skill"``  ``skill [B,N,horizon,6]``: per series and horizon h, over the pairs (o, t = o + h) with ``t_first <= o``, t < T
                     and y[t] observed, ``[count, sum e, sum e^2, sum e^2/s, sum log s, hits]`` of e = y - mean, s = variance, in the
                     filter's units; hits counts e^2 <= z^2 s with z the two-sided normal quantile of ``coverage``.

        Returns a dict with those tensors and ``status`` (the filter's MK_FLAG_* bits); the rows of an instance whose status
        carries ``FLAG_NONPOSITIVE_F`` are NaN.  Every sum has a fixed order: an instance's rows do not depend on the batch."""
        from scipy.stats import norm

        torch = _torch()
        horizon, outputs = self._forecast_request(horizon, outputs)
        track_horizon, t_first, coverage = int(track_horizon), int(t_first), float(coverage)
        if "track" in outputs and not 1 <= track_horizon <= self.T:
            raise ValueError("track_horizon must be in 1..T = %d" % self.T)
        if t_first < 0:
            raise ValueError("t_first must be >= 0")
        if not 0.0 < coverage < 1.0:
            raise ValueError("coverage must be in (0, 1)")
        stride = self._reader_stride("forecast", refuse=True)
        prob, keep, B = self._problem(phi, q, 0, x0, P0)
        shapes = self._forecast_shapes(B, horizon, outputs)
        res = self._reader_buffers("forecast", buffers, shapes, stride)
        org = None
        if origins is not None and "fan" in outputs:
            org = torch.as_tensor(origins, dtype=torch.int64).reshape(-1).to(self.device).contiguous()
            if org.numel() != self.R:
                raise ValueError("origins must hold one origin per record (%d)" % self.R)
        req = ForecastRequest()
        req.horizon, req.t_first, req.track_horizon = horizon, t_first, track_horizon
        req.coverage_z = float(norm.ppf(0.5 + 0.5 * coverage))
        req.d_fan_origins = None if org is None else org.data_ptr()
        for field, key in (("d_fan_means", "fan_mean"), ("d_fan_vars", "fan_var"), ("d_track_means", "track_mean"),
                           ("d_track_vars", "track_var"), ("d_skill", "skill")):
            setattr(req, field, res[key].data_ptr() if key in shapes else None)
        return self._reader_call("mk_forecast", prob, res, ctypes.byref(req),
                                 mask=[key for key in shapes if key not in ("_work", "status")])

    # ------------------------------------------------------------------ observation weights of smoothed series and states
    @property
    def observation_weights_supported(self):
        """True when ``observation_weights`` serves this engine's shape (C ABI ``mk_weights_work_stride`` > 0): N + K <= 64,
        specialised or size-generic kernels alike."""
        return self._reader_stride("weights") > 0

    def _weights_shapes(self, B, M):
        return self._reader_shapes(B, weights=(B, M, self.T, self.N), intercept=(B, M))

    def alloc_observation_weights(self, B, M):
        """Buffers of ``observation_weights`` for B instances and M targets per record (the forward pass's workspace with the
        gain tape + the two outputs), for callers that run it repeatedly (pass them back as ``buffers=``)."""
        M = int(M)
        if M < 1:
            raise ValueError("M must be >= 1")
        return self._reader_buffers("weights", None, self._weights_shapes(B, M))

    def observation_weights(self, phi, q, targets, what="series", x0=None, P0=None, buffers=None):
        """OBSERVATION WEIGHTS of smoothed series or states for B instances (C ABI ``mk_observation_weights``; Koopman & Harvey
        2003): for fixed parameters the smoother is linear in the data, so the projected smoothed mean at a target is
        ``sum w * y + intercept`` over the observed cells of the record, ``y`` the standardised observations the filter runs on.
        ``targets``: ``[R,M,2]`` integers ``(step, column)`` (or ``[M,2]``, shared by the records) -- column = series j
        (``what="series"``: the unscaled projection ``z_j x_{t|T}``) or state i (``what="states"``); instance b uses the targets of
        record ``b % R``.  Returns a dict with ``weights [B,M,T,N]`` (NaN at every cell that is not observed), ``intercept [B,M]``
        (the part that comes from ``x0``) and ``status`` (the filter's MK_FLAG_* bits); the rows of an instance whose status
        carries ``FLAG_NONPOSITIVE_F`` are NaN.  A target whose step is outside ``[0, T)`` or whose column is out of range has an
        all-NaN row (a negative step marks an unused slot).  Four launches (the recording forward pass, a clear, the gain writer,
        one walk per target); a target's weights do not depend on the batch or on the other targets, bit for bit."""
        torch = _torch()
        if what not in ("series", "states"):
            raise ValueError("what must be 'series' or 'states'")
        stride = self._reader_stride("weights", refuse=True)
        tg = torch.as_tensor(targets, dtype=torch.int64)
        if tg.ndim == 2:
            tg = tg[None].expand(self.R, -1, -1)
        if tg.ndim != 3 or tg.shape[0] != self.R or tg.shape[1] < 1 or tg.shape[2] != 2:
            raise ValueError("targets must be [%d,M,2] (or [M,2]) integers (step, column), M >= 1" % self.R)
        tg = tg.to(self.device).contiguous()
        M = int(tg.shape[1])
        prob, keep, B = self._problem(phi, q, 0, x0, P0)
        res = self._reader_buffers("weights", buffers, self._weights_shapes(B, M), stride)
        req = WeightsRequest()
        req.n_targets, req.what = M, 0 if what == "series" else 1   # MK_DRAW_SERIES / MK_DRAW_STATES
        req.d_targets, req.d_weights, req.d_intercept = tg.data_ptr(), res["weights"].data_ptr(), res["intercept"].data_ptr()
        return self._reader_call("mk_observation_weights", prob, res, ctypes.byref(req), mask=("weights", "intercept"))

    # ------------------------------------------------------------------ intervention effects by GLS
    EFFECT_KINDS = {"level": 0, "ramp": 1}   # MK_EFFECT_LEVEL / MK_EFFECT_RAMP

    @property
    def regression_supported(self):
        """True when ``regression`` serves this engine's shape (C ABI ``mk_regression_work_stride`` > 0): N + K <= 64,
        specialised or size-generic kernels alike."""
        return self._reader_stride("regression") > 0

    def _regression_shapes(self, B, M):
        torch = _torch()
        return self._reader_shapes(B, beta=(B, M), cov=(B, M, M), gain=(B,), normal=(B, M + 1, M + 1),
                                   ints=dict(support=((B, M), torch.int64), dropped=((B,), torch.int32)))

    def _effect_table(self, effects):
        """``[R,M,4]`` int64 on the device from ``[R,M,4]`` or ``[M,4]`` (shared by the records)."""
        torch = _torch()
        ef = torch.as_tensor(effects, dtype=torch.int64)
        if ef.ndim == 2:
            ef = ef[None].expand(self.R, -1, -1)
        mmax = int(self._L.mk_regression_max_effects())
        if ef.ndim != 3 or ef.shape[0] != self.R or not 1 <= ef.shape[1] <= mmax or ef.shape[2] != 4:
            raise ValueError("effects must be [%d,M,4] (or [M,4]) integers (series, kind, t0, t1), 1 <= M <= %d" % (self.R, mmax))
        return ef.to(self.device).contiguous()

    def alloc_regression(self, B, M):
        """Buffers of ``regression`` for B instances and M effects per record (the forward pass's workspace with the gain tape +
        the outputs), for callers that run it repeatedly (pass them back as ``buffers=``)."""
        M = int(M)
        if not 1 <= M <= int(self._L.mk_regression_max_effects()):
            raise ValueError("M must be in 1..%d" % int(self._L.mk_regression_max_effects()))
        return self._reader_buffers("regression", None, self._regression_shapes(B, M))

    def regression(self, phi, q, effects, t_first=1, x0=None, P0=None, buffers=None):
        """INTERVENTION EFFECTS by GLS for B instances (C ABI ``mk_regression``; de Jong's augmented filter): level shifts,
        outliers and trends of single series as known regressors of the observation equation, ``y_t = X_t beta + Z x_t + e_t``,
        estimated for fixed parameters.  ``effects``: ``[R,M,4]`` integers ``(series, kind, t0, t1)`` (or ``[M,4]``, shared by
        the records), ``0 <= t0 < t1 <= T``; kind 0 (``EFFECT_KINDS["level"]``): x = 1 on ``t0 <= t < t1``; kind 1 (``"ramp"``):
        x = min(t, t1 - 1) - t0 + 1 from t0 on; a negative series marks an unused slot; instance b uses the effects of record
        ``b % R``.  The cells of the steps ``t >= t_first`` are counted.  Returns a dict with ``beta [B,M]`` (in the units of the
        standardised observations the filter runs on), ``cov [B,M,M]`` = Var beta, ``gain [B]`` (the drop of -2 log L at beta),
        ``normal [B,M+1,M+1]`` (the augmented normal matrix A: A[0,0] the filter's sum of sigmas, A[0,1:] = s, A[1:,1:] = S),
        ``support [B,M]`` (counted observed cells with x != 0), ``dropped [B]`` (bit m: effect m has support 0 or is collinear
        with the effects before it; its beta and its row and column of cov are NaN, the others are solved without it) and
        ``status`` (the filter's MK_FLAG_* bits); the rows of an instance whose status carries ``FLAG_NONPOSITIVE_F`` are NaN.
        Four launches (the recording forward pass, a clear, the gain writer, the replay); an instance's outputs do not depend on
        the batch, bit for bit."""
        t_first = int(t_first)
        if t_first < 0:
            raise ValueError("t_first must be >= 0")
        stride = self._reader_stride("regression", refuse=True)
        ef = self._effect_table(effects)
        M = int(ef.shape[1])
        prob, keep, B = self._problem(phi, q, 0, x0, P0)
        res = self._reader_buffers("regression", buffers, self._regression_shapes(B, M), stride)
        req = RegressionRequest()
        req.n_effects, req.t_first, req.d_effects = M, t_first, ef.data_ptr()
        for key in ("beta", "cov", "gain", "normal", "support", "dropped"):
            setattr(req, "d_" + key, res[key].data_ptr())
        return self._reader_call("mk_regression", prob, res, ctypes.byref(req), mask=("beta", "cov", "gain", "normal"))

    # ------------------------------------------------------------------ per-step scores by the tangent filter
    _SCORE_OUTPUTS = ("score", "grad", "count", "opg", "cusum")

    @property
    def scores_supported(self):
        """True when ``scores`` serves this engine (C ABI ``mk_scores_work_stride`` > 0): N + K <= 64, specialised or
        size-generic kernels alike, full-square records."""
        return self._reader_stride("scores") > 0

    def _scores_shapes(self, B):
        n = self.n
        return self._reader_shapes(B, bt=dict(score=n), grad=(B, n), opg=(B, n, n), cusum=(B, n, n),
                                   ints=dict(count=((B,), _torch().int64)))

    def alloc_scores(self, B):
        """Buffers of ``scores`` for B instances (the forward pass's workspace with the gain tape and the innovations + the
        outputs), for callers that run it repeatedly (pass them back as ``buffers=``)."""
        return self._reader_buffers("scores", None, self._scores_shapes(B))

    def scores(self, phi, q, dphi, dq, t_first=1, x0=None, P0=None, buffers=None):
        """PER-STEP SCORES for B instances (C ABI ``mk_scores``; the forward-mode, tangent filter): ``score[b,t,p]`` is the
        derivative of step t's contribution to -2 log L, ``sum_j (log f + v^2 / f)`` over the cells observed at t, with respect to
        parameter p -- one per state, moving ``phi_p`` by ``dphi[b,p]`` and ``q_p`` by ``dq[b,p]`` (the chain rule to the caller's
        parameters stays outside; ``scores_alpha`` is Metran's).  What statsmodels calls ``score_obs``.  A step is counted when
        ``t >= t_first`` and it holds an observation.  Returns a dict with ``score [B,T,n]`` (zero at an empty step; stored for
        t < t_first too), ``grad [B,n]`` (the sum over the counted steps), ``count [B]`` (their number m), ``opg [B,n,n]`` =
        ``sum s_t s_t'`` (an information matrix that is positive semi-definite by construction), ``cusum [B,n,n]`` =
        ``sum S_t S_t'`` with ``S_t = sum_{u <= t} (s_u - grad / m)`` (the tied-down cumulative scores of the Nyblom-Hansen test:
        ``metran_amd.scores.nyblom``) and ``status`` (the filter's MK_FLAG_* bits); the rows of an instance whose status carries
        ``FLAG_NONPOSITIVE_F`` are NaN.  Five launches (the recording forward pass, a clear, the gain writer, the tangent kernel,
        the sums); an instance's outputs do not depend on the batch, bit for bit."""
        t_first = int(t_first)
        if t_first < 0:
            raise ValueError("t_first must be >= 0")
        stride = self._reader_stride("scores", refuse=True)
        prob, keep, B = self._problem(phi, q, 0, x0, P0)
        dphi, dq = self._dev(dphi, (B, self.n), "dphi").contiguous(), self._dev(dq, (B, self.n), "dq").contiguous()
        res = self._reader_buffers("scores", buffers, self._scores_shapes(B), stride)
        req = ScoresRequest()
        req.d_dphi, req.d_dq, req.t_first = dphi.data_ptr(), dq.data_ptr(), t_first
        for key in self._SCORE_OUTPUTS:
            setattr(req, "d_" + key, res[key].data_ptr())
        return self._reader_call("mk_scores", prob, res, ctypes.byref(req), mask=("score", "grad", "opg", "cusum"))

    def scores_alpha(self, alpha, dt=1.0, t_first=1):
        """``scores`` for Metran's parametrisation: ``phi, q`` by ``params_from_alpha`` and the derivatives with respect to alpha,
        ``dphi = phi dt / alpha^2`` and ``dq = -2 phi dphi c`` with c = 1 - communality for a series and 1 for a factor."""
        torch = _torch()
        alpha = self._dev(alpha)
        if alpha.ndim == 1:
            alpha = alpha[None]
        phi, q = self.params_from_alpha(alpha, dt=dt)
        B = int(alpha.shape[0])
        if B % self.R != 0:
            raise ValueError("number of instances B=%d must be a multiple of the number of records R=%d" % (B, self.R))
        c = torch.cat([1.0 - (self.loadings * self.loadings).sum(2), torch.ones((self.R, self.K), dtype=torch.float64, device=self.device)], 1)
        dphi = phi * float(dt) / (alpha * alpha)
        dq = -2.0 * phi * dphi * c.repeat(B // self.R, 1)
        return self.scores(phi, q, dphi, dq, t_first=t_first)

    # ------------------------------------------------------------------ leave-block-out predictions
    _BLOCK_OUTPUTS = ("means", "vars", "summary", "flags")

    @property
    def block_predict_supported(self):
        """True when ``block_predict`` serves this engine (C ABI ``mk_block_work_stride`` > 0): N + K <= 64, specialised or
        size-generic kernels alike, full-square records."""
        return self._reader_stride("blocks") > 0

    @property
    def block_max_cells(self):
        """The largest number of steps of a block (C ABI ``mk_block_max_cells``)."""
        return int(self._L.mk_block_max_cells())

    def _block_shapes(self, B, W, L):
        n = self.n
        return self._reader_shapes(B, means=(B, W, L), vars=(B, W, L), summary=(B, W, 4), _checkpoints=(B, W, n + n * n),
                                   ints=dict(flags=((B, W), _torch().int32)))

    def _block_table(self, blocks):
        """``[R,W,3]`` int64 on the host from ``[R,W,3]`` or ``[W,3]`` (shared by the records), validated."""
        torch = _torch()
        bl = torch.as_tensor(blocks, dtype=torch.int64).cpu()
        if bl.ndim == 2:
            bl = bl[None].expand(self.R, -1, -1)
        if bl.ndim != 3 or bl.shape[0] != self.R or bl.shape[1] < 1 or bl.shape[2] != 3:
            raise ValueError("blocks must be [%d,W,3] (or [W,3]) integers (series, t0, t1), W >= 1" % self.R)
        used = bl[..., 0] >= 0
        if bool((used & (bl[..., 0] >= self.N)).any()):
            raise ValueError("blocks: a series is outside 0 .. N - 1 = %d" % (self.N - 1))
        if bool((used & ~((bl[..., 1] >= 0) & (bl[..., 1] < bl[..., 2]) & (bl[..., 2] <= self.T))).any()):
            raise ValueError("blocks: need 0 <= t0 < t1 <= T = %d" % self.T)
        length = int(((bl[..., 2] - bl[..., 1]) * used).max()) if bool(used.any()) else 1
        if length > self.block_max_cells:
            raise ValueError("blocks: a block of %d steps is longer than the limit of %d" % (length, self.block_max_cells))
        return bl.contiguous(), max(length, 1)

    def alloc_block_predict(self, B, W, L):
        """Buffers of ``block_predict`` for B instances, W blocks per record and rows of L cells (the forward pass's workspace
        with the gain tape and the innovations, the checkpoints + the outputs), for callers that run it repeatedly (pass them
        back as ``buffers=``)."""
        W, L = int(W), int(L)
        if W < 1 or not 1 <= L <= self.block_max_cells:
            raise ValueError("W must be >= 1 and L in 1..%d" % self.block_max_cells)
        return self._reader_buffers("blocks", None, self._block_shapes(B, W, L))

    def block_predict(self, phi, q, blocks, x0=None, P0=None, buffers=None):
        """LEAVE-BLOCK-OUT PREDICTIONS for B instances (C ABI ``mk_block_predict``): for every block ``(series, t0, t1)`` --
        ``blocks`` is ``[R,W,3]`` integers (or ``[W,3]``, shared by the records), ``0 <= t0 < t1 <= T``, at most
        ``block_max_cells`` = 64 steps, a negative series marks an unused slot, instance b uses the blocks of record ``b % R`` --
        the prediction of the block's observed cells from EVERY observation outside the block, with its covariance V: how well a
        gap of that length is filled.  Returns a dict with ``means [B,W,L]`` and ``vars [B,W,L]`` (L = the longest block, or the
        row length of ``buffers``; position c is step t0 + c; the caller's units, ``vars`` without the observation variance, as
        ``loo_predict``; NaN where the cell is not observed or beyond t1), ``summary [B,W,4]`` = (m observed cells, quad =
        e'V^-1 e of the prediction errors e, log det V, 1'V1 / m^2 in the caller's units: the variance of the block's mean),
        ``flags [B,W]`` (bit 0: the block is degenerate -- a pivot of the unit-diagonal precision block below 1e-12; its outputs
        except m are NaN) and ``status`` (the filter's MK_FLAG_* bits); the rows of an instance whose status carries
        ``FLAG_NONPOSITIVE_F`` are NaN.  quad and log det V are in the units of the standardised observations the filter runs on.
        Five launches (the recording forward pass, a clear, the gain writer, the checkpoint walk, the block walk); a block's
        outputs do not depend on the batch or on the other blocks, bit for bit."""
        stride = self._reader_stride("blocks", refuse=True)
        bl, length = self._block_table(blocks)
        W = int(bl.shape[1])
        prob, keep, B = self._problem(phi, q, 0, x0, P0)
        L = int(buffers["means"].shape[2]) if buffers is not None and hasattr(buffers.get("means"), "shape") and buffers["means"].ndim == 3 else length
        if L < length:
            raise ValueError("buffers hold rows of %d cells; a block has %d steps" % (L, length))
        res = self._reader_buffers("blocks", buffers, self._block_shapes(B, W, L), stride)
        bl = bl.to(self.device)
        req = BlockRequest()
        req.n_blocks, req.n_cells, req.d_blocks, req.d_checkpoints = W, L, bl.data_ptr(), res["_checkpoints"].data_ptr()
        for key in self._BLOCK_OUTPUTS:
            setattr(req, "d_" + key, res[key].data_ptr())
        return self._reader_call("mk_block_predict", prob, res, ctypes.byref(req), mask=("means", "vars", "summary"))

    # ------------------------------------------------------------------ level-shift scan
    @property
    def level_shifts_supported(self):
        """True when ``level_shifts`` serves this engine (C ABI ``mk_shift_work_stride`` > 0): N + K <= 64, specialised or
        size-generic kernels alike, full-square records."""
        return self._reader_stride("shifts") > 0

    def _shift_shapes(self, B):
        return self._reader_shapes(B, bt=dict(num=self.N, den=self.N))

    def alloc_level_shifts(self, B):
        """Buffers of ``level_shifts`` for B instances (the forward pass's workspace with the gain tape and the innovations + the
        two outputs), for callers that run it repeatedly (pass them back as ``buffers=``)."""
        return self._reader_buffers("shifts", None, self._shift_shapes(B))

    def level_shifts(self, phi, q, x0=None, P0=None, buffers=None):
        """LEVEL-SHIFT SCAN for B instances (C ABI ``mk_level_shifts``): for every observed cell (t, j) the GLS statistic of a
        permanent offset of series j from step t on -- the regressor x = 1 on the observed cells of series j at the steps >= t --
        for all dates from one backward walk (de Jong & Penzer 1998).  Returns a dict with ``num [B,T,N]`` = A = x'u,
        ``den [B,T,N]`` = D = x'Mx (M the precision of the record's data vector, u = M (y - mu)) and ``status`` (the filter's
        MK_FLAG_* bits): the estimate of the shift is A / D, its standard error 1 / sqrt(D), its t-statistic A / sqrt(D), in the
        standardised units the filter runs on (``set_scaling`` does not enter); what ``regression`` gives for the single level
        effect ``(j, level, t, T)`` as ``beta``, ``cov`` and ``gain`` = A^2 / D.  NaN where a cell is not observed; the rows of an
        instance whose status carries ``FLAG_NONPOSITIVE_F`` are NaN.  Four launches (the recording forward pass, a clear, the
        gain writer, the scan); an instance's outputs do not depend on the batch or the layout, bit for bit."""
        stride = self._reader_stride("shifts", refuse=True)
        prob, keep, B = self._problem(phi, q, 0, x0, P0)
        res = self._reader_buffers("shifts", buffers, self._shift_shapes(B), stride)
        req = ShiftRequest()
        req.d_num, req.d_den = res["num"].data_ptr(), res["den"].data_ptr()
        return self._reader_call("mk_level_shifts", prob, res, ctypes.byref(req), mask=("num", "den"))

    # ------------------------------------------------------------------ exact window means, changes and contrasts
    @property
    def functionals_supported(self):
        """True when ``functionals`` serves this engine (C ABI ``mk_functionals_work_stride`` > 0): N + K <= 64, specialised or
        size-generic kernels alike, full-square records."""
        return self._reader_stride("functionals") > 0

    def _functionals_shapes(self, B, W, C):
        return self._reader_shapes(B, mean=(B, W, C), var=(B, W, C))

    def _functionals_counts(self, W, C):
        W, C, cmax = int(W), int(C), int(self._L.mk_functionals_max_contrasts())
        if W < 1 or not 1 <= C <= cmax:
            raise ValueError("need W >= 1 windows and 1 <= C <= %d contrasts (got W = %d, C = %d)" % (cmax, W, C))
        return W, C

    def alloc_functionals(self, B, W, C):
        """Buffers of ``functionals`` for B instances, W windows and C contrasts per record (the workspace of the filtered and the
        smoothed records + the two outputs), for callers that run it repeatedly (pass them back as ``buffers=``)."""
        W, C = self._functionals_counts(W, C)
        return self._reader_buffers("functionals", None, self._functionals_shapes(B, W, C))

    def functionals(self, phi, q, windows, contrasts=None, x0=None, P0=None, buffers=None):
        """EXACT posterior mean and variance of linear functionals of the smoothed signal for B instances (C ABI
        ``mk_functionals``): ``l = sum_t alpha_t c'(scale o Z x_t + offset)`` with ``alpha_t = 1/(t1 - t0)`` on ``[t0, t1)`` and
        ``-1/(t3 - t2)`` on ``[t2, t3)`` -- the mean over a window (``t2 == t3``), a point value (``t1 - t0 == 1``) or the
        difference of two periods' means -- from the smoother's covariance across time (the smoothed state autocovariance), never
        from draws.  ``windows``: ``[R,W,4]`` integers ``(t0, t1, t2, t3)`` (or ``[W,4]``, shared by the records), clamped to
        ``[0, T]``; ``contrasts``: ``[R,C,N]`` weights of the series (or ``[C,N]``, shared), None = the N unit contrasts; instance
        b uses the windows and contrasts of record ``b % R``.  Units as set by ``set_scaling``; no observation variance is added.
        Returns a dict with ``mean, var [B,W,C]`` and ``status`` (the filter's and the smoothers' MK_FLAG_* bits); a functional whose
        first range is empty is NaN; the rows of an instance whose status carries ``FLAG_NONPOSITIVE_F`` are NaN.  Three launches
        (the recording forward pass, the smoother, one walk per window); an instance's results do not depend on the batch, on the
        other windows or on the other contrasts, bit for bit."""
        torch = _torch()
        stride = self._reader_stride("functionals", refuse=True)
        wn = torch.as_tensor(windows, dtype=torch.int64)
        if wn.ndim == 2:
            wn = wn[None].expand(self.R, -1, -1)
        if wn.ndim != 3 or wn.shape[0] != self.R or wn.shape[1] < 1 or wn.shape[2] != 4:
            raise ValueError("windows must be [%d,W,4] (or [W,4]) integers (t0, t1, t2, t3), W >= 1" % self.R)
        wn = wn.to(self.device).contiguous()
        ct = None
        if contrasts is not None:
            ct = torch.as_tensor(contrasts, dtype=torch.float64)
            if ct.ndim == 2:
                ct = ct[None].expand(self.R, -1, -1)
            if ct.ndim != 3 or ct.shape[0] != self.R or ct.shape[2] != self.N:
                raise ValueError("contrasts must be [%d,C,%d] (or [C,%d]) weights of the series" % (self.R, self.N, self.N))
            ct = ct.to(self.device).contiguous()
        W, C = self._functionals_counts(wn.shape[1], self.N if ct is None else ct.shape[1])
        prob, keep, B = self._problem(phi, q, 0, x0, P0)
        res = self._reader_buffers("functionals", buffers, self._functionals_shapes(B, W, C), stride)
        req = FunctionalRequest()
        req.n_windows, req.n_contrasts = W, C
        req.d_windows, req.d_contrasts = wn.data_ptr(), None if ct is None else ct.data_ptr()
        return self._reader_call("mk_functionals", prob, res, ctypes.byref(req), self._p(res["mean"]), self._p(res["var"]),
                                 mask=("mean", "var"))

    def adjust_observations(self, effects, beta):
        """Subtract fitted intervention effects from the observations (C ABI ``mk_regression_adjust``): ``obs - sum_m beta_m x_m``
        with ``effects [R,M,4]`` as in ``regression`` and ``beta [R,M]`` in the units of the engine's observations (a NaN beta, a
        dropped effect, counts as 0).  Applied to the current observations and, if a mask is active, to the kept unmasked copy
        as well, so that ``unmask_observations`` afterwards gives adjusted, unmasked records.  The originals of both are kept:
        ``unadjust_observations`` restores them (a mask set or lifted in between goes with it), and a second
        ``adjust_observations`` starts again from them."""
        torch = _torch()
        if self.obs is None:
            raise MetranHipError("call set_observations first")
        ef = self._effect_table(effects)
        M = int(ef.shape[1])
        beta = self._dev(beta, (self.R, M), "beta")
        kept = getattr(self, "_obs_unadjusted", None)
        base, base_unmasked = kept if kept is not None else (self.obs, getattr(self, "_obs_unmasked", None))
        self._bind_stream()

        def adjusted(t):
            if t is None:
                return None
            out = torch.empty_like(t)
            check(self._L.mk_regression_adjust(self._ctx, self.R, self.T, self.N, 1 if self.time_major else 0, M, self._p(ef),
                                               self._p(beta), self._p(t), self._p(out)))
            return out

        obs, unmasked = adjusted(base), adjusted(base_unmasked)
        self._obs_unadjusted = (base, base_unmasked)
        self.obs, self._obs_unmasked = obs, unmasked
        self._grad_pending = self._grad_alpha = None  # a pending forward pass belongs to the records before
        check(self._L.mk_observations_changed(self._ctx))
        return self

    @property
    def observations_adjusted(self):
        """True between ``adjust_observations`` and ``unadjust_observations``: the observations carry fitted effects."""
        return getattr(self, "_obs_unadjusted", None) is not None

    def unadjust_observations(self):
        """The observations as they were before ``adjust_observations`` (and the kept unmasked copy, if a mask was active)."""
        kept = getattr(self, "_obs_unadjusted", None)
        if kept is not None:
            self.obs, self._obs_unmasked = kept
            self._obs_unadjusted = None
            self._grad_pending = self._grad_alpha = None
            check(self._L.mk_observations_changed(self._ctx))
        return self

    # ------------------------------------------------------------------ posterior draws (simulation smoother)
    def _draw_perturb(self, prob, B, ndraws, seed, first_instance, first_draw, antithetic, L0, want_zx, want_x):
        """``mk_draw_perturb`` for ``ndraws`` draws of the B instances of ``prob``: ``(ystar, zxplus or None, xplus or None)``,
        logical ``[ndraws*B,T,.]`` in the engine's layout."""
        SB = ndraws * B
        ystar = self._empty_bt(SB, self.T, self.N)
        zx = self._empty_bt(SB, self.T, self.N) if want_zx else None
        xp = self._empty_bt(SB, self.T, self.n) if want_x else None
        self._bind_stream()
        check(self._L.mk_draw_perturb(self._ctx, ctypes.byref(prob), int(seed) & (2 ** 64 - 1), int(first_instance), int(first_draw),
                                      int(ndraws), 1 if antithetic else 0, self._p(L0), self._p(ystar), self._p(zx), self._p(xp)))
        return ystar, zx, xp

    def _adopt_records(self, obs, loadings, obsvar=None, scale=None, offset=None):
        """Take device-resident records and their per-record arrays as they are -- ``obs [R,T,N]`` already in this engine's
        layout with NaN for missing, ``loadings [R,N,K]``, ``obsvar / scale / offset [R,N]`` or None -- with everything
        ``set_observations`` + ``set_loadings`` + ``set_scaling`` guarantee except the copies: shapes checked, kernels for
        (N, K) ensured, anything that belonged to the previous records (unmasked copy, pending forward pass, the context's
        cached observed-step list) dropped."""
        torch = _torch()
        for name, t in (("obs", obs), ("loadings", loadings), ("obsvar", obsvar), ("scale", scale), ("offset", offset)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.device == self.device):
                raise ValueError("%s must be a float64 tensor on %s" % (name, self.device))
        if obs.ndim != 3 or self._layout(obs) is not obs:
            raise ValueError("obs must be [R,T,N] in the engine's layout")
        R, T, N = (int(v) for v in obs.shape)
        if loadings.ndim != 3 or tuple(loadings.shape[:2]) != (R, N) or not loadings.is_contiguous():
            raise ValueError("loadings must be a contiguous [R=%d,N=%d,K] tensor, got %s" % (R, N, tuple(loadings.shape)))
        for name, t in (("obsvar", obsvar), ("scale", scale), ("offset", offset)):
            if t is not None and (tuple(t.shape) != (R, N) or not t.is_contiguous()):
                raise ValueError("%s must be a contiguous [%d,%d] tensor" % (name, R, N))
        shape_before = (self.N, getattr(self, "K", None))
        self.obs, self.R, self.T, self.N = obs, R, T, N
        self.loadings, self.K = loadings, int(loadings.shape[2])
        self.obsvar, self.scale, self.offset = obsvar, scale, offset
        self._obs_unmasked = self._obs_unadjusted = None
        self._grad_pending = self._grad_alpha = None
        if (self.N, self.K) != shape_before:
            self._ensure_kernels()
        check(self._L.mk_observations_changed(self._ctx))
        return self

    def _draw_sub_engine(self, B):
        """The engine that smooths the perturbed records: same device, layout, kernels and projection path as this one (the
        wide filter's batch-size rule "auto" pinned to what it picks for this engine's B instances, so that a draw does not
        depend on how many draws share its launch)."""
        sub = getattr(self, "_draw_kf", None)
        if sub is None or sub._ctx is None:
            sub = self._draw_kf = BatchedKalman(self.device.index, layout="time_major" if self.time_major else "model_major",
                                                packed_sym=False)
        sub.projection_path = self.projection_path
        for which in self._VARIANTS:
            sub.set_variant(which, self.get_variant(which))
        if self.get_variant("wide_filter") == "auto":
            sub.set_variant("wide_filter", self.resolved_wide_filter(B))
        return sub

    def _draw_bytes_per_draw(self, B, what):
        """Device bytes one draw of B instances needs next to the result: y*, the unconditional part, and the smoothing pass's
        record array / tape and moments."""
        N, n = self.N, self.n
        if what == "series":
            stride = int(self._L.mk_tape_stride(N, self.K)) if self.tape_path() else self.record_stride()
            per_step = 2 * N + stride + 2 * N
        else:
            stride = int(self._L.mk_state_tape_stride(N, self.K)) if self.state_tape_path() else self.record_stride()
            per_step = N + n + stride + 2 * n
        return 8.0 * B * self.T * per_step

    def draw_smoothed(self, phi, q, ndraws, seed=0, what="series", x0=None, P0=None, antithetic=False, first_draw=0,
                      first_instance=0, chunk=None):
        """Joint posterior DRAWS given the data -- the simulation smoother by mean correction (Durbin & Koopman 2002): for every
        draw one unconditional simulation of the model (``mk_draw_perturb``: counter-based normals, so draw ``s`` of instance
        ``i`` is the same numbers whatever launch computes it), one smoothing pass of the perturbed record through the route
        ``simulate_smoothed`` (``what="series"``) or ``smooth_state_variances`` (``"states"``) takes for this engine, and the
        sum of the two (``mk_draw_combine``).  Series draws are in the units of ``set_scaling``; at an observed cell without
        observation variance a series draw is the observation.  ``antithetic``: draws 2k and 2k + 1 mirror each other around
        the smoothed mean.  Draws run in chunks sized by the free device memory (``chunk=`` forces a size); the result does not
        depend on the chunk size.  ``first_draw`` / ``first_instance`` number this call's draws / instances within a larger
        ensemble.  Returns ``{"draws": [S,B,T,N] or [S,B,T,n], "status": [S,B]}``; a path whose parameters are invalid (its
        simulated record is not finite at an observed cell) carries ``FLAG_NONPOSITIVE_F`` and NaN draws."""
        torch = _torch()
        S = self._draw_check(ndraws, what, "draw_smoothed")
        prob, keep, B = self._problem(phi, q, 1, x0, P0)
        W = self.N if what == "series" else self.n
        draws = torch.empty((S, B, self.T, W), dtype=torch.float64, device=self.device)
        status = torch.empty((S, B), dtype=torch.int32, device=self.device)

        def keep_chunk(s0, c, out, lost, flags):
            draws[s0:s0 + c] = out.masked_fill(lost[:, None, None], float("nan")).unflatten(0, (c, B))
            status[s0:s0 + c] = flags.view(c, B)

        self._draw_chunks(prob, keep, B, S, what, seed, antithetic, first_draw, first_instance, chunk, keep_chunk)
        return {"draws": draws, "status": status}

    def _draw_check(self, ndraws, what, who):
        if what not in ("series", "states"):
            raise ValueError("what must be 'series' or 'states'")
        S = int(ndraws)
        if S < 1:
            raise ValueError("ndraws must be >= 1")
        if self.packed_sym:
            raise MetranHipError("%s needs a full-square engine (packed_sym=False)" % who)
        return S

    def _draw_chunks(self, prob, keep, B, S, what, seed, antithetic, first_draw, first_instance, chunk, sink):
        """The chunk loop of the simulation smoother, shared by ``draw_smoothed`` and ``draw_window_statistics``: calls
        ``sink(s0, c, out, lost, flags)`` per chunk of ``c`` draws starting at draw ``s0`` -- ``out`` the combined draws, logical
        ``[c*B,T,W]`` in the engine's layout, which is the smoothing workspace (the sink reads it and keeps no reference),
        ``lost [c*B]`` the flagged paths (``out`` is NOT masked for them) and ``flags [c*B]`` their status words.  The caller
        allocates its results BEFORE the call: the chunk size comes from the memory that is free then."""
        torch = _torch()
        phi_, q_, x0_, P0_ = keep
        L0 = torch.linalg.cholesky(P0_).contiguous() if P0_ is not None else None
        series = what == "series"
        ws = getattr(self, "_draw_ws", None)
        if chunk is None:
            per = self._draw_bytes_per_draw(B, what)
            have = ws["bytes"] if ws is not None and ws["key"][:2] == (what, B) and ws["key"][3:6] == (self.T, self.N, self.K) else 0.0
            room = max(have, 0.8 * float(torch.cuda.mem_get_info(self.device)[0]))
            chunk = int(min(S, room // per))
            if chunk < 1:
                raise MemoryError("one draw of %d instances needs %.1f GB (T=%d, N=%d, K=%d); %.1f GB are free -- draw fewer "
                                  "instances at a time" % (B, per / 1e9, self.T, self.N, self.K, room / 0.8 / 1e9))
        chunk = max(1, min(int(chunk), S))
        sub = self._draw_sub_engine(B)
        rec = torch.arange(B, device=self.device) % self.R
        rep = lambda a, c, *ones: None if a is None else a.repeat(c, *ones)  # noqa: E731
        seen = torch.isfinite(self.obs)[rec]             # [B,T,N]: the observed cells of every instance's record
        res = out = None
        for s0 in range(0, S, chunk):
            c = min(chunk, S - s0)
            ystar, zx, xp = self._draw_perturb(prob, B, c, seed, first_instance, first_draw + s0, antithetic, L0, series, not series)
            # an OBSERVED cell whose y* is not finite: the path's parameters are invalid (a NaN persistence, a negative or NaN q or
            # observation variance: mk_draw_perturb).  The smoothing pass would take the cell for a missing one and never meet them,
            # so the path is flagged here (MK_FLAG_NONPOSITIVE_F, the filter's error bit) and its draws are NaN
            lost = (seen.repeat(c, 1, 1) & ~torch.isfinite(ystar)).flatten(1).any(1)
            # the derived problem: one record per path, this engine's CURRENT loadings / variances / scaling replicated over the draws
            sub._adopt_records(ystar, rep(self.loadings[rec], c, 1, 1), rep(None if self.obsvar is None else self.obsvar[rec], c, 1),
                               rep(None if self.scale is None else self.scale[rec], c, 1),
                               rep(None if self.offset is None else self.offset[rec], c, 1))
            # the workspace is kept between chunks (and calls) of one size AND one smoothing route
            route = (sub.tape_path() if series else sub.state_tape_path(), sub.get_variant("kernel_family"))
            key = (what, B, c, self.T, self.N, self.K) + route
            if ws is None or ws["key"] != key:
                res = out = ws = self._draw_ws = None   # the old workspace goes before the new one comes (a tail chunk, another route)
                buffers = sub.alloc_projection(c * B) if series else sub.alloc_state_variances(c * B)
                ws = self._draw_ws = {"key": key, "buffers": buffers, "bytes": c * self._draw_bytes_per_draw(B, what)}
                del buffers
            ws["buffers"]["status"].zero_()
            kw = dict(x0=rep(x0_, c, 1), P0=rep(P0_, c, 1, 1), buffers=ws["buffers"])
            res = (sub.simulate_smoothed if series else sub.smooth_state_variances)(rep(phi_, c, 1), rep(q_, c, 1), **kw)
            out = res["sim_means"] if series else res["S"]
            self._bind_stream()
            check(self._L.mk_draw_combine(self._ctx, ctypes.byref(prob), c, 0 if series else 1, 1 if self.time_major else 0,
                                          self._p(zx if series else xp), self._p(out)))
            sink(s0, c, out, lost, res["status"] | lost.to(torch.int32) * FLAG_NONPOSITIVE_F)
            sub.obs = None   # y* of this chunk is done with

    def _step_windows(self, windows):
        """``windows`` as the int64 ``[R,W,2]`` device tensor of ``mk_path_functionals``, its precondition checked here."""
        torch = _torch()
        w = windows.cpu().numpy() if isinstance(windows, torch.Tensor) else np.asarray(windows)
        if w.ndim == 2:
            w = np.broadcast_to(w, (self.R,) + w.shape)
        if w.ndim != 3 or w.shape[0] != self.R or w.shape[1] < 1 or w.shape[2] != 2 or not np.issubdtype(w.dtype, np.integer):
            raise ValueError("windows must be integer step ranges [R=%d,W>=1,2] (or [W,2] for all records)" % self.R)
        w = np.ascontiguousarray(w, dtype=np.int64)
        a, b = w[:, :, 0], w[:, :, 1]
        if (a < 0).any() or (b > self.T).any() or (a > b).any():
            raise ValueError("every window [a, b) needs 0 <= a <= b <= T = %d" % self.T)
        if (b[:, :-1] > a[:, 1:]).any():
            raise ValueError("the windows of a record must be sorted and must not overlap (b_w <= a_{w+1})")
        return torch.from_numpy(w).to(self.device)

    def draw_window_statistics(self, phi, q, ndraws, windows, thresholds=None, probs=(0.025, 0.5, 0.975), seed=0, what="series",
                               x0=None, P0=None, antithetic=False, first_draw=0, first_instance=0, chunk=None,
                               return_functionals=False):
        """WINDOW STATISTICS of the posterior draws of ``draw_smoothed`` (same arguments, same draws), reduced on the device
        inside its chunk loop: the ensemble ``[S,B,T,W]`` is never allocated.  ``windows`` int ``[R,W,2]`` (or ``[W,2]`` for all
        records): half-open step ranges ``[a, b)`` per record, sorted and not overlapping, ``0 <= a <= b <= T`` (``ValueError``
        otherwise); empty windows are allowed.  Per path, column and window ``mk_path_functionals`` takes the five functionals
        mean, min, max, fraction of steps below ``thresholds [R,Wd]`` (the path's units; None or NaN: functionals 3, 4 are NaN)
        and longest spell below it; over the draws of every cell one ``mk_ensemble_summary`` then takes count, mean, sd, min,
        max and the quantiles ``probs`` (at most 16) of the finite values.  Returns ``{"summary": [B,Wd,W,5,5+P], "status":
        [S,B]}`` and, with ``return_functionals``, ``"functionals": [S,B,Wd,W,5]``.  A flagged path (see ``draw_smoothed``) is NaN
        in the functionals and therefore outside the summary's counts.  ``ndraws`` is at most ``mk_ensemble_max_draws()``."""
        torch = _torch()
        S = self._draw_check(ndraws, what, "draw_window_statistics")
        cap, NF = int(self._L.mk_ensemble_max_draws()), int(self._L.mk_path_functional_count())
        if S > cap:
            raise ValueError("ndraws = %d is above the %d draws the ensemble summary serves" % (S, cap))
        probs = np.ascontiguousarray(np.asarray(probs, dtype=np.float64).reshape(-1))
        if probs.size > 16 or not ((probs >= 0.0) & (probs <= 1.0)).all():
            raise ValueError("probs must be at most 16 probabilities in [0, 1]")
        win = self._step_windows(windows)
        prob, keep, B = self._problem(phi, q, 1, x0, P0)
        Wd, W = (self.N if what == "series" else self.n), int(win.shape[1])
        thr = self._dev(thresholds, (self.R, Wd), "thresholds") if thresholds is not None else None
        functionals = torch.empty((S, B, Wd, W, NF), dtype=torch.float64, device=self.device)
        summary = torch.empty((B, Wd, W, NF, 5 + probs.size), dtype=torch.float64, device=self.device)
        status = torch.empty((S, B), dtype=torch.int32, device=self.device)

        def reduce_chunk(s0, c, out, lost, flags):
            part = functionals[s0:s0 + c]
            self._bind_stream()
            check(self._L.mk_path_functionals(self._ctx, ctypes.byref(prob), c, 0 if what == "series" else 1, 1 if self.time_major else 0,
                                              self._p(out), W, self._p(win), self._p(thr), self._p(part)))
            part.view(c * B, -1).masked_fill_(lost[:, None], float("nan"))
            status[s0:s0 + c] = flags.view(c, B)

        self._draw_chunks(prob, keep, B, S, what, seed, antithetic, first_draw, first_instance, chunk, reduce_chunk)
        self._bind_stream()
        check(self._L.mk_ensemble_summary(self._ctx, S, B * Wd * W * NF, self._p(functionals), probs.size,
                                          probs.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), self._p(summary)))
        res = {"summary": summary, "status": status}
        if return_functionals:
            res["functionals"] = functionals
        return res

    def simulate_unconditional(self, phi, q, ndraws, seed=0, P0=None, antithetic=False, first_draw=0, first_instance=0):
        """Unconditional simulations of the model (the first half of ``draw_smoothed``, same kernel, same normals): ``xplus
        [S,B,T,n]`` state paths started from N(0, P0), ``zxplus [S,B,T,N]`` their projections ``[I | loadings] x+`` (unscaled)
        and ``yplus [S,B,T,N]`` the simulated records (with observation noise where observation variances are set)."""
        torch = _torch()
        S = int(ndraws)
        if S < 1:
            raise ValueError("ndraws must be >= 1")
        held = self.obs
        try:   # against an all-zero record the perturbed record is -y+ at every cell
            self.obs = self._layout(torch.zeros((self.R, self.T, self.N), dtype=torch.float64, device=self.device))
            prob, keep, B = self._problem(phi, q, 1, None, P0)
            L0 = torch.linalg.cholesky(keep[3]).contiguous() if keep[3] is not None else None
            ystar, zx, xp = self._draw_perturb(prob, B, S, seed, first_instance, first_draw, antithetic, L0, True, True)
        finally:
            self.obs = held
        return {"xplus": xp.unflatten(0, (S, B)), "zxplus": zx.unflatten(0, (S, B)), "yplus": (-ystar).unflatten(0, (S, B))}

    def state_tape_path(self):
        """True when ``smooth_state_variances`` runs over the STATE tape (``MK_OUT_TAPE | MK_OUT_VAR_ONLY``: the tape of
        ``tape_path`` plus K factor entries per step; ``mk_dk.hip`` STATE = true): the shapes of ``tape_path`` with zero
        observation variances (Metran's, metran.py:382-384)."""
        return self.tape_path() and self.obsvar is None

    def alloc_state_variances(self, B, projection=False):
        """Buffers of ``smooth_state_variances`` for B instances (pass them back as ``buffers=``).  ``projection``: on the
        state-tape path the same backward pass can write the projected moments ``sim_means / sim_vars [B,T,N]`` as well."""
        torch = _torch()
        res = {"mle": torch.empty(B, dtype=torch.float64, device=self.device),
               "status": torch.zeros(B, dtype=torch.int32, device=self.device),
               "sigmacount": torch.empty(B, dtype=torch.int64, device=self.device), "_rs": self.record_stride(),
               "_var_only": True}
        if self.state_tape_path():
            res["_rs"] = int(self._L.mk_state_tape_stride(self.N, self.K))
            res["_tape"] = True
            res["F"] = res["_rec_filt"] = self._empty_bt(B, self.T, res["_rs"])  # d_F = the state tape
            if projection:
                res["sim_means"] = self._empty_bt(B, self.T, self.N)
                res["sim_vars"] = self._empty_bt(B, self.T, self.N)
        else:
            if projection:
                raise MetranHipError("projection=True needs the state-tape path (state_tape_path())")
            res["_rec_filt"], res["F"], res["Pf"], res["sigmas"], res["detfs"] = self._alloc_records(B)
        res["S"] = self._empty_bt(B, self.T, self.n)
        res["var"] = self._empty_bt(B, self.T, self.n)
        return res

    def smooth_state_variances(self, phi, q, warmup=1, x0=None, P0=None, buffers=None):
        """``Metran.get_state_means`` / ``get_state_variances`` (metran.py:655-711, method="smoother") for B instances
        without materialising the smoothed covariances (``MK_OUT_VAR_ONLY``): smoothed state means ``S [B,T,n]`` and
        variances ``var [B,T,n]``.  n <= 16 and the shapes without a tape: the filter writes the filtered records, the
        RTS smoother reads them.  Wide models on the tape path (``state_tape_path``): the filter writes the STATE tape and
        the inverse-free backward pass turns it into the same moments -- no filtered record, no LDL^T chain."""
        prob, keep, B = self._problem(phi, q, warmup, x0, P0)
        res = buffers if buffers is not None else self.alloc_state_variances(B)
        o = self._outputs_struct(dict(res, Ps=res["var"]))
        self._bind_stream()
        check(self._L.mk_filter_smooth(self._ctx, ctypes.byref(prob), ctypes.byref(o)))
        return res

    def supported_shapes(self):
        """(N, K) pairs with kernels compiled into the library."""
        shapes = (ctypes.c_int64 * 256)()
        cnt = self._L.mk_supported_shapes(shapes, 128)
        return [(int(shapes[2 * i]), int(shapes[2 * i + 1])) for i in range(min(cnt, 128))]

    def smooth(self, phi, q, F, Pf, outputs=("S", "Ps")):
        """``kalmansmoother`` (kalmanfilter.py:403-476) from existing filtered moments
        ``F [B,T,n]``, ``Pf [B,T,n,n]``; needs no observations (the kernel depends on n only)."""
        F = self._layout(self._dev(F) if not isinstance(F, _torch().Tensor) else F.to(self.device))
        Pf = self._layout(self._dev(Pf) if not isinstance(Pf, _torch().Tensor) else Pf.to(self.device))
        B, T, n = (int(s) for s in F.shape)
        if tuple(Pf.shape) != (B, T, n, n):
            raise ValueError("Pf must be [B,T,n,n]")
        phi = self._dev(phi, (B, n), "phi")
        q = self._dev(q, (B, n), "q")
        shape = [(N, K) for (N, K) in self.supported_shapes() if N + K == n]
        if not shape and n >= 2 and self._L.mk_shape_supported(n - 1, 1):
            shape = [(n - 1, 1)]  # no specialised kernel of this state dimension: the size-generic smoother (it depends on n only)
        if not shape:
            raise MetranHipError("no HIP smoother kernel for state dimension n=%d" % n)
        N, K = shape[0]
        prob = Problem(B, 1, T, N, K, 1, None, self._p(phi), self._p(q), None, None, None, None, 0, None, None)
        torch = _torch()
        res = {"F": F, "Pf": Pf, "status": torch.zeros(B, dtype=torch.int32, device=self.device)}
        if "S" in outputs:
            res["S"] = self._empty_bt(B, T, n)
        if "Ps" in outputs:
            res["Ps"] = self._empty_bt(B, T, n, n)
        o = self._outputs_struct(res)
        self._bind_stream()
        check(self._L.mk_smooth(self._ctx, ctypes.byref(prob), ctypes.byref(o)))
        return res

    def smooth_dense(self, phi, F, Pf, Xp, Pp):
        """``kalmansmoother`` in its literal 5-argument form (kalmanfilter.py:403-476) for B models: the predicted moments
        ``Xp [B,T,n]``, ``Pp [B,T,n,n]`` are READ as handed in (:454-474), not recomputed from the filtered ones -- for
        moments that did not come out of this engine's own filter.  ``mk_smooth_dense`` (size-generic kernel, n <= 128).
        Returns a dict with ``S [B,T,n]``, ``Ps [B,T,n,n]``, ``status [B]``."""
        torch = _torch()
        F, Pf, Xp, Pp = (self._dev(a) for a in (F, Pf, Xp, Pp))
        B, T, n = (int(s) for s in F.shape)
        if tuple(Pf.shape) != (B, T, n, n) or tuple(Xp.shape) != (B, T, n) or tuple(Pp.shape) != (B, T, n, n):
            raise ValueError("F, Xp must be [B,T,n] and Pf, Pp [B,T,n,n]")
        phi = self._dev(phi, (B, n), "phi")
        res = {"S": torch.empty((B, T, n), dtype=torch.float64, device=self.device),
               "Ps": torch.empty((B, T, n, n), dtype=torch.float64, device=self.device),
               "status": torch.zeros(B, dtype=torch.int32, device=self.device)}
        self._bind_stream()
        check(self._L.mk_smooth_dense(self._ctx, B, T, n, self._p(phi), self._p(F), self._p(Pf), self._p(Xp), self._p(Pp),
                                      self._p(res["S"]), self._p(res["Ps"]), self._p(res["status"])))
        return res

    # ------------------------------------------------------------------ projection epilogues
    def simulate(self, Z, means, covs):
        """``SPKalmanFilter.simulate`` (kalmanfilter.py:569-603): Z ``[RZ,N,n]`` or ``[N,n]``."""
        torch = _torch()
        Z = self._dev(Z)
        if Z.ndim == 2:
            Z = Z[None]
        means = self._dev(means)
        covs = self._dev(covs)
        B, T, n = (int(s) for s in means.shape)
        RZ, N = int(Z.shape[0]), int(Z.shape[1])
        sm = torch.empty((B, T, N), dtype=torch.float64, device=self.device)
        sv = torch.empty((B, T, N), dtype=torch.float64, device=self.device)
        self._bind_stream()
        check(self._L.mk_simulate(self._ctx, B, RZ, T, N, n, self._p(Z), self._p(means), self._p(covs), self._p(sm),
                                  self._p(sv)))
        return sm, sv

    def decompose(self, Z, means):
        """``SPKalmanFilter.decompose`` (kalmanfilter.py:605-644) -> (sdf [B,T,N], cdf [B,K,T,N])."""
        torch = _torch()
        Z = self._dev(Z)
        if Z.ndim == 2:
            Z = Z[None]
        means = self._dev(means)
        B, T, n = (int(s) for s in means.shape)
        RZ, N = int(Z.shape[0]), int(Z.shape[1])
        sdf = torch.empty((B, T, N), dtype=torch.float64, device=self.device)
        cdf = torch.empty((B, n - N, T, N), dtype=torch.float64, device=self.device)
        self._bind_stream()
        check(self._L.mk_decompose(self._ctx, B, RZ, T, N, n, self._p(Z), self._p(means), self._p(sdf), self._p(cdf)))
        return sdf, cdf

    def sum(self, values):
        """Deterministic device sum (fixed order) of a 1-D tensor -> 0-d tensor."""
        torch = _torch()
        values = self._dev(values).reshape(-1)
        out = torch.empty(1, dtype=torch.float64, device=self.device)
        self._bind_stream()
        check(self._L.mk_sum(self._ctx, int(values.numel()), self._p(values), self._p(out)))
        return out[0]

    # ------------------------------------------------------------------ the one collective (C ABI mk_allreduce_sum)
    @staticmethod
    def comm_unique_id():
        """128 bytes identifying a new RCCL communicator (``mk_comm_unique_id`` = ``ncclGetUniqueId``): ONE rank calls it
        and hands the bytes to the others (``distributed.attach_communicator`` does that over the process group's store)."""
        buf = ctypes.create_string_buffer(128)
        check(_lib.lib().mk_comm_unique_id(buf))
        return buf.raw

    def init_communicator(self, nranks, rank, unique_id):
        """``mk_comm_init_rank``: join the RCCL communicator ``unique_id`` as ``rank`` of ``nranks`` on this engine's device
        (collective: every rank calls it).  The context owns the communicator until ``close()``."""
        if len(unique_id) != 128:
            raise ValueError("unique_id must be the 128 bytes of comm_unique_id()")
        check(self._L.mk_comm_init_rank(self._ctx, int(nranks), int(rank), ctypes.c_char_p(bytes(unique_id))))
        self._has_comm = True
        return self

    def set_communicator(self, nccl_comm):
        """``mk_set_communicator``: use a caller-owned ``ncclComm_t`` (an integer address / ``c_void_p``); None detaches."""
        check(self._L.mk_set_communicator(self._ctx, ctypes.c_void_p(nccl_comm) if nccl_comm else None))
        self._has_comm = bool(nccl_comm)
        return self

    def has_communicator(self):
        return bool(getattr(self, "_has_comm", False))

    def allreduce_sum(self, t):
        """In-place all-reduce(sum) of a float64 device tensor over the engine's communicator (``mk_allreduce_sum``, on the
        current stream).  Raises without a communicator: there is no single-rank shortcut."""
        torch = _torch()
        if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous():
            raise ValueError("allreduce_sum takes a contiguous float64 tensor on the engine's device")
        self._bind_stream()
        check(self._L.mk_allreduce_sum(self._ctx, self._p(t), int(t.numel())))
        return t

    # ------------------------------------------------------------------ lock-step L-BFGS (calibrate_batch; mk_lbfgs.hip)
    def lbfgs_direction(self, x, g, lo, active, Sh, Yh, rho, hlen, hpos, gtol, pg, d, phase=None, step=None, nback=None):
        """Projected gradient into ``pg``, ``active &= max|pg| > gtol``, the two-loop recursion over every model's own history
        ring (``hlen`` live pairs from slot ``hpos``) with its safeguards into ``d``.  With ``phase / step / nback`` (own line
        search per model) a model in the middle of its search keeps direction and step, the others start a new one.  Returns the
        number of active models."""
        R, n = (int(v) for v in x.shape)
        cnt = ctypes.c_int(0)
        self._bind_stream()
        check(self._L.mk_lbfgs_direction(self._ctx, R, n, int(Sh.shape[0]), self._p(x), self._p(g), self._p(lo), self._p(active), self._p(Sh),
                                         self._p(Yh), self._p(rho), self._p(hlen), self._p(hpos), float(gtol), self._p(pg), self._p(d),
                                         self._p(phase), self._p(step), self._p(nback), ctypes.byref(cnt)))
        return int(cnt.value)

    def lbfgs_trial(self, x, d, step, lo, searching, x_new, xt, xe):
        """``xt = max(x + step d, lo)``; ``xe = xt`` for the searching models, their accepted point for the settled ones."""
        R, n = (int(v) for v in x.shape)
        self._bind_stream()
        check(self._L.mk_lbfgs_trial(self._ctx, R, n, self._p(x), self._p(d), self._p(step), self._p(lo), self._p(searching), self._p(x_new),
                                     self._p(xt), self._p(xe)))

    def lbfgs_armijo(self, ft, f, pg, xt, x, searching, step, x_new, f_new, nback=None, max_backtracks=0, accepted=None):
        """Armijo test of the searching models at their trial points (in place: ``x_new, f_new, searching, step``).  Lock-step form:
        returns the number of models still searching.  Own-line-search form (``nback``, ``accepted`` given): an accepted model is
        marked in ``accepted`` and stays in ``searching`` (the active mask), a model out of trial points leaves it; returns
        ``(still searching, accepted)``."""
        R, n = (int(v) for v in x.shape)
        ns, na = ctypes.c_int(0), ctypes.c_int(0)
        self._bind_stream()
        own = nback is not None
        check(self._L.mk_lbfgs_armijo(self._ctx, R, n, self._p(ft), self._p(f), self._p(pg), self._p(xt), self._p(x), self._p(searching),
                                      self._p(step), self._p(x_new), self._p(f_new), self._p(nback), int(max_backtracks), self._p(accepted),
                                      ctypes.byref(ns), ctypes.byref(na) if own else None))
        return (int(ns.value), int(na.value)) if own else int(ns.value)

    def lbfgs_update(self, x, f, g, x_new, f_new, g_new, keep_old, searching, active, ftol, Sh, Yh, rho, hlen, hpos, mask=None, phase=None,
                     nit=None, maxiter=0):
        """For the models of ``mask`` (None: all): the pair of the accepted point into the model's ring if it is usable,
        ``(x, f, g) <- (x_new, f_new, g_new)`` (lock-step form: models still searching keep their old gradient if ``keep_old`` and
        leave ``active``), ``active &= relative reduction > ftol``.  ``nit [R]`` int32: every active model updated here has taken one
        more quasi-Newton iteration; at ``maxiter`` (> 0) it leaves ``active``.  Returns the number of usable pairs."""
        R, n = (int(v) for v in x.shape)
        cnt = ctypes.c_int(0)
        self._bind_stream()
        check(self._L.mk_lbfgs_update(self._ctx, R, n, int(Sh.shape[0]), self._p(x), self._p(f), self._p(g), self._p(x_new), self._p(f_new),
                                      self._p(g_new), 1 if keep_old else 0, self._p(searching), self._p(mask), self._p(active), float(ftol),
                                      self._p(Sh), self._p(Yh), self._p(rho), self._p(hlen), self._p(hpos), self._p(phase), self._p(nit),
                                      int(maxiter), ctypes.byref(cnt)))
        return int(cnt.value)

    # ------------------------------------------------------------------ instrumentation
    def enable_timing(self, enable=True, accumulate=False):
        """hipEvents around every hot-kernel launch.  ``accumulate``: every launch keeps its own event pair until
        ``kernel_ms_totals`` collects them (no host synchronisation inside a timed loop); otherwise only the most
        recent launch of each kind is kept (``last_kernel_ms``)."""
        self._timing = bool(enable)
        check(self._L.mk_enable_timing(self._ctx, (2 if accumulate else 1) if enable else 0))

    def kernel_ms_totals(self):
        """(filter_ms, filter_launches, smoother_ms, smoother_launches) since the previous call (accumulate mode)."""
        f, s = ctypes.c_double(0.0), ctypes.c_double(0.0)
        nf, ns = ctypes.c_int64(0), ctypes.c_int64(0)
        check(self._L.mk_kernel_ms_totals(self._ctx, ctypes.byref(f), ctypes.byref(nf), ctypes.byref(s), ctypes.byref(ns)))
        return float(f.value), int(nf.value), float(s.value), int(ns.value)

    def last_kernel_ms(self):
        """(filter_ms, smoother_ms) of the most recent launches, measured with hipEvents on the launch stream."""
        f, s = ctypes.c_float(-1.0), ctypes.c_float(-1.0)
        check(self._L.mk_last_kernel_ms(self._ctx, ctypes.byref(f), ctypes.byref(s)))
        return float(f.value), float(s.value)

    def synchronize(self):
        check(self._L.mk_sync(self._ctx))

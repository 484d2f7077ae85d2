"""Many Metran models at once: everything a user of ``metran.Metran`` calls after construction (``get_factors``,
``solve``, ``get_mle``, ``get_simulated_means/variances``, ``get_simulation``, ``decompose_simulation``,
``get_state_means/variances``, ``get_state``, ``mask_observations``; metran/metran.py:199-226,
464-506, 605-989, 991-1045) on top of the batched engine.  The orchestration is Python, as in the reference; every
number comes from the HIP kernels:

    ingest.ObservationBatch  ->  mk_standardize             (Metran.__init__: combine, daily grid, standardise)
    FactorAnalysisBatch      ->  mk_fa_*                     (Metran.get_factors for all models)
    calibrate_batch          ->  mk_loglik_grad / mk_loglik  (Metran.solve for all models in lock-step)
    simulate_smoothed        ->  filter + projecting smoother (get_simulated_means / _variances)
    loo_predict              ->  leave-one-out predictions of every observation (get_loo_simulation, get_deletion_residuals)
    smooth_state_variances   ->  state means / variances / decomposition
    disturbances             ->  smoothed state disturbances and auxiliary residuals (get_auxiliary_residuals, screen_breaks)
    forecast                 ->  multi-step-ahead forecasts and forecast skill by horizon (get_forecast, get_prediction_at,
                                 forecast_skill)
    observation_weights      ->  which observations a smoothed value comes from (get_observation_weights, get_state_weights,
                                 get_weight_shares)
    block_predict            ->  leave-block-out predictions: how well a gap of a given length is filled (get_gap_predictions,
                                 gap_fill_skill)
    regression               ->  intervention effects by GLS: level shifts, outliers and trends of single series
                                 (fit_interventions, adjust_observations)
    scores_alpha             ->  per-step scores of the parameters by the tangent filter: OPG and robust standard errors,
                                 the Nyblom-Hansen test of parameter constancy (get_scores, get_parameter_covariance,
                                 test_parameter_stability)
    functionals              ->  exact window means, changes between periods and contrasts of series, from the smoother's
                                 covariance across time (get_window_means, get_window_mean, get_changes)
    level_shifts             ->  the t-statistic of a level shift of every series from every date, from one backward pass
                                 (get_level_shift_statistics, get_level_shift, screen_level_shifts, detect_level_shifts)
    draw_smoothed            ->  posterior draws of series and states (get_simulation_draws, get_state_draws)
    draw_window_statistics   ->  window statistics of the draws, reduced on the device (get_window_statistics)

Results are cached like ``Metran._run_kalman`` does (metran.py:963-989), by one method (``MetranBatch._run``) over one
table (``_KINDS``): ``_cache[kind] = (parameter set, {request: kept result})``.  Every kind holds the results of ONE
parameter set -- different kinds may hold different ones -- and of that result only the keys its accessors read (the table's
keep-list: never the forward pass's workspace, the records or the tape, which are hundreds of times the outputs), plus what
the accessors derive from them once (``("simf", standardized)``, ``("decomp", standardized)``).  The kinds with a request
(``forecast``, ``weights``, ``regress``, ``functionals``, ``blocks``, ``scores``, ``hessian``; ``shifts`` has none) keep every request of their parameter set; another parameter set drops them all.  ``solve``,
``mask_observations``, ``unmask_observations``, ``adjust_observations`` and ``unadjust_observations`` clear the cache.  So asking for another series, the variances after the
means, or the decomposition after the simulation does not launch anything.  The draws and their window statistics are not
cached: an ensemble is the size of the thing it summarises.

With ``torch.distributed`` initialised and ``shard=True`` each rank ingests and owns a contiguous slice of the models
(``distributed.shard_range``); no collective is needed (per-model parameters) and ``gather`` concatenates per-model results
in rank order.
"""
import numpy as np

from .calibrate import calibrate_batch
from .engine import BatchedKalman
from .ingest import ObservationBatch
from .kalmanfilter import check_status

__all__ = ["MetranBatch"]


def _forecast(mb, phi, q, request):
    """request = (outputs, horizon, track horizon, first origin, coverage); the fan from every model's last real step
    (``lengths[r] - 1``: shorter records are padded with empty steps)."""
    outputs, horizon, track_horizon, t_first, coverage = request
    return mb.kf.forecast(phi, q, horizon=horizon, outputs=outputs, origins=np.asarray(mb.batch.lengths, dtype=np.int64) - 1,
                          track_horizon=track_horizon, t_first=t_first, coverage=coverage)


def _weights(mb, phi, q, request):
    """request = (model, column, steps, what), run on a sub-engine that holds that model alone (``BatchedKalman.subset``: the
    walks cost one pass over a record per target, the other models' records are not touched)."""
    r, column, steps, what = request
    targets = np.stack([np.asarray(steps, dtype=np.int64), np.full(len(steps), column, dtype=np.int64)], axis=1)
    return mb.kf.subset([r]).observation_weights(phi[r:r + 1], q[r:r + 1], targets, what=what)


def _regress(mb, phi, q, request):
    """request = (effect table as nested tuples [R][M][4], t_first); beside the regression the objective it is the drop of:
    -2 log L of the records as they are, counted from the same step."""
    effects, t_first = request
    out = mb.kf.regression(phi, q, np.asarray(effects, dtype=np.int64).reshape(mb.R, -1, 4), t_first=t_first)
    return dict(out, obj=mb.kf.loglik(phi, q, warmup=t_first))


def _functionals(mb, phi, q, request):
    """request = (windows as nested tuples [R][W][4], contrasts as nested tuples [R][C][N] or None, standardized): the call sets
    the scaling it is asked for itself (standardised units: none) and leaves the facade's behind."""
    windows, contrasts, standardized = request
    mb.kf.set_scaling(None, None) if standardized else mb.kf.set_scaling(mb._std, mb._mean)
    try:
        return mb.kf.functionals(phi, q, np.asarray(windows, dtype=np.int64).reshape(mb.R, -1, 4),
                                 None if contrasts is None else np.asarray(contrasts, dtype=np.float64).reshape(mb.R, -1, mb.N))
    finally:
        mb.kf.set_scaling(mb._std, mb._mean)


def _blocks(mb, phi, q, request):
    """request = the block table as nested tuples [R][W][3]; original units (the facade's scaling is set)."""
    return mb.kf.block_predict(phi, q, np.asarray(request, dtype=np.int64).reshape(mb.R, -1, 3))


def _shifts(mb, phi, q, request):
    """No request: the scan of every (series, date) of every model, in the standardised units the filter runs on."""
    return mb.kf.level_shifts(phi, q)


def _blocks_that_fit(kf, W, L, budget=None):
    """How many instances one ``block_predict`` call can take so that its workspace, checkpoints and outputs stay within
    ``budget`` bytes (None: 0.8 of the free device memory, as ``calibrate._grad_sets_that_fit`` has it).  Raises when not one fits."""
    import torch

    n = kf.N + kf.K
    per_instance = 8.0 * (W * (n + n * n + 2 * L + 4.5) + kf.T * kf._reader_stride("blocks", refuse=True))
    if budget is None:
        dev = kf.device
        budget = 0.8 * float(torch.cuda.mem_get_info(dev)[0]) if getattr(dev, "type", "cpu") == "cuda" else float("inf")
    fit = int(min(kf.R, budget // per_instance))
    if fit < 1:
        raise MemoryError("leave-block-out predictions of %d blocks per model need %.3g bytes per model; the budget is %.3g" % (
            W, per_instance, budget))
    return fit


def _scores(mb, alpha, request):
    """request = t_first.  The derivatives are Metran's, with respect to alpha: the engine forms them from the parameter set itself."""
    return mb.kf.scores_alpha(alpha, dt=mb.dt, t_first=request)


def _hessian(mb, alpha, request):
    """request = t_first: the Hessian of -2 log L with respect to alpha, differenced from the adjoint gradient as
    ``calibrate_batch(stderr=True)`` does, over the steps the scores count.  The filter's warm-up skips steps that HOLD an
    observation, so a record's warm-up is the number of its non-empty steps before t_first; the records are taken in groups
    of equal warm-up (one group, the whole engine, unless records begin with empty steps)."""
    import torch

    from .scores import hessian_alpha

    kf = mb.kf
    warm = torch.isfinite(kf.obs[:, :request]).any(2).sum(1).cpu().numpy() if request > 0 else np.zeros(mb.R, dtype=np.int64)
    hess = torch.empty((mb.R, mb.N + mb.K, mb.N + mb.K), dtype=torch.float64, device=alpha.device)
    for w in np.unique(warm):
        idx = np.nonzero(warm == w)[0]
        whole = idx.size == mb.R
        part = hessian_alpha(kf if whole else kf.subset(idx), alpha if whole else alpha[torch.as_tensor(idx, device=alpha.device)],
                             dt=mb.dt, warmup=int(w))
        hess[torch.as_tensor(idx, device=hess.device)] = part
    return {"hessian": hess, "status": torch.zeros(mb.R, dtype=torch.int32, device=hess.device)}


# kind -> (engine call (facade, phi, q, request), whether the scaling is set first, keys of the result that are kept).
# The scaling is set where the call writes ORIGINAL units: the projection, the leave-one-out predictions, the one- and
# multi-step-ahead forecasts.  "q" is the q the run was computed for.
_KINDS = {
    "project": (lambda mb, phi, q, _: mb.kf.simulate_smoothed(phi, q), True, ("sim_means", "sim_vars")),
    # state means + variances only (MK_OUT_VAR_ONLY): the smoothed covariances [R,T,n,n] are never written (wide models: the
    # state tape, BatchedKalman.state_tape_path)
    "smoother": (lambda mb, phi, q, _: mb.kf.smooth_state_variances(phi, q), False, ("S", "var")),
    "filter": (lambda mb, phi, q, _: mb.kf.filter(phi, q, outputs=("F", "Pf")), False, ("F", "Pf")),
    "loo": (lambda mb, phi, q, _: mb.kf.loo_predict(phi, q), True, ("loo_means", "loo_vars")),
    # v / f in standardised units, pred_mean / pred_var in original units
    "innov": (lambda mb, phi, q, _: mb.kf.innovations(phi, q), True, ("v", "f", "pred_mean", "pred_var")),
    "dist": (lambda mb, phi, q, _: mb.kf.disturbances(phi, q), False, ("r", "ninfo", "q")),
    "forecast": (_forecast, True, ("fan_mean", "fan_var", "track_mean", "track_var", "skill")),
    "weights": (_weights, False, ("weights", "intercept")),
}
# The kinds that ESTIMATE something from the records instead of reading the filter's or the smoother's output: the same three
# columns, the same cache and the same way through ``MetranBatch._run``; a table of their own because ``_KINDS`` is the list of
# the views of one smoothing pass that tests/test_batch_facade_host.py states.  Standardised units: the facade scales the estimates.
_FIT_KINDS = {
    "regress": (_regress, False, ("beta", "cov", "gain", "normal", "support", "dropped", "obj")),
    # exact moments of linear functionals of the smoothed signal, in the units the request names
    "functionals": (_functionals, False, ("mean", "var")),
    # leave-block-out predictions of the requested gaps, original units
    "blocks": (_blocks, True, ("means", "vars", "summary", "flags")),
    # the level-shift scan: A = x'u and D = x'Mx of a shift of every series from every date, standardised units
    "shifts": (_shifts, False, ("num", "den")),
}
# The kinds whose engine call takes the parameter set itself, alpha, not (phi, q): kind -> (engine call (facade, alpha, request),
# keys of the result that are kept).  The same cache and the same status check, through ``MetranBatch._run``.
_ALPHA_KINDS = {
    # per-step scores with respect to alpha and their sums; the Hessian that the "hessian" and "robust" covariances need
    "scores": (_scores, ("score", "grad", "count", "opg", "cusum")),
    "hessian": (_hessian, ("hessian",)),
}


class MetranBatch:
    """R independent dynamic-factor models with N series and K common factors each.

    Parameters
    ----------
    models : sequence of whatever ``Metran(oseries)`` accepts (one entry per model)
    factors : array ``[R,N,K]`` or ``[N,K]`` (shared), optional
        factor loadings ``Metran.factors``.  Default None: batched factor analysis of every model
        (``FactorAnalysisBatch``, the reference's ``get_factors``); models with fewer factors than the batch maximum
        K get zero columns (a common factor nobody loads on: it changes no likelihood and no projection).
    maxfactors : as ``FactorAnalysis(maxfactors)``
    shard : bool   with torch.distributed initialised, keep only this rank's slice of ``models``
    device, tmin, tmax, min_pairs : as in ``BatchedKalman`` / ``Metran.settings``
    """

    def __init__(self, models, factors=None, device=None, tmin=None, tmax=None, min_pairs=20, dt=1.0, maxfactors=None,
                 shard=False):
        models = list(models)
        total = len(models)
        span = (0, total)
        if shard:
            from .distributed import shard_range, world

            rank, size = world()
            span = shard_range(total, rank, size)
            models = models[span[0]:span[1]]
            if factors is not None and np.ndim(factors) == 3:
                factors = np.asarray(factors)[span[0]:span[1]]
        batch = ObservationBatch(models, tmin=tmin, tmax=tmax, min_pairs=min_pairs)
        kf = BatchedKalman(device, layout="time_major")
        batch.upload(kf)  # standardised records + (std, mean) scaling on the device
        eigval = fep = nfactors = None
        if factors is None:
            from .factoranalysis import FactorAnalysisBatch

            fa = FactorAnalysisBatch(maxfactors=maxfactors, engine=kf).solve()
            nfactors = fa.nfactors.cpu().numpy()
            if (nfactors == 0).any():
                bad = np.nonzero(nfactors == 0)[0]
                # the reference cannot solve such a model either (metran.py:1022-1023: factors is None)
                raise Exception("No proper common factors could be derived from series of model(s) %s"
                                % ", ".join(str(int(b) + span[0]) for b in bad))
            factors = fa.factors.cpu().numpy()
            eigval = fa.eigval.cpu().numpy()
            fep = fa.fep.cpu().numpy()
        factors = np.asarray(factors, dtype=np.float64)
        if factors.ndim == 2:
            factors = np.broadcast_to(factors, (batch.shape[0],) + factors.shape).copy()
        kf.set_loadings(factors)
        self._assemble(batch, kf, kf.scale, kf.offset, factors, nfactors, dt, span, total, eigval, fep)

    def _assemble(self, batch, kf, std, mean, factors, nfactors=None, dt=1.0, shard=None, n_models_total=None, eigval=None, fep=None):
        """Every attribute of the facade from its parts -- the ingested batch, the engine that holds its standardised records and
        the loadings ``factors [R,N,K]``, the series' ``std`` / ``mean`` ``[R,N]`` on the engine's device; ``shard`` the span of
        this rank's models among all ``n_models_total`` (default: all of them) -- what ``__init__`` ends with, and what builds a
        facade over a stand-in engine where there is no GPU (tests/batch_standin.py)."""
        self.batch, self.kf = batch, kf
        self.R, self.T, self.N = batch.shape
        self.K = int(factors.shape[2])
        self.factors = factors
        self.nfactors = np.full(self.R, self.K, dtype=np.int64) if nfactors is None else nfactors
        self.eigval, self.fep = eigval, fep
        self.dt = float(dt)
        self.shard = (0, self.R) if shard is None else shard
        self.n_models_total = self.R if n_models_total is None else n_models_total
        self._std, self._mean = std, mean
        self.alpha = None
        self.fit = None
        self._cache = {}
        return self

    # ------------------------------------------------------------------ parameters / objective
    def _alpha(self, alpha):
        if alpha is None:
            if self.alpha is None:
                raise ValueError("no parameters: call solve() first or pass alpha [R,N+K]")
            return self.alpha
        return self.kf._dev(alpha, (self.R, self.N + self.K), "alpha")

    def _params(self, alpha, scaling=False):
        """``(phi, q)`` of the parameter set (None: the default one); ``scaling``: the engine's next call writes original units."""
        phi, q = self.kf.params_from_alpha(self._alpha(alpha), dt=self.dt)
        if scaling:
            self.kf.set_scaling(self._std, self._mean)
        return phi, q

    def _launch(self, what, alpha, scaling, call):
        """The way to the engine: the parameters, the scaling, ``call(phi, q)`` and the check of its status bits (``what`` names
        the run in the refusal) -> ``(result, q)``."""
        phi, q = self._params(alpha, scaling)
        out = call(phi, q)
        check_status(out["status"].reshape(-1), "MetranBatch(%s)" % what)
        return out, q

    def get_mle(self, alpha=None):
        """``Metran.get_mle`` (metran.py:605-622) for every model: -2 log L ``[R]``."""
        return self.kf.loglik(*self._params(alpha))

    def solve(self, **kwargs):
        """``Metran.solve`` (metran.py:991-1045) for all models in lock-step (``calibrate_batch``);
        the optimum becomes the default parameter set of the accessors.  Returns the CalibrationResult.
        Keyword arguments go to ``calibrate_batch``; ``fd_below=4096`` (2048 for models of more than 16 states) lets the last
        stragglers finish on differenced gradients -- what the reference's own solver uses throughout -- and is what
        ``bench.py``'s calibration lines are measured with."""
        kwargs.setdefault("dt", self.dt)
        self.fit = calibrate_batch(self.kf, **kwargs)
        self.alpha = self.fit.alpha
        if (self.nfactors < self.K).any():
            # models with fewer factors than the batch maximum carry zero loading columns: their surplus cdf states are
            # decoupled dummies (alpha stays at its start value, zero gradient).  The reference counts N + nfactors[r]
            # parameters (solver.py:280: aic = 2 P + fun) and has no such rows in its parameter table.
            import torch

            nf = torch.as_tensor(self.nfactors, device=self.fit.obj.device)
            self.fit["aic"] = 2.0 * (self.N + nf).to(self.fit.obj.dtype) + self.fit.obj
            dummy = torch.arange(self.N + self.K, device=nf.device)[None, :] >= (self.N + nf)[:, None]
            self.fit["dummy_parameters"] = dummy          # [R, N+K] True where a parameter does not exist for the model
            if "stderr" in self.fit:
                self.fit["stderr"] = torch.where(dummy, torch.full_like(self.fit["stderr"], float("nan")), self.fit["stderr"])
        self._cache.clear()
        return self.fit

    def gather(self, t):
        """Per-model result ``[R_local, ...]`` of this rank -> ``[R_total, ...]`` on every rank, rank order."""
        from .distributed import gather_concat

        tail = tuple(t.shape[1:])
        return gather_concat(t.reshape(-1)).reshape((-1,) + tail)

    # ------------------------------------------------------------------ observations
    def mask_observations(self, mask):
        """``Metran.mask_observations`` (metran.py:464-494) for the batch: ``mask [R,T,N]`` non-zero = hide."""
        self.kf.mask_observations(mask)
        self._cache.clear()

    def unmask_observations(self):
        """``Metran.unmask_observations`` (metran.py:496-506)."""
        self.kf.unmask_observations()
        self._cache.clear()

    # ------------------------------------------------------------------ cached kernel runs (Metran._run_kalman)
    def _run(self, kind, alpha, request=None):
        """The result of ``_KINDS[kind]`` (or ``_FIT_KINDS[kind]``, ``_ALPHA_KINDS[kind]``) for the parameter set and the (hashable) ``request``: from the cache, or from the engine
        and then kept -- the keys of the kind's keep-list, nothing else.  A kind holds the results of one parameter set
        (metran.py:978-989 keeps one too); another parameter set replaces them once its own run has passed the status check."""
        import torch

        a = self._alpha(alpha)
        hit = self._cache.get(kind)
        if hit is None or hit[0].shape != a.shape or not bool(torch.equal(hit[0], a)):
            hit = (a.clone(), {})
        if request not in hit[1]:
            if kind in _ALPHA_KINDS:
                call, keep = _ALPHA_KINDS[kind]
                out = call(self, a, request)
                check_status(out["status"].reshape(-1), "MetranBatch(%s)" % kind)
            else:
                call, scaling, keep = _KINDS[kind] if kind in _KINDS else _FIT_KINDS[kind]
                out, q = self._launch(kind, a, scaling, lambda phi, q: call(self, phi, q, request))
                out = dict(out, q=q)
            hit[1][request] = {key: value for key, value in out.items() if key in keep}
            self._cache[kind] = hit
        return hit[1][request]

    def _method(self, method):
        if method not in ("smoother", "filter"):
            raise ValueError("method must be 'smoother' or 'filter'")
        return method

    def _observation_matrix(self, standardized):
        """``get_observation_matrix`` / ``get_scaled_observation_matrix`` (metran.py:365-370, 944-961) ``[R,N,n]``."""
        import torch

        Z = torch.zeros((self.R, self.N, self.N + self.K), dtype=torch.float64, device=self.kf.device)
        Z[:, :, : self.N] = torch.eye(self.N, dtype=torch.float64, device=self.kf.device)
        Z[:, :, self.N:] = self.kf.loadings
        return Z if standardized else Z * self._std[:, :, None]

    # ------------------------------------------------------------------ what the accessors share
    def _series(self, r, name):
        names = list(self.batch.names[r])
        if name not in names:
            raise KeyError("Unknown name: " + str(name))  # the reference logs this and returns None (metran.py:881)
        return names.index(name)

    def _check_state(self, i):
        if i < 0 or i >= self.N + self.K:
            raise IndexError("Value of i must be >=0 and <%d" % (self.N + self.K))  # the reference logs and returns None

    def _units(self, means, variances, standardized):
        """``means`` and ``variances`` (or None) ``[..., R, steps, N]`` in ORIGINAL units, as they are or in standardised units."""
        if not standardized:
            return means, variances
        std, mean = self._std[:, None, :], self._mean[:, None, :]
        return (means - mean) / std, None if variances is None else variances / (std * std)

    @staticmethod
    def _band(mean, variance, ci):
        from pandas import concat
        from scipy.stats import norm

        if ci is None:
            return mean
        if not (0 < ci < 1):
            raise Exception("The value of alpha must be between 0 and 1.")  # metran.py:741-744, 868-871
        iv = norm.ppf(1 - ci / 2.0) * np.sqrt(variance)
        out = concat([mean, mean - iv, mean + iv], axis=1)
        out.columns = ["mean", "lower", "upper"]
        return out

    def _series_band(self, r, j, means, variances, ci):
        """Series ``j`` of model ``r`` of ``means`` / ``variances [R,T,N]``, cut to the model's length, on its index: ``_band``."""
        L = int(self.batch.lengths[r])
        sim = self.batch.frame(r, means[r].cpu().numpy()).iloc[:L, j]
        return self._band(sim, self.batch.frame(r, variances[r].cpu().numpy()).iloc[:L, j] if ci is not None else None, ci)

    def _rows(self, labels, names):
        """Row labels ``(model, ...)``: ``labels(r)`` yields the rest of the rows of model ``r``, named ``names``; a model is
        numbered by its place among ALL models (the shard's offset)."""
        from pandas import MultiIndex

        return MultiIndex.from_tuples([(r + self.shard[0],) + tuple(rest) for r in range(self.R) for rest in labels(r)],
                                      names=["model"] + list(names))

    # ------------------------------------------------------------------ simulation (projection of the states)
    def _simulate(self, alpha, standardized, method):
        if self._method(method) == "smoother":
            out = self._run("project", alpha)  # fused epilogue, original units
            return self._units(out["sim_means"], out["sim_vars"], standardized)
        out = self._run("filter", alpha)
        key = ("simf", bool(standardized))
        if key not in out:
            m, v = self.kf.simulate(self._observation_matrix(standardized), out["F"], out["Pf"])
            out[key] = (m if standardized else m + self._mean[:, None, :], v)
        return out[key]

    def get_simulated_means(self, alpha=None, standardized=False, method="smoother"):
        """``Metran.get_simulated_means`` (metran.py:758-795): tensor ``[R,T,N]`` (padding steps included)."""
        return self._simulate(alpha, standardized, method)[0]

    def get_simulated_variances(self, alpha=None, standardized=False, method="smoother"):
        """``Metran.get_simulated_variances`` (metran.py:797-829)."""
        return self._simulate(alpha, standardized, method)[1]

    # ------------------------------------------------------------------ leave-one-out predictions (outlier screening)
    def _loo(self, alpha, standardized):
        out = self._run("loo", alpha)  # original units
        return self._units(out["loo_means"], out["loo_vars"], standardized)

    def get_loo_simulated_means(self, alpha=None, standardized=False):
        """Leave-one-out means ``[R,T,N]``: at every observed cell the series' value predicted from every OTHER observation
        of the model -- what ``mask_observations`` of that one cell followed by ``get_simulated_means`` gives there (the
        outlier screen of Metran's worked example), for all cells at once; parameters held fixed.  NaN where the cell is
        not observed (``get_simulated_means`` serves those)."""
        return self._loo(alpha, standardized)[0]

    def get_loo_simulated_variances(self, alpha=None, standardized=False):
        """Leave-one-out variances ``[R,T,N]`` of the projected state at every observed cell (NaN elsewhere)."""
        return self._loo(alpha, standardized)[1]

    def get_loo_simulation(self, r, name, alpha=None, ci=0.05, standardized=False):
        """``get_simulation``'s DataFrame (``mean``, ``lower``, ``upper``) of the leave-one-out predictions of series ``name`` of
        model ``r``: row t is what ``get_simulation`` returns at t after masking the observation at t alone; NaN rows where
        the series is not observed."""
        j = self._series(r, name)
        return self._series_band(r, j, *self._loo(alpha, standardized), ci)

    def get_deletion_residuals(self, alpha=None):
        """Deletion residuals ``[R,T,N]``: (y - loo mean) / sqrt(loo variance) at every observed cell, NaN elsewhere -- the
        same number in standardised and original units.  A large magnitude flags an outlier."""
        import torch

        means, variances = self._loo(alpha, True)
        obs = self.kf.obs
        return torch.where(torch.isfinite(obs), (obs - means) / torch.sqrt(variances), torch.full_like(means, float("nan")))

    # ------------------------------------------------------------------ leave-block-out predictions (gap filling)
    def get_gap_predictions(self, gaps, alpha=None, standardized=False):
        """How well GAPS would be filled: for every gap ``(model, series name, start, end)`` -- start and end timestamps on the
        model's index or integer steps, end exclusive, None = the end of the record -- the observations inside it are predicted
        from every observation OUTSIDE it (``BatchedKalman.block_predict``; parameters held fixed), which is what
        ``mask_observations`` of the gap followed by ``get_simulation`` gives there, for all gaps in one pass.  Returns a
        DataFrame with one row per observed cell of a gap, indexed (model, series, gap, time): ``observed``, ``predicted`` and
        ``stderr`` (of the projected state, as ``get_loo_simulation``'s band) in ORIGINAL units, or standardised ones.
        ``frame.attrs["gaps"]`` has one row per gap: ``n_obs``, ``quad`` (the errors' quadratic form in their covariance),
        ``logdet`` and ``degenerate``.  A gap may span at most ``kf.block_max_cells`` = 64 steps."""
        from pandas import DataFrame, MultiIndex

        limit = int(self.kf.block_max_cells)
        per_model = [[] for _ in range(self.R)]
        for model, name, start, end in gaps:
            r = int(model) - self.shard[0]
            if not 0 <= r < self.R:
                raise IndexError("model %s is not one of this batch" % (model,))
            t0, t1 = self._effect_step(r, start), self._effect_step(r, end, end=True)
            if not t0 < t1:
                raise ValueError("a gap must end after it starts (model %s, series %s)" % (model, name))
            if t1 - t0 > limit:
                raise ValueError("a gap of %d steps is longer than the limit of %d steps (model %s, series %s)" % (t1 - t0, limit, model, name))
            per_model[r].append((self._series(r, name), t0, t1))
        W = max(len(b) for b in per_model) if per_model else 0
        if W < 1:
            raise ValueError("gaps must name at least one gap")
        table = tuple(tuple(b + [(-1, 0, 0)] * (W - len(b))) for b in per_model)   # unused slots for the models with fewer
        out = self._run("blocks", alpha, table)
        means, variances = out["means"].cpu().numpy(), out["vars"].cpu().numpy()
        summary, flags = out["summary"].cpu().numpy(), out["flags"].cpu().numpy()
        obs, std, mean = self.kf.obs.cpu().numpy(), self._std.cpu().numpy(), self._mean.cpu().numpy()
        rows, labels, grows, glabels = [], [], [], []
        for r, blocks in enumerate(per_model):
            index = self.batch.index[r]
            for w, (j, t0, t1) in enumerate(blocks):
                name = self.batch.names[r][j]
                glabels.append((r + self.shard[0], name, w))
                grows.append({"start": index[t0], "steps": t1 - t0, "n_obs": int(summary[r, w, 0]), "quad": summary[r, w, 1],
                              "logdet": summary[r, w, 2], "degenerate": bool(flags[r, w] & 1)})
                for c in range(t1 - t0):
                    y = obs[r, t0 + c, j]
                    if not np.isfinite(y):
                        continue
                    m, v = means[r, w, c], variances[r, w, c]
                    if standardized:
                        m, v = (m - mean[r, j]) / std[r, j], v / std[r, j] ** 2
                    else:
                        y = y * std[r, j] + mean[r, j]
                    labels.append((r + self.shard[0], name, w, index[t0 + c]))
                    rows.append({"observed": y, "predicted": m, "stderr": np.sqrt(v)})
        frame = DataFrame(rows, columns=["observed", "predicted", "stderr"],
                          index=MultiIndex.from_tuples(labels, names=["model", "series", "gap", "time"]))
        frame.attrs["gaps"] = DataFrame(grows, index=MultiIndex.from_tuples(glabels, names=["model", "series", "gap"]))
        return frame

    def gap_fill_skill(self, lengths=(7, 30), alpha=None, t_first=1, coverage=0.95, budget=None):
        """GAP-FILLING SKILL by gap length: every series is tiled with consecutive blocks of ``length`` steps from ``t_first``
        (the last block of a record may be shorter; blocks without an observation are skipped), each block is predicted from
        everything outside it (``BatchedKalman.block_predict``; length 1 is ``loo_predict``) and the errors are summarised per
        (model, series, length): ``n_blocks``, ``n_cells``; ``bias`` = mean error and ``rmse`` in ORIGINAL units; ``msse`` = the
        mean over the blocks of quad / m, quad the errors' quadratic form in their joint covariance and m the block's cells
        (about 1 for an adequate model); ``coverage`` = the share of the cells inside the central ``coverage`` band;
        ``log_score`` = the mean of (m log 2 pi + log det V + quad) / m in standardised units; and ``rmse_loo``, the same
        cells' leave-one-out error (``get_deletion_residuals``' route) -- by what factor leave-one-out flatters the filling
        of a gap of that length.  NaN where ``n_blocks`` = 0.  The models are taken in chunks whose checkpoints and outputs
        stay within ``budget`` bytes (default: 0.8 of the free device memory); the reduction runs on the device."""
        import torch
        from pandas import DataFrame, concat
        from scipy.stats import norm

        t_first, limit = int(t_first), int(self.kf.block_max_cells)
        lengths = [int(h) for h in lengths]
        if t_first < 0 or not lengths or min(lengths) < 1 or max(lengths) > limit:
            raise ValueError("t_first must be >= 0 and the lengths in 1..%d" % limit)
        if not 0.0 < coverage < 1.0:
            raise ValueError("coverage must be between 0 and 1")
        a = self._alpha(alpha)
        zq = float(norm.ppf(0.5 + coverage / 2.0))
        kf, R, N, T = self.kf, self.R, self.N, self.T
        dev = a.device
        obs = kf.obs.to(dev)                                                    # standardised records [R,T,N]
        seen_host = torch.isfinite(obs).cpu().numpy()
        std = self._std.to(dev)
        rec_len = np.asarray(self.batch.lengths, dtype=np.int64)
        lm, lv = self._loo(a, True)                                            # standardised leave-one-out moments
        loo_err = torch.where(torch.isfinite(obs), obs - lm, torch.zeros_like(obs))
        frames = []
        for h in lengths:
            # the blocks of every model, series by series in slots of their own (those without an observation are left out, a
            # series with fewer blocks has unused slots): the sums over a series' slots have a fixed order
            per_series = [[[(j, t0, min(t0 + h, int(rec_len[r]))) for t0 in range(t_first, int(rec_len[r]), h)
                            if seen_host[r, t0:min(t0 + h, int(rec_len[r])), j].any()] for j in range(N)] for r in range(R)]
            Ws = max(1, max(len(b) for blocks in per_series for b in blocks))
            W = N * Ws
            table = torch.tensor([[b + [(-1, 0, 0)] * (Ws - len(b)) for b in blocks] for blocks in per_series],
                                 dtype=torch.int64).reshape(R, W, 3)
            tab = table.to(dev)
            used = tab[..., 0] >= 0
            js = tab[..., 0].clamp_min(0)
            steps = tab[..., 1, None] + torch.arange(h, device=dev)[None, None, :]                 # [R,W,h]
            inside = used[..., None] & (steps < tab[..., 2, None])
            tt = steps.clamp_max(T - 1)
            rr = torch.arange(R, device=dev)[:, None, None].expand_as(tt)
            y = obs[rr, tt, js[..., None].expand_as(tt)]
            cell = inside & torch.isfinite(y)
            if h == 1:    # one-cell blocks: the leave-one-out predictions
                pm = lm[rr, tt, js[..., None].expand_as(tt)]
                pv = lv[rr, tt, js[..., None].expand_as(tt)]
                rv = torch.zeros((R, N), dtype=obs.dtype, device=dev) if getattr(kf, "obsvar", None) is None else kf.obsvar.to(dev)
                vfull = pv[..., 0] + rv[torch.arange(R, device=dev)[:, None], js]
                e0 = torch.where(cell[..., 0], y[..., 0] - pm[..., 0], torch.zeros_like(vfull))
                m = cell[..., 0].to(obs.dtype)
                quad, logdet = e0 * e0 / vfull, torch.log(vfull)
            else:
                pm = torch.full((R, W, h), float("nan"), dtype=obs.dtype, device=dev)
                pv = torch.full_like(pm, float("nan"))
                summary = torch.empty((R, W, 4), dtype=obs.dtype, device=dev)
                chunk = _blocks_that_fit(kf, W, h, budget)
                kf.set_scaling(None, None)                                     # standardised units; the facade's scaling is put back
                try:
                    phi, q = kf.params_from_alpha(a, dt=self.dt)
                    for r0 in range(0, R, chunk):
                        r1 = min(R, r0 + chunk)
                        whole = r0 == 0 and r1 == R
                        sub = kf if whole else kf.subset(np.arange(r0, r1))
                        out = sub.block_predict(phi[r0:r1], q[r0:r1], table[r0:r1])
                        check_status(out["status"].reshape(-1), "MetranBatch(blocks)")
                        width = min(h, int(out["means"].shape[2]))       # the longest block of the chunk
                        pm[r0:r1, :, :width], pv[r0:r1, :, :width] = out["means"][..., :width], out["vars"][..., :width]
                        summary[r0:r1] = out["summary"]
                finally:
                    kf.set_scaling(self._std, self._mean)
                m, quad, logdet = summary[..., 0], summary[..., 1], summary[..., 2]
            good = used & (m > 0) & torch.isfinite(quad)                       # a degenerate block is left out
            cell = cell & good[..., None]
            zero = torch.zeros_like(y)
            err = torch.where(cell, y - pm, zero)
            inband = (cell & (err.abs() <= zq * torch.sqrt(torch.where(cell, pv, zero + 1.0)))).to(obs.dtype)
            le = torch.where(cell, loo_err[rr, tt, js[..., None].expand_as(tt)], zero)
            mm = torch.where(good, m, torch.ones_like(m))
            per_block = torch.stack([good.to(obs.dtype), cell.sum(2).to(obs.dtype), err.sum(2), (err * err).sum(2),
                                     torch.where(good, quad / mm, zero[..., 0]), inband.sum(2),
                                     torch.where(good, (mm * np.log(2.0 * np.pi) + logdet + quad) / mm, zero[..., 0]), (le * le).sum(2)], dim=2)
            sums = torch.where(used[..., None], per_block, torch.zeros_like(per_block)).reshape(R, N, Ws, 8).sum(2)
            nb = sums[..., 0]
            nbn = torch.where(nb > 0, nb, torch.full_like(nb, float("nan")))
            nc = torch.where(sums[..., 1] > 0, sums[..., 1], torch.full_like(nb, float("nan")))
            cols = torch.stack([nb, sums[..., 1], sums[..., 2] / nc * std, torch.sqrt(sums[..., 3] / nc) * std, sums[..., 4] / nbn,
                                sums[..., 5] / nc, sums[..., 6] / nbn, torch.sqrt(sums[..., 7] / nc) * std], dim=2).cpu().numpy().reshape(R * N, 8)
            index = self._rows(lambda r, h=h: ((name, h) for name in self.batch.names[r]), ["series", "length"])
            frames.append(DataFrame({"n_blocks": cols[:, 0].astype(np.int64), "n_cells": cols[:, 1].astype(np.int64), "bias": cols[:, 2],
                                     "rmse": cols[:, 3], "msse": cols[:, 4], "coverage": cols[:, 5], "log_score": cols[:, 6],
                                     "rmse_loo": cols[:, 7]}, index=index))
        order = self._rows(lambda r: ((name, h) for name in self.batch.names[r] for h in lengths), ["series", "length"])
        return concat(frames).reindex(order)

    # ------------------------------------------------------------------ one-step-ahead innovations (model adequacy)
    def get_innovations(self, alpha=None, standardized=True):
        """One-step-ahead prediction errors ``[R,T,N]`` of every observed cell (NaN elsewhere).  ``standardized=True``:
        ``e = v / sqrt(f)``, independent N(0,1) under the fitted model -- the same number in standardised and original units.
        ``standardized=False``: the pair ``(v, f)`` of raw innovations and their variances, in the units the filter runs in
        (the standardised series).  Cell (t, j) is predicted from the past and from the series before j of the same step (the
        filter's sequential updates), so ``v`` and ``f`` -- not the whiteness of ``e`` -- depend on the order of the series."""
        import torch

        out = self._run("innov", alpha)
        if not standardized:
            return out["v"], out["f"]
        return out["v"] / torch.sqrt(out["f"])

    def get_prediction(self, r, name, alpha=None, ci=0.05, standardized=False):
        """The ONE-STEP-AHEAD counterpart of ``get_simulation``: DataFrame (``mean``, ``lower``, ``upper``) of the forecast of
        series ``name`` of model ``r`` at every step from the observations before that step alone -- the band is that of the
        OBSERVATION (projected state variance plus observation variance), defined at every step, observed or not, and
        independent of the order of the series.  ``ci=None`` returns the mean Series."""
        j = self._series(r, name)
        out = self._run("innov", alpha)  # original units
        return self._series_band(r, j, *self._units(out["pred_mean"], out["pred_var"], standardized), ci)

    def test_whiteness(self, alpha=None, nlags=10, t_first=1):
        """Portmanteau (Ljung-Box) check of every series' standardised innovations: DataFrame indexed (model, series) with
        ``nobs`` (cells used: observed, ``t >= t_first``), ``mean`` and ``var`` of ``e``, ``Q = m (m + 2) sum_l r_l^2 / (m - l)``,
        ``pvalue = chi2.sf(Q, nlags)`` and the autocorrelations ``r1 .. r<nlags>``.  Lags count successive OBSERVED cells of the
        series, not calendar steps (the portmanteau test on the non-missing values; Metran's records are sparse).  A small
        p-value says the model's noise is not white: the model is not adequate for that series.  NO degrees of freedom are
        subtracted for the estimated parameters (the textbook correction for a fitted ARMA model would use ``nlags - p``): the
        p-value is on the generous side for a calibrated model.  ``t_first=1`` leaves out the first step, whose prediction is
        the initial state's.  NaN where a series has no more than ``nlags`` cells or does not vary."""
        from pandas import DataFrame
        from scipy.stats import chi2

        nlags = int(nlags)
        out = self._run("innov", alpha)
        stats = self.kf.innovation_stats(out["v"], out["f"], nlags=nlags, t_first=t_first).cpu().numpy()
        flat = stats.reshape(self.R * self.N, 4 + nlags)
        frame = DataFrame({"nobs": flat[:, 0].astype(np.int64), "mean": flat[:, 1], "var": flat[:, 2], "Q": flat[:, 3],
                           "pvalue": chi2.sf(flat[:, 3], nlags)},
                          index=self._rows(lambda r: ((name,) for name in self.batch.names[r]), ["series"]))
        for l in range(1, nlags + 1):
            frame["r%d" % l] = flat[:, 3 + l]
        return frame

    # ------------------------------------------------------------------ residual diagnostics (normality, variance, cross-series)
    def _residual_kept(self, alpha):
        """``(cached "innov" result, the residual sums derived from it so far)``: a dict of its own, keyed by request and tied
        to that very result -- when the cache replaces or drops the innovations (another parameter set, new observations) the
        sums derived from the old ones go with them."""
        out = self._run("innov", alpha)
        kept = getattr(self, "_resid_kept", None)
        if kept is None or kept[0] is not out:
            kept = self._resid_kept = (out, {})
        return out, kept[1]

    def _residual_stats(self, alpha, t_first):
        """``(cached "innov" result, BatchedKalman.residual_series of it)`` for the parameter set, one tensor per ``t_first``."""
        out, kept = self._residual_kept(alpha)
        key = ("series", int(t_first))
        if key not in kept:
            kept[key] = self.kf.residual_series(out["v"], out["f"], t_first=int(t_first))
        return out, kept[key]

    def _residual_cross(self, alpha, t_first, nlags):
        """``(counts, sums)`` ``[R,nlags+1,N,N]`` of ``BatchedKalman.residual_cross`` as numpy arrays, kept the same way."""
        out, stats = self._residual_stats(alpha, t_first)
        kept = self._resid_kept[1]
        key = ("cross", int(t_first), int(nlags))
        if key not in kept:
            counts, sums = self.kf.residual_cross(out["v"], out["f"], stats, nlags=int(nlags), t_first=int(t_first))
            kept[key] = (counts.cpu().numpy(), sums.cpu().numpy())
        return kept[key]

    def _step_times(self, steps):
        """Calendar steps ``[R*N]`` (-1: none) of every (model, series) row as time stamps of each model's own index."""
        from pandas import DatetimeIndex, NaT

        steps = np.asarray(steps).reshape(self.R, self.N)
        return DatetimeIndex([self.batch.index[r][int(t)] if 0 <= t < len(self.batch.index[r]) else NaT
                              for r in range(self.R) for t in steps[r]])

    def test_normality(self, alpha=None, t_first=1):
        """Jarque-Bera check of every series' standardised innovations ``e`` (statsmodels' ``test_normality``): DataFrame
        indexed (model, series) with ``nobs`` (cells used: observed, ``t >= t_first``), ``skew = m3 / m2^1.5``, ``kurtosis =
        m4 / m2^2`` (central moments with divisor m; 3 for a normal), ``JB = m / 6 (skew^2 + (kurtosis - 3)^2 / 4)`` and
        ``pvalue = chi2.sf(JB, 2)``.  The chi-square law is asymptotic: with a few dozen cells the test is conservative.  NaN
        where a series has fewer than 4 cells or does not vary."""
        from pandas import DataFrame

        from .residuals import normality

        cols = normality(self._residual_stats(alpha, t_first)[1].cpu().numpy().reshape(self.R * self.N, 12))
        return DataFrame(cols, index=self._rows(lambda r: ((name,) for name in self.batch.names[r]), ["series"]))

    def test_heteroskedasticity(self, alpha=None, t_first=1):
        """Is the variance of every series' standardised innovations ``e`` constant over the record?  DataFrame indexed (model,
        series) with ``nobs``; the break-variance test of statsmodels / STAMP: ``h = (nobs + 1) // 3``, ``H`` = the sum of
        ``e^2`` over the LAST ``h`` observed cells over that of the FIRST ``h`` (thirds of the sequence of observed cells, as
        ``test_whiteness`` counts its lags) and the two-sided ``pvalue = 2 min(F.cdf(H, h, h), F.sf(H, h, h))``; and the two
        running checks, with ``d = e - mean`` and ``s^2`` its variance (divisor m): ``cusum = max_k |sum_{i<=k} d_i| / sqrt(m
        s^2)`` (a shift of the LEVEL) and ``cusumsq = sqrt(m / 2) max_k |sum_{i<=k} d_i^2 / (m s^2) - k / m|`` (a shift of the
        VARIANCE, Brown-Durbin-Evans), each with the time stamp of the cell at which the excursion is largest (``cusum_time``,
        ``cusumsq_time``, from the model's own index: where the break is) and ``cusum_pvalue`` / ``cusumsq_pvalue`` =
        ``scipy.special.kolmogorov`` of the statistic, the law of the supremum of a Brownian bridge.  That limit is
        ASYMPTOTIC and, for ``cusumsq``, assumes GAUSSIAN ``e``: on finite records both are conservative (they reject less
        often than the level says).  NaN where ``h = 0``, the first third's sum is 0 or the series does not vary."""
        from pandas import DataFrame

        from .residuals import heteroskedasticity

        c = heteroskedasticity(self._residual_stats(alpha, t_first)[1].cpu().numpy().reshape(self.R * self.N, 12))
        frame = DataFrame({"nobs": c["nobs"], "h": c["h"], "H": c["H"], "pvalue": c["pvalue"],
                           "cusum": c["cusum"], "cusum_time": self._step_times(c["cusum_step"]), "cusum_pvalue": c["cusum_pvalue"],
                           "cusumsq": c["cusumsq"], "cusumsq_time": self._step_times(c["cusumsq_step"]),
                           "cusumsq_pvalue": c["cusumsq_pvalue"]},
                          index=self._rows(lambda r: ((name,) for name in self.batch.names[r]), ["series"]))
        return frame

    def test_cross_correlation(self, alpha=None, nlags=5, min_pairs=20, t_first=1):
        """Are the standardised innovations of DIFFERENT series of a model uncorrelated -- at the same step and at the lags
        ``1 .. nlags`` in CALENDAR steps?  Under the fitted model they are independent N(0,1) across time and across series;
        correlation that remains between two series is the signature of a common factor that is missing or has the wrong
        loadings.  ``e[t,j]`` is CONDITIONED on the series before ``j`` of the same step (the filter's sequential updates), so
        ``r_ij(0)`` is the correlation left AFTER the model's own account of the two series' common part -- exactly what the
        test is for.  With ``e~`` the innovations of a series centred and scaled by their own mean and standard deviation,
        ``n_ij(l)`` the number of steps t at which (t, i) and (t - l, j) are both observed (``t - l >= t_first``) and ``r_ij(l) =
        sum e~[t,i] e~[t-l,j] / n``: DataFrame indexed by model with ``Q = sum n r^2`` over the pairs ``i < j`` at lag 0 and
        ``i != j`` at the lags >= 1 that have ``n >= min_pairs``, ``df`` = the number of those terms, ``pvalue = chi2.sf(Q,
        df)``, and the term of largest ``|z|``, ``z = r sqrt(n)``: ``series_a``, ``series_b``, ``lag``, ``r``, ``z``
        (``series_a`` at t, ``series_b`` at t - lag).  As in ``test_whiteness`` NO degrees of freedom are subtracted for the
        estimated parameters: the p-value is on the generous side for a calibrated model.  NaN where no pair has
        ``min_pairs`` common steps."""
        from pandas import DataFrame, Index

        from .residuals import cross_correlation

        counts, sums = self._residual_cross(alpha, t_first, nlags)
        rows = []
        for r in range(self.R):
            c = cross_correlation(counts[r], sums[r], min_pairs)
            w = c["worst"]
            names = self.batch.names[r]
            rows.append({"Q": c["Q"], "df": c["df"], "pvalue": c["pvalue"], "series_a": None if w is None else names[w[0]],
                         "series_b": None if w is None else names[w[1]], "lag": -1 if w is None else w[2],
                         "r": np.nan if w is None else w[3], "z": np.nan if w is None else w[4]})
        return DataFrame(rows, index=Index([r + self.shard[0] for r in range(self.R)], name="model"),
                         columns=["Q", "df", "pvalue", "series_a", "series_b", "lag", "r", "z"])

    def get_residual_correlations(self, r, lag=0, nlags=None, alpha=None, t_first=1):
        """The ``N x N`` DataFrame of ``r_ij(lag)`` of model ``r`` (``test_cross_correlation``): row ``i`` at step t against
        column ``j`` at step t - ``lag`` (calendar steps), rows / columns by series name; the diagonal at lag 0 is 1 and at
        other lags the series' own calendar-lag autocorrelation.  NaN where the two have no common step.  ``nlags``: the
        number of lags of the device run to read from (default: ``lag``; a run already made for ``test_cross_correlation`` is
        reused when given the same)."""
        from pandas import DataFrame

        from .residuals import correlations

        lag = int(lag)
        nlags = lag if nlags is None else int(nlags)
        if not 0 <= lag <= nlags:
            raise ValueError("lag must be in 0..nlags")
        if not 0 <= int(r) < self.R:
            raise IndexError("model %d is outside the batch's %d models" % (int(r), self.R))
        counts, sums = self._residual_cross(alpha, t_first, nlags)
        names = list(self.batch.names[r])
        return DataFrame(correlations(counts[r, lag], sums[r, lag]), index=names, columns=names)

    def screen_residuals(self, alpha=None, nlags=10, level=0.01, t_first=1):
        """The residual checks side by side, one row per (model, series): the p-values ``whiteness`` (``test_whiteness`` with
        ``nlags``), ``normality`` (``test_normality``), ``heteroskedasticity`` (``test_heteroskedasticity``'s ``H``) and
        ``cross_correlation`` (``test_cross_correlation`` with ``nlags``; the model's value repeated on its rows), and
        ``flag``: True where any of them is below ``level``.  A NaN p-value (too few cells) does not flag."""
        from pandas import DataFrame

        white = self.test_whiteness(alpha, nlags=nlags, t_first=t_first)
        cross = self.test_cross_correlation(alpha, nlags=nlags, t_first=t_first)["pvalue"].values
        frame = DataFrame({"whiteness": white["pvalue"].values,
                           "normality": self.test_normality(alpha, t_first=t_first)["pvalue"].values,
                           "heteroskedasticity": self.test_heteroskedasticity(alpha, t_first=t_first)["pvalue"].values,
                           "cross_correlation": np.repeat(cross, self.N)}, index=white.index)
        with np.errstate(invalid="ignore"):
            frame["flag"] = (frame.values < float(level)).any(axis=1)
        return frame

    # ------------------------------------------------------------------ multi-step-ahead forecasts and their skill
    def _forecast(self, alpha, outputs, horizon=1, track_horizon=1, t_first=1, coverage=0.95):
        """``BatchedKalman.forecast`` for the parameter set: the cached kind "forecast", one result per REQUEST (outputs,
        horizon, track horizon, first origin, coverage); fan and track in ORIGINAL units."""
        return self._run("forecast", alpha, (tuple(outputs), int(horizon), int(track_horizon), int(t_first), float(coverage)))

    def _forecast_moments(self, steps, alpha, standardized):
        out = self._forecast(alpha, ("fan",), horizon=steps)
        return self._units(out["fan_mean"], out["fan_var"], standardized)

    def get_forecast_means(self, steps=14, alpha=None, standardized=False):
        """OUT-OF-SAMPLE forecast means ``[R,steps,N]``: row h - 1 is the forecast of every series h steps after the model's
        last real step (``lengths[r] - 1``), from all of its observations."""
        return self._forecast_moments(steps, alpha, standardized)[0]

    def get_forecast_variances(self, steps=14, alpha=None, standardized=False):
        """The variances ``[R,steps,N]`` of ``get_forecast_means``: those of the OBSERVATION (projected state variance plus
        observation variance)."""
        return self._forecast_moments(steps, alpha, standardized)[1]

    def get_forecast(self, r, name, steps=14, alpha=None, ci=0.05, standardized=False):
        """The forecast of series ``name`` of model ``r`` over the ``steps`` days after the model's last real step: DataFrame
        (``mean``, ``lower``, ``upper``) whose index continues the record's daily index; the band is that of the OBSERVATION, as
        in ``get_prediction``.  ``ci=None`` returns the mean Series."""
        from pandas import Series, Timedelta, date_range

        j = self._series(r, name)
        means, variances = self._forecast_moments(steps, alpha, standardized)
        index = date_range(self.batch.index[r][-1] + Timedelta(days=1), periods=int(steps), freq="D")
        mean = Series(means[r, :, j].cpu().numpy(), index=index, name=name)
        return self._band(mean, Series(variances[r, :, j].cpu().numpy(), index=index, name=name) if ci is not None else None, ci)

    def get_prediction_at(self, r, name, horizon, alpha=None, ci=0.05, standardized=False):
        """The ``horizon``-STEP-AHEAD counterpart of ``get_prediction``: DataFrame (``mean``, ``lower``, ``upper``) of the forecast
        of series ``name`` of model ``r`` at every step t made ``horizon`` steps earlier, from the observations up to step
        t - horizon alone (from the initial state where t < horizon) -- what one plots against the observations to see how
        far ahead the model is worth anything.  ``horizon=1`` is ``get_prediction``."""
        j = self._series(r, name)
        out = self._forecast(alpha, ("track",), track_horizon=horizon)  # original units
        return self._series_band(r, j, *self._units(out["track_mean"], out["track_var"], standardized), ci)

    def forecast_skill(self, horizon=14, alpha=None, t_first=1, coverage=0.95):
        """Forecast skill by horizon, the out-of-sample counterpart of ``test_whiteness``: DataFrame indexed (model, series,
        horizon) over the pairs (origin o, target t = o + h) with ``o >= t_first`` and the series observed at t, every
        forecast made from the observations up to o alone (parameters held fixed): ``nobs``; ``bias`` = mean error and ``rmse``
        in ORIGINAL units; ``msse`` = mean of e^2 / s (about 1 for an adequate model: the bands are honest); ``logscore`` =
        -(log 2 pi + mean log s + msse) / 2 in standardised units; ``coverage`` = the share of the pairs inside the central
        ``coverage`` band, beside ``nominal``; ``skill`` = 1 - mse / var, var the variance of the series' standardised
        observations: the gain over predicting the series' mean.  NaN where ``nobs`` = 0.  Padding steps of a shorter record
        are empty and add no pairs."""
        import torch
        from pandas import DataFrame

        horizon = int(horizon)
        out = self._forecast(alpha, ("skill",), horizon=horizon, t_first=t_first, coverage=coverage)
        s = out["skill"].cpu().numpy().reshape(self.R * self.N, horizon, 6)
        obs = self.kf.obs
        seen = torch.isfinite(obs)
        cnt = seen.sum(1).to(obs.dtype)
        mean = torch.where(seen, obs, torch.zeros_like(obs)).sum(1) / cnt
        var = (torch.where(seen, obs - mean[:, None, :], torch.zeros_like(obs)) ** 2).sum(1) / cnt   # [R,N], divisor m
        var = np.repeat(var.cpu().numpy().reshape(-1), horizon)
        std = np.repeat(self._std.cpu().numpy().reshape(-1), horizon)
        index = self._rows(lambda r: ((name, h) for name in self.batch.names[r] for h in range(1, horizon + 1)), ["series", "horizon"])
        flat = s.reshape(-1, 6)
        with np.errstate(invalid="ignore", divide="ignore"):
            m = np.where(flat[:, 0] > 0, flat[:, 0], np.nan)
            mse, msse = flat[:, 2] / m, flat[:, 3] / m
            frame = DataFrame({"nobs": flat[:, 0].astype(np.int64), "bias": flat[:, 1] / m * std, "rmse": np.sqrt(mse) * std, "msse": msse,
                               "logscore": -0.5 * (np.log(2.0 * np.pi) + flat[:, 4] / m + msse), "coverage": flat[:, 5] / m,
                               "nominal": np.where(np.isnan(m), np.nan, float(coverage)), "skill": 1.0 - mse / var}, index=index)
        return frame

    # ------------------------------------------------------------------ observation weights (which data a number comes from)
    def _target_steps(self, r, times):
        """``times`` of the weight accessors as integer steps of model ``r``: timestamps on the model's index or integer steps,
        one or a list."""
        from pandas import Timestamp

        index = self.batch.index[r]
        if isinstance(times, (str, Timestamp, np.datetime64, int, np.integer)) or not hasattr(times, "__iter__"):
            times = [times]
        steps = []
        for t in times:
            if isinstance(t, (int, np.integer)):
                if not 0 <= int(t) < len(index):
                    raise IndexError("step %d is outside the model's %d steps" % (int(t), len(index)))
                steps.append(int(t))
            else:
                pos = index.get_indexer([Timestamp(t)])[0]
                if pos < 0:
                    raise KeyError("%s is not on the index of model %d" % (t, r))
                steps.append(int(pos))
        if not steps:
            raise ValueError("times must name at least one step")
        return steps

    def _weights(self, r, column, steps, what, alpha):
        """``BatchedKalman.observation_weights`` for the targets (step, column) of model ``r``: ``(w [M,T,N], intercept [M])`` on
        the device, in the filter's units; the cached kind "weights", one result per request (model, column, steps, what)."""
        out = self._run("weights", alpha, (int(r), int(column), tuple(steps), what))
        return out["weights"][0], out["intercept"][0]

    def _weight_frames(self, r, steps, w, intercept):
        from pandas import DataFrame

        L = int(self.batch.lengths[r])
        w, intercept = w.cpu().numpy(), intercept.cpu().numpy()
        frames = {}
        for m, s in enumerate(steps):
            frame = DataFrame(w[m, :L], index=self.batch.index[r], columns=list(self.batch.names[r]))
            frame.attrs["intercept"] = float(intercept[m])
            frames[self.batch.index[r][s]] = frame
        return frames

    def get_observation_weights(self, r, name, times, alpha=None, standardized=False):
        """Which observations the smoothed value of series ``name`` of model ``r`` comes from (``get_simulation``'s mean, e.g. a
        gap-filled value): for fixed parameters the smoother is linear in the data, so that mean is a weighted sum of the model's
        observations (Koopman & Harvey 2003; ``BatchedKalman.observation_weights``).  ``times``: timestamps on the model's index
        or integer steps, one or a list.  Returns a dict timestamp -> DataFrame (index = the model's time index, columns = its
        series) of the weights, NaN where a series is not observed; the part that comes from the initial state is
        ``frame.attrs["intercept"]`` (0 for the default initial state).  Original units (the default): with y the observations,
        ``sum_i,t w (y_i - mean_i) + mean_name + intercept`` is ``get_simulation``'s mean at that time -- the weight of series i is
        ``w std_name / std_i`` of the standardised one.  ``standardized=True``: the units the filter runs in,
        ``sum w y_standardised + intercept`` is the standardised mean."""
        j = self._series(r, name)
        steps = self._target_steps(r, times)
        w, intercept = self._weights(r, j, steps, "series", alpha)
        if not standardized:
            w = w * (self._std[r, j] / self._std[r])[None, None, :]
            intercept = intercept * self._std[r, j]
        return self._weight_frames(r, steps, w, intercept)

    def get_state_weights(self, r, i, times, alpha=None):
        """``get_observation_weights`` for state ``i`` of model ``r`` (``get_state``'s mean), in the filter's units:
        ``sum w y_standardised + intercept`` is the smoothed state."""
        self._check_state(i)
        steps = self._target_steps(r, times)
        w, intercept = self._weights(r, int(i), steps, "states", alpha)
        return self._weight_frames(r, steps, w, intercept)

    def get_weight_shares(self, r, name, times, alpha=None, mass=0.9):
        """What the smoothed value of series ``name`` of model ``r`` at ``times`` leans on, one row per (time, source series):
        ``sum_w`` (the sum of the series' weights over time), ``share`` (``sum_t |w|`` of the series over ``sum_t,i |w|`` of all,
        in standardised units: the shares of a time add up to 1) and ``first`` / ``last``, the time stamps of the SHORTEST run of
        steps that contains the target's step and holds ``mass`` (90 %) of the series' ``sum_t |w|`` -- the earliest such run
        when several are equally short; NaT for a series without weight (never observed).  Reduced on the device; only the
        table crosses to the host."""
        import torch
        from pandas import DataFrame, MultiIndex, NaT

        j = self._series(r, name)
        steps = self._target_steps(r, times)
        w, _ = self._weights(r, j, steps, "series", alpha)          # [M,T,N], standardised units
        M, T, N = (int(s) for s in w.shape)
        w0 = torch.nan_to_num(w, nan=0.0)
        aw = w0.abs().permute(0, 2, 1).reshape(M * N, T).contiguous()   # one row per (target, series)
        tot = aw.sum(1)
        csum = torch.cumsum(aw, 1)                                  # inclusive prefix sums, non-decreasing
        before = csum - aw                                          # the mass before step a
        # for every start a the first end b whose run holds the mass; the run must contain the target's step
        need = before + float(mass) * tot[:, None]
        need = torch.minimum(need, tot[:, None])                    # rounding must not ask for more than there is
        end = torch.searchsorted(csum, need, right=False)
        tstar = torch.as_tensor(steps, device=w.device).repeat_interleave(N)[:, None]
        end = torch.maximum(end, tstar)
        start = torch.arange(T, device=w.device)[None, :]
        ok = (start <= tstar) & (end < T)
        length = torch.where(ok, end - start, torch.full_like(end, 2 * T))
        first = torch.argmin(length, 1)
        last = end.gather(1, first[:, None])[:, 0]
        table = torch.stack([w0.sum(1).reshape(-1), tot / tot.reshape(M, N).sum(1).repeat_interleave(N), first.to(w.dtype), last.to(w.dtype),
                             tot], 1).cpu().numpy()
        index = self.batch.index[r]
        rows = [(index[s], nm) for s in steps for nm in self.batch.names[r]]
        stamp = lambda v, k: index[int(v[k])] if v[4] > 0 else NaT  # noqa: E731
        return DataFrame({"sum_w": table[:, 0], "share": table[:, 1], "first": [stamp(v, 2) for v in table], "last": [stamp(v, 3) for v in table]},
                         index=MultiIndex.from_tuples(rows, names=["time", "series"]))

    # ------------------------------------------------------------------ intervention effects (estimating what the screens found)
    _EFFECT_KINDS = {"level": 0, "ramp": 1}

    def _effect_step(self, r, when, end=False):
        """A start (or exclusive end) of an intervention as a step of model ``r``: a timestamp on its index or an integer step;
        an end may also be the model's length."""
        L = int(self.batch.lengths[r])
        if end and when is None:
            return L
        if end and isinstance(when, (int, np.integer)) and int(when) == L:
            return L
        return self._target_steps(r, when)[0]

    def fit_interventions(self, interventions, alpha=None, t_first=1, standardized=False):
        """Estimate intervention effects by GLS, parameters held fixed (``BatchedKalman.regression``; de Jong's augmented
        filter, what statsmodels' ``mle_regression``, KFAS regression effects and STAMP interventions do): what
        ``get_deletion_residuals`` and ``screen_breaks`` find, estimated instead of masked.  ``interventions``: a list of
        ``(model, series name, kind, start, end=None)`` -- kind ``"level"`` (the series reads a constant off between start and
        end: a pulse for one step, a re-installed sensor for ``end=None``) or ``"ramp"`` (it drifts one unit per step from start
        and holds after end: a change of trend for ``end=None``); start and end are timestamps on the model's index or integer
        steps, end is exclusive, None = to the end of the record.  The steps ``t >= t_first`` count, as in ``get_mle``'s warm-up.

        Returns a DataFrame with one row per effect, indexed (model, effect): ``series, kind, start, end`` (time stamps; end NaT
        = the end of the record), ``n_obs`` (the observations the effect acts on), ``estimate`` and ``stderr`` in the series'
        ORIGINAL units (per step for a ramp; ``standardized=True``: the units the filter runs in), ``t``, ``pvalue`` (two-sided
        normal) and ``dropped`` (True, with NaN estimates, for an effect without observations or collinear with the ones before
        it).  ``frame.attrs["models"]`` is a per-model frame with ``gain`` (the drop of -2 log L), ``df`` (effects kept),
        ``pvalue`` (chi-square with df degrees of freedom), ``obj`` and ``obj_adjusted``.  The standardisation constants are
        those of the RAW series: they are not re-estimated for the adjusted ones."""
        from pandas import DataFrame, Index, MultiIndex, NaT
        from scipy.stats import chi2, norm

        t_first = int(t_first)
        per_model = [[] for _ in range(self.R)]
        for item in interventions:
            model, name, kind, start = item[:4]
            end = item[4] if len(item) > 4 else None
            r = int(model) - self.shard[0]
            if not 0 <= r < self.R:
                raise IndexError("model %s is not one of this batch" % (model,))
            if kind not in self._EFFECT_KINDS:
                raise ValueError("kind must be 'level' or 'ramp'")
            t0, t1 = self._effect_step(r, start), self._effect_step(r, end, end=True)
            if not t0 < t1:
                raise ValueError("an intervention must end after it starts (model %s, series %s)" % (model, name))
            per_model[r].append((self._series(r, name), self._EFFECT_KINDS[kind], t0, t1))
        M = max(len(e) for e in per_model) if per_model else 0
        if M < 1:
            raise ValueError("interventions must name at least one effect")
        table = tuple(tuple(e + [(-1, 0, 0, 1)] * (M - len(e))) for e in per_model)   # unused slots for the models with fewer
        out = self._run("regress", alpha, (table, t_first))
        beta, cov = out["beta"].cpu().numpy(), out["cov"].cpu().numpy()
        support, dropped = out["support"].cpu().numpy(), out["dropped"].cpu().numpy()
        gain, obj = out["gain"].cpu().numpy(), out["obj"].cpu().numpy()
        std = self._std.cpu().numpy()
        rows, labels = [], []
        for r, effects in enumerate(per_model):
            index = self.batch.index[r]
            for m, (j, kind, t0, t1) in enumerate(effects):
                scale = 1.0 if standardized else std[r, j]
                gone = bool((int(dropped[r]) >> m) & 1)
                est, se = beta[r, m] * scale, np.sqrt(cov[r, m, m]) * scale
                tval = est / se
                labels.append((r + self.shard[0], m))
                rows.append({"series": self.batch.names[r][j], "kind": "level" if kind == 0 else "ramp", "start": index[t0],
                             "end": index[t1] if t1 < len(index) else NaT, "n_obs": int(support[r, m]), "estimate": est, "stderr": se,
                             "t": tval, "pvalue": 2.0 * norm.sf(abs(tval)), "dropped": gone})
        frame = DataFrame(rows, index=MultiIndex.from_tuples(labels, names=["model", "effect"]))
        df = np.array([sum(1 for m in range(len(e)) if not (int(dropped[r]) >> m) & 1) for r, e in enumerate(per_model)])
        frame.attrs["models"] = DataFrame({"gain": gain, "df": df, "pvalue": np.where(df > 0, chi2.sf(gain, np.maximum(df, 1)), np.nan),
                                           "obj": obj, "obj_adjusted": obj - gain},
                                          index=Index(np.arange(self.R) + self.shard[0], name="model"))
        frame.attrs["effects"] = np.asarray(table, dtype=np.int64).reshape(self.R, M, 4)
        frame.attrs["beta"] = beta.copy()                  # standardised units: what adjust_observations subtracts
        self.interventions = frame
        return frame

    def adjust_observations(self, table=None):
        """Subtract fitted intervention effects from the records (``table``: a frame of ``fit_interventions``; None = the last
        fit): afterwards ``get_simulation``, ``screen_breaks``, ``test_whiteness`` and ``solve`` run on the adjusted records.  A
        dropped effect subtracts nothing.  A second call starts again from the original records; ``unadjust_observations``
        reverts.  The series' standardisation constants stay those of the raw series."""
        table = getattr(self, "interventions", None) if table is None else table
        if table is None or "effects" not in getattr(table, "attrs", {}):
            raise ValueError("no fitted interventions: call fit_interventions first or pass its frame")
        self.kf.adjust_observations(table.attrs["effects"], table.attrs["beta"])
        self._cache.clear()

    def unadjust_observations(self):
        """The records as they were before ``adjust_observations``."""
        self.kf.unadjust_observations()
        self._cache.clear()

    # ------------------------------------------------------------------ scores of the parameters (uncertainty, stability)
    def _parameter_names(self, r):
        return [c + "_alpha" for c in self._state_columns(r)]

    def _parameter_exists(self):
        """``[R,N+K]`` bool: False for the surplus factor parameters of a model with fewer factors than the batch maximum."""
        return np.arange(self.N + self.K)[None, :] < (self.N + np.asarray(self.nfactors))[:, None]

    def get_scores(self, r, alpha=None, t_first=1):
        """The per-step scores of model ``r`` (``BatchedKalman.scores_alpha``; what statsmodels calls ``score_obs``): DataFrame on
        the model's index, one column per parameter (``<series>_sdf_alpha`` ..., ``cdf1_alpha`` ...), the derivative of every
        step's contribution to -2 log L with respect to that alpha; 0 at a step without observations.  Every step is there,
        also those before ``t_first`` (which only says what the sums count: it is part of the cache key)."""
        from pandas import DataFrame

        out = self._run("scores", alpha, int(t_first))
        L = int(self.batch.lengths[r])
        return DataFrame(out["score"][r, :L].cpu().numpy(), index=self.batch.index[r], columns=self._parameter_names(r))

    def get_parameter_covariance(self, kind="robust", alpha=None, t_first=1):
        """Covariance of the parameter estimates of every model (``metran_amd.scores.parameter_covariance``): ``"opg"`` =
        4 pinv(sum s s') from the per-step scores, positive semi-definite by construction and available for every shape the
        scores serve; ``"hessian"`` = 2 pinv(H) and ``"robust"`` = pinv(H) opg pinv(H) (the sandwich: trustworthy when the model is
        slightly wrong), H the Hessian of -2 log L differenced from the adjoint gradient exactly as ``solve(stderr=True)`` does
        -- where the shape has no adjoint gradient those two raise its message.  ``fit["pcov"]`` keeps the reference's pinv(H),
        half of ``"hessian"``.  The steps ``t >= t_first`` that hold an observation count, in the scores and in the Hessian alike
        (its warm-up is each record's number of non-empty steps before ``t_first``).  Returns a dict of numpy arrays ``pcov
        [R,n,n]``, ``stderr [R,n]`` and ``corr [R,n,n]``; NaN for the parameters a model does not have."""
        from .scores import COVARIANCE_KINDS, parameter_covariance

        if kind not in COVARIANCE_KINDS:
            raise ValueError("kind must be one of %s" % ", ".join(repr(k) for k in COVARIANCE_KINDS))
        hess = None if kind == "opg" else self._run("hessian", alpha, int(t_first))["hessian"]
        out = self._run("scores", alpha, int(t_first))
        pcov = parameter_covariance(out["opg"], out["count"], out["grad"], hess, kind).cpu().numpy()
        gone = ~self._parameter_exists()
        pcov = np.where(gone[:, :, None] | gone[:, None, :], np.nan, pcov)
        var = np.diagonal(pcov, axis1=1, axis2=2)
        with np.errstate(invalid="ignore", divide="ignore"):
            se = np.sqrt(np.where(var >= 0, var, np.nan))
            corr = pcov / (se[:, :, None] * se[:, None, :])
        return {"pcov": pcov, "stderr": se, "corr": corr}

    def test_parameter_stability(self, alpha=None, t_first=1):
        """Nyblom-Hansen test of parameter constancy (``metran_amd.scores.nyblom``): are the response times constant over the
        record?  The parameter-side counterpart of ``screen_breaks``: a well field that started pumping half-way changes a
        series' alpha without necessarily producing one large state disturbance.  DataFrame indexed (model, parameter) with
        ``L`` (the statistic), ``pvalue`` (``cvm_sf(L, 1)``; small = the parameter moved) and ``n_steps`` (the counted steps: ``t
        >= t_first`` with an observation), and per model a row ``joint`` over all its parameters (``cvm_sf(L, k)``).  The scores are
        centred, so the test is also meaningful at a bound or for a model that has not converged.  NaN for the parameters a
        model does not have."""
        from pandas import DataFrame

        from .scores import nyblom

        out = self._run("scores", alpha, int(t_first))
        count = out["count"].cpu().numpy()
        res = nyblom(out["cusum"].cpu().numpy(), out["opg"].cpu().numpy(), out["grad"].cpu().numpy(), count, self._parameter_exists())
        rows = {"L": [], "pvalue": [], "n_steps": []}
        for r in range(self.R):
            rows["L"] += list(res["L_param"][r]) + [res["L"][r]]
            rows["pvalue"] += list(res["pvalue_param"][r]) + [res["pvalue"][r]]
            rows["n_steps"] += [int(count[r])] * (self.N + self.K + 1)
        return DataFrame(rows, index=self._rows(lambda r: [(name,) for name in self._parameter_names(r) + ["joint"]], ["parameter"]))

    # ------------------------------------------------------------------ state disturbances (break detection)
    def get_state_disturbances(self, alpha=None):
        """Smoothed disturbances of the state equation x_t = phi o x_{t-1} + eta_t: ``(mean, variance)`` ``[R,T,N+K]`` of
        ``eta_t`` given ALL data (statsmodels' ``smoothed_state_disturbance`` and its variance), in the filter's units.  With the
        backward pair ``(r, N)`` of ``BatchedKalman.disturbances``: ``mean = q r`` and ``variance = q - q^2 N_ii`` (clipped at 0).
        Row t = 0 is the disturbance between the initial state and the first prediction; padding steps are included."""
        out = self._run("dist", alpha)
        q = out["q"][:, None, :]
        return q * out["r"], (q - q * q * out["ninfo"]).clamp_min(0.0)

    def get_auxiliary_residuals(self, alpha=None, min_information=1e-6):
        """Auxiliary residuals of the state equation ``[R,T,N+K]`` (Harvey & Koopman 1992; KFAS ``rstandard(type = "state")``):
        ``u = r / sqrt(N_ii)``, the smoothed disturbance over its own standard deviation -- formed from the kernel's raw pair,
        never from a difference.  Under the model every ``u`` has unit spread (neighbouring ones are correlated); a large
        magnitude at (t, i) says that state i moved at step t by more than its noise allows: a level shift in a series' own
        state, a shift of a common factor.  NaN beyond a model's own length, and where ``q_i N_ii < min_information``:
        ``q_i N_ii`` in [0,1] is the share of the disturbance's variance that the data determine -- 0 behind the last
        observation and for a state with q = 0 -- and a ratio of two vanishing numbers is not a residual.  The threshold is a
        stated policy, not a measurement."""
        import torch

        out = self._run("dist", alpha)
        r, ninfo = out["r"], out["ninfo"]
        q = out["q"][:, None, :]
        lengths = torch.as_tensor(np.asarray(self.batch.lengths), device=r.device)
        inside = torch.arange(r.shape[1], device=r.device)[None, :, None] < lengths[:, None, None]
        ok = inside & (q * ninfo >= float(min_information))
        return torch.where(ok, r / torch.sqrt(ninfo), torch.full_like(r, float("nan")))

    def get_state_disturbance(self, r, i, alpha=None, ci=0.05):
        """The smoothed disturbance of state ``i`` of model ``r`` with its 1-ci band: DataFrame (``mean``, ``lower``, ``upper``)
        on the model's index, as ``get_state`` returns the state itself; ``ci=None`` returns the mean Series."""
        from pandas import DataFrame

        self._check_state(i)
        mean, variance = self.get_state_disturbances(alpha)
        L = int(self.batch.lengths[r])
        frame = lambda a: DataFrame(a[r, :L].cpu().numpy(), index=self.batch.index[r], columns=self._state_columns(r)).iloc[:, i]  # noqa: E731
        return self._band(frame(mean), frame(variance) if ci is not None else None, ci)

    def screen_breaks(self, alpha=None, t_first=1, min_information=1e-6):
        """One row per (model, state): where the state equation failed most.  DataFrame indexed (model, state) -- states named
        as ``get_state_means`` names them -- with ``max_abs_u`` (the largest auxiliary residual in magnitude over the steps
        ``t >= t_first``), ``time`` (its time stamp), ``nobs`` (the number m of finite residuals searched) and ``pvalue``, the
        Sidak-corrected two-sided normal p-value of the maximum of m residuals, ``1 - (1 - 2 Phi(-max|u|))^m``.  The correction
        treats the m residuals as independent; neighbouring ones are positively correlated, so the p-value is on the
        conservative side.  ``t_first=1`` leaves out the disturbance between the initial state and the first prediction.
        Rows with m = 0 carry NaN (``time`` NaT)."""
        from pandas import DataFrame, NaT
        from scipy.stats import norm

        u = self.get_auxiliary_residuals(alpha, min_information).cpu().numpy()
        rows = []
        for r in range(self.R):
            L = int(self.batch.lengths[r])
            au = np.abs(u[r, int(t_first):L])
            for i in range(self.N + self.K):
                m = int(np.isfinite(au[:, i]).sum())
                if m == 0:
                    rows.append((np.nan, NaT, 0, np.nan))
                    continue
                t = int(np.nanargmax(au[:, i]))
                umax = float(au[t, i])
                rows.append((umax, self.batch.index[r][t + int(t_first)], m, -np.expm1(m * np.log1p(-2.0 * norm.cdf(-umax)))))
        return DataFrame(rows, columns=["max_abs_u", "time", "nobs", "pvalue"],
                         index=self._rows(lambda r: ((name,) for name in self._state_columns(r)), ["state"]))

    # ------------------------------------------------------------------ level shifts at an unknown date
    def get_level_shift_statistics(self, alpha=None, standardized=False):
        """The GLS statistic of a LEVEL SHIFT of every series from every date (``BatchedKalman.level_shifts``; de Jong & Penzer
        1998): a dict of tensors ``[R,T,N]`` -- at cell (t, j) ``estimate`` of a permanent offset of series j from step t on,
        its ``stderr`` and ``t`` = estimate / stderr, parameters held fixed -- what ``fit_interventions`` gives for the single
        effect ``(model, series, "level", t)``, for all dates from one backward pass.  ``estimate`` and ``stderr`` in the series'
        ORIGINAL units (the shift times the series' standard deviation; the mean does not enter) or standardised ones; ``t`` is
        the same in both.  NaN where the cell is not observed.  The first observed cell of a series is the shift of the whole
        record: the series' mean, not a break (``screen_level_shifts`` leaves it out)."""
        import torch

        out = self._run("shifts", alpha)
        key = ("stat", bool(standardized))
        if key not in out:
            num, den = out["num"], out["den"]
            root = torch.sqrt(den)
            scale = 1.0 if standardized else self._std[:, None, :]
            out[key] = {"estimate": num / den * scale, "stderr": scale / root, "t": num / root}
        return dict(out[key])

    def get_level_shift(self, r, name, alpha=None):
        """The level-shift statistics of series ``name`` of model ``r``: DataFrame on the model's index with ``estimate`` and
        ``stderr`` (original units) and ``t``; NaN rows where the series is not observed."""
        from pandas import DataFrame

        j = self._series(r, name)
        stat = self.get_level_shift_statistics(alpha)
        L = int(self.batch.lengths[r])
        return DataFrame({key: stat[key][r, :L, j].cpu().numpy() for key in ("estimate", "stderr", "t")}, index=self.batch.index[r][:L])

    def _shift_candidates(self, t_first, min_segment):
        """``[R,T,N]`` bool: the observed cells at steps >= t_first with at least ``min_segment`` observed cells of their series
        before them and at least ``min_segment`` from them on."""
        seen = np.isfinite(self.kf.obs.cpu().numpy())
        upto = np.cumsum(seen, axis=1)                     # observed cells of the series at the steps <= t
        before, from_on = upto - seen, upto[:, -1:, :] - upto + seen
        cand = seen & (before >= int(min_segment)) & (from_on >= int(min_segment))
        cand[:, :max(int(t_first), 0)] = False
        return cand

    def screen_level_shifts(self, alpha=None, t_first=1, min_segment=10):
        """One row per (model, series): where a level shift fits best.  DataFrame indexed (model, series) with ``max_abs_t`` (the
        largest level-shift t-statistic in magnitude over the candidate dates), ``time`` (its time stamp), ``estimate`` and
        ``stderr`` of the shift from there on (original units), ``ncand`` (the number m of candidates searched) and ``pvalue``,
        the Sidak-corrected two-sided normal p-value of the maximum of m statistics, ``1 - (1 - 2 Phi(-max|t|))^m``.  The
        correction treats the m statistics as independent; neighbouring ones are positively correlated, so the p-value is on the
        conservative side.  Candidates are the observed cells of the series at the steps ``t >= t_first`` with at least
        ``min_segment`` observed cells of that series before them and at least ``min_segment`` from them on: a shift over the
        whole record is the series' mean, not a break, and one over a handful of cells is an outlier patch.  Rows without
        candidates carry NaN (``time`` NaT)."""
        from pandas import DataFrame, NaT
        from scipy.stats import norm

        stat = {key: value.cpu().numpy() for key, value in self.get_level_shift_statistics(alpha).items()}
        cand = self._shift_candidates(t_first, min_segment)
        rows = []
        for r in range(self.R):
            for j in range(self.N):
                steps = np.nonzero(cand[r, :, j] & np.isfinite(stat["t"][r, :, j]))[0]
                if steps.size == 0:
                    rows.append((np.nan, NaT, np.nan, np.nan, 0, np.nan))
                    continue
                t = int(steps[np.argmax(np.abs(stat["t"][r, steps, j]))])
                tmax, m = float(abs(stat["t"][r, t, j])), int(steps.size)
                rows.append((tmax, self.batch.index[r][t], float(stat["estimate"][r, t, j]), float(stat["stderr"][r, t, j]), m,
                             -np.expm1(m * np.log1p(-2.0 * norm.cdf(-tmax)))))
        return DataFrame(rows, columns=["max_abs_t", "time", "estimate", "stderr", "ncand", "pvalue"],
                         index=self._rows(lambda r: ((name,) for name in self.batch.names[r]), ["series"]))

    _INTERVENTION_COLUMNS = ("series", "kind", "start", "end", "n_obs", "estimate", "stderr", "t", "pvalue", "dropped")

    def detect_level_shifts(self, level=0.01, max_shifts=4, alpha=None, t_first=1, min_segment=10):
        """Find level shifts at unknown dates, one per model and round: the shifts found so far are estimated jointly
        (``fit_interventions``) and taken out of the records (``adjust_observations``), the adjusted records are scanned
        (``screen_level_shifts``' candidates), and per model the candidate with the largest |t| over all its series is added when
        its Sidak p-value over the model's total number of candidates is below ``level``.  Stops when no model adds a shift or
        after ``max_shifts`` (at most 16: the regression's limit) rounds.  Parameters are held fixed throughout.  Returns
        ``fit_interventions``' frame of the final set, estimated jointly on the records as they are (empty, with the same
        columns, if nothing was found).  The records are left unadjusted, bit for bit, also when a step raises; records that are
        already adjusted when it is called are refused (ValueError): revert them first."""
        from pandas import DataFrame, MultiIndex
        from scipy.stats import norm

        max_shifts = int(max_shifts)
        if not 1 <= max_shifts <= 16:
            raise ValueError("max_shifts must be in 1..16 (the regression takes 16 effects per model)")
        if not 0 < float(level) < 1:
            raise ValueError("level must be between 0 and 1")
        if self.kf.observations_adjusted:
            raise ValueError("the records are adjusted: call unadjust_observations first (detect_level_shifts adjusts and reverts them itself)")
        found = [[] for _ in range(self.R)]            # per model (series, step) in the order found
        effects = lambda: [(r + self.shard[0], self.batch.names[r][j], "level", int(t)) for r in range(self.R) for j, t in found[r]]  # noqa: E731
        try:
            for _ in range(max_shifts):
                self.unadjust_observations()
                if any(found):
                    self.adjust_observations(self.fit_interventions(effects(), alpha=alpha, t_first=t_first))
                tstat = np.abs(self.get_level_shift_statistics(alpha, standardized=True)["t"].cpu().numpy())
                cand = self._shift_candidates(t_first, min_segment) & np.isfinite(tstat)
                added = False
                for r in range(self.R):
                    for j, t in found[r]:
                        cand[r, t, j] = False           # a date already in the model's list is no candidate
                    m = int(cand[r].sum())
                    if m == 0:
                        continue
                    t, j = np.unravel_index(int(np.argmax(np.where(cand[r], tstat[r], -1.0))), tstat[r].shape)
                    if -np.expm1(m * np.log1p(-2.0 * norm.cdf(-float(tstat[r, t, j])))) < float(level):
                        found[r].append((int(j), int(t)))
                        added = True
                if not added:
                    break
        finally:
            self.unadjust_observations()
        if not any(found):
            return DataFrame(columns=list(self._INTERVENTION_COLUMNS), index=MultiIndex.from_tuples([], names=["model", "effect"]))
        return self.fit_interventions(effects(), alpha=alpha, t_first=t_first)

    # ------------------------------------------------------------------ posterior draws (simulation smoother)
    # The draws and their window statistics go to the engine like the cached kinds (``_launch``) but are not kept: an ensemble is
    # the size of the thing it summarises.
    def _draws(self, what, ndraws, seed, alpha, antithetic):
        # a model's instance number is its place among ALL models, so its draws do not depend on the number of ranks
        out, _ = self._launch("draws of %s" % what, alpha, True, lambda phi, q: self.kf.draw_smoothed(
            phi, q, ndraws, seed=seed, what=what, antithetic=antithetic, first_instance=self.shard[0]))
        return out["draws"]

    def get_simulation_draws(self, ndraws, seed=0, alpha=None, standardized=False, antithetic=False):
        """``ndraws`` joint realisations of every series given the data, tensor ``[S,R,T,N]``: what ``get_simulated_means`` /
        ``_variances`` are the pointwise mean and variance of -- but a draw is a whole path, so the uncertainty of a monthly
        mean, of a yearly minimum or of the time spent below a threshold is read off the ensemble (simulation smoother,
        Durbin & Koopman 2002; ``BatchedKalman.draw_smoothed``).  Where a series is observed a draw equals the observation.
        Draw ``s`` of a model is fixed by ``seed``: asking for more draws extends the ensemble, it does not change it."""
        return self._units(self._draws("series", ndraws, seed, alpha, antithetic), None, standardized)[0]  # the draws: original units

    def get_state_draws(self, ndraws, seed=0, alpha=None, antithetic=False):
        """``ndraws`` joint realisations of the states given the data, tensor ``[S,R,T,N+K]`` (``get_state_means`` is their
        pointwise mean)."""
        return self._draws("states", ndraws, seed, alpha, antithetic)

    def get_simulation_draw(self, r, name, ndraws, seed=0, alpha=None, standardized=False, antithetic=False):
        """Draws of series ``name`` of model ``r``: DataFrame on the model's index, one column ``draw<s>`` per draw."""
        from pandas import DataFrame

        j = self._series(r, name)
        draws = self.get_simulation_draws(ndraws, seed, alpha, standardized, antithetic)
        L = int(self.batch.lengths[r])
        return DataFrame(draws[:, r, :L, j].transpose(0, 1).cpu().numpy(), index=self.batch.index[r],
                         columns=["draw%d" % s for s in range(int(ndraws))])

    # ------------------------------------------------------------------ window statistics of the draws
    def _thresholds(self, thresholds):
        """``thresholds`` of ``get_window_statistics`` as ``[R,N]`` in original units (NaN = no level), or None."""
        if thresholds is None:
            return None
        if isinstance(thresholds, dict):
            return np.array([[float(thresholds.get(name, np.nan)) for name in self.batch.names[r]] for r in range(self.R)])
        thresholds = np.asarray(thresholds, dtype=np.float64)
        if thresholds.ndim == 0:
            return np.full((self.R, self.N), float(thresholds))
        if thresholds.shape != (self.R, self.N):
            raise ValueError("thresholds must be a scalar, a dict name -> level or an array [%d,%d]" % (self.R, self.N))
        return thresholds

    def get_window_statistics(self, windows, thresholds=None, ndraws=200, probs=(0.025, 0.5, 0.975), seed=0, alpha=None,
                              antithetic=False):
        """What the ensemble of ``get_simulation_draws`` is read for, without holding it: per model, series and time window the
        posterior distribution of the window's ``mean``, ``min``, ``max``, ``fraction_below`` (the share of its steps below the
        series' level) and ``longest_spell`` (the longest run of consecutive steps below it, in steps), summarised over
        ``ndraws`` draws -- reduced on the device (``BatchedKalman.draw_window_statistics``), same draws as
        ``get_simulation_draws(ndraws, seed)``, original units.  ``windows``: a pandas offset alias (``"MS"``, ``"YS"``, ``"W"``,
        ...) or a list of ``(start, stop)`` timestamps, sorted and not overlapping; step t of a model is in a window when
        ``start <= index[t] < stop`` on the model's own index (``metran_amd.windows.step_windows``).  ``thresholds``: a scalar, a
        dict series name -> level, or an array ``[R,N]``; without a level the last two functionals are NaN.  Returns a DataFrame:
        rows (model, series, window start), columns (functional, statistic) with the statistics ``count`` (draws used),
        ``mean``, ``sd``, ``min``, ``max`` and one ``q<p>`` per probability; a window without a step of the model has count 0."""
        from pandas import DataFrame, MultiIndex

        from .windows import step_windows

        steps, starts = step_windows(self.batch.index, windows, self.T)
        probs = np.asarray(probs, dtype=np.float64).reshape(-1)
        # a model's instance number is its place among ALL models, so its statistics do not depend on the number of ranks
        out, _ = self._launch("window statistics", alpha, True, lambda phi, q: self.kf.draw_window_statistics(
            phi, q, ndraws, steps, thresholds=self._thresholds(thresholds), probs=probs, seed=seed, antithetic=antithetic,
            first_instance=self.shard[0]))
        summary = out["summary"].cpu().numpy()   # [R,N,W,5,5+P]
        functionals = ("mean", "min", "max", "fraction_below", "longest_spell")
        statistics = ["count", "mean", "sd", "min", "max"] + ["q%g" % p for p in probs]
        values = [summary[r, :, : len(starts[r])].reshape(-1, len(functionals) * len(statistics)) for r in range(self.R)]
        return DataFrame(np.concatenate(values, axis=0),
                         index=self._rows(lambda r: ((name, start) for name in self.batch.names[r] for start in starts[r]), ["series", "window"]),
                         columns=MultiIndex.from_product([functionals, statistics], names=["functional", "statistic"]))

    def get_window_statistic(self, r, name, windows, thresholds=None, ndraws=200, probs=(0.025, 0.5, 0.975), seed=0, alpha=None,
                             antithetic=False):
        """The rows of ``get_window_statistics`` for series ``name`` of model ``r``: DataFrame indexed by window start."""
        self._series(r, name)
        frame = self.get_window_statistics(windows, thresholds, ndraws, probs, seed, alpha, antithetic)
        return frame.loc[(r + self.shard[0], name)]

    # ------------------------------------------------------------------ exact window means, changes and contrasts
    def _contrast_table(self, contrasts):
        """``contrasts`` of ``get_window_means`` / ``get_changes`` -> (labels per model, the engine's table as nested tuples
        [R][C][N] or None for the unit contrasts).  A dict ``label -> {series name: weight}`` is applied to every model that has
        all of the label's series; the models with fewer labels are padded with all-zero contrasts."""
        if contrasts is None:
            return [list(self.batch.names[r]) for r in range(self.R)], None
        if not isinstance(contrasts, dict) or not contrasts:
            raise ValueError("contrasts must be None or a non-empty dict label -> {series name: weight}")
        labels, rows = [], []
        for r in range(self.R):
            names = list(self.batch.names[r])
            mine, table = [], []
            for label, weights in contrasts.items():
                if not weights or not all(name in names for name in weights):
                    continue
                row = [0.0] * self.N
                for name, weight in weights.items():
                    row[names.index(name)] += float(weight)
                mine.append(label)
                table.append(tuple(row))
            labels.append(mine)
            rows.append(table)
        C = max(len(t) for t in rows)
        if C < 1:
            raise KeyError("no model has the series of any contrast")
        return labels, tuple(tuple(t + [(0.0,) * self.N] * (C - len(t))) for t in rows)

    def get_window_means(self, windows, contrasts=None, alpha=None, standardized=False):
        """The EXACT posterior mean and standard deviation of the mean of the smoothed signal over time windows
        (``BatchedKalman.functionals``): one smoothing pass and the smoother's covariance across time, where
        ``get_window_statistics`` needs an ensemble of draws for an sd that is right to 1/sqrt(2 ndraws).  ``windows`` as in
        ``get_window_statistics`` (``metran_amd.windows.step_windows``), except that explicit ``(start, stop)`` pairs may overlap
        and come in any order.  ``contrasts``: None = every series, or a dict ``label -> {series name: weight}`` -- the head
        difference of two wells ``{"gradient": {"w1": 1, "w2": -1}}``, the mean of a group -- applied to every model that has
        those series.  It is the signal ``Z x`` whose mean is taken, as in ``get_simulated_means``: no observation variance is
        added.  Returns a DataFrame: rows (model, series or label, window start), columns ``mean`` and ``sd`` in original units
        (``standardized=True``: the units the filter runs in); a window without a step of the model is NaN."""
        from pandas import DataFrame

        from .windows import step_windows

        steps, starts = step_windows(self.batch.index, windows, self.T, overlap=True)
        labels, table = self._contrast_table(contrasts)
        request = (tuple(tuple((int(a), int(b), 0, 0) for a, b in model) for model in steps), table, bool(standardized))
        out = self._run("functionals", alpha, request)
        mean, sd = out["mean"].cpu().numpy(), np.sqrt(out["var"].cpu().numpy())      # [R,W,C]
        values = [np.stack([mean[r, : len(starts[r]), : len(labels[r])].T.reshape(-1), sd[r, : len(starts[r]), : len(labels[r])].T.reshape(-1)],
                           axis=1) for r in range(self.R)]
        return DataFrame(np.concatenate(values, axis=0),
                         index=self._rows(lambda r: ((label, start) for label in labels[r] for start in starts[r]), ["series", "window"]),
                         columns=["mean", "sd"])

    def get_window_mean(self, r, name, windows, alpha=None, standardized=False):
        """The rows of ``get_window_means`` for series ``name`` of model ``r``: DataFrame indexed by window start."""
        self._series(r, name)
        return self.get_window_means(windows, None, alpha, standardized).loc[(r + self.shard[0], name)]

    def get_changes(self, period_a, period_b, contrasts=None, alpha=None, standardized=False):
        """The change between two periods with its exact standard error: per model and series (or contrast label) the mean of the
        smoothed signal over ``period_a`` minus its mean over ``period_b`` -- each a ``(start, stop)`` pair of timestamps, half
        open, disjoint, in either order -- with the covariance between the two periods' steps taken from the smoother's
        covariance across time.  Returns a DataFrame with one row per (model, series or label): ``estimate``, ``sd``, ``z`` =
        estimate / sd and the two-sided normal ``pvalue``; NaN for a model without a step in one of the periods."""
        from pandas import DataFrame
        from scipy.stats import norm

        from .windows import step_windows

        sa, _ = step_windows(self.batch.index, [tuple(period_a)], self.T, overlap=True)
        sb, _ = step_windows(self.batch.index, [tuple(period_b)], self.T, overlap=True)
        rows = []
        for (a0, a1), (b0, b1) in zip(sa[:, 0], sb[:, 0]):
            if a0 < a1 and b0 < b1 and max(a0, b0) < min(a1, b1):
                raise ValueError("period_a and period_b must not overlap")
            rows.append(((int(a0), int(a1), int(b0), int(b1)) if b0 < b1 else (self.T, self.T, 0, 0),))   # a period without a step: NaN
        labels, table = self._contrast_table(contrasts)
        out = self._run("functionals", alpha, (tuple(rows), table, bool(standardized)))
        est, var = out["mean"].cpu().numpy()[:, 0], out["var"].cpu().numpy()[:, 0]   # [R,C]
        est = np.concatenate([est[r, : len(labels[r])] for r in range(self.R)])
        sd = np.sqrt(np.concatenate([var[r, : len(labels[r])] for r in range(self.R)]))
        with np.errstate(divide="ignore", invalid="ignore"):
            z = est / sd
        return DataFrame({"estimate": est, "sd": sd, "z": z, "pvalue": 2.0 * norm.sf(np.abs(z))},
                         index=self._rows(lambda r: ((label,) for label in labels[r]), ["series"]))

    # ------------------------------------------------------------------ one series' simulation and its decomposition
    def get_simulation(self, r, name, alpha=None, ci=0.05, standardized=False, method="smoother"):
        """``Metran.get_simulation`` (metran.py:831-883) for series ``name`` of model ``r``: DataFrame with
        ``mean`` (and ``lower``/``upper`` of the 1-ci interval; ``ci=None`` returns the mean Series)."""
        j = self._series(r, name)
        return self._series_band(r, j, *self._simulate(alpha, standardized, method), ci)

    def decompose_simulation(self, r, name, alpha=None, standardized=False, method="smoother"):
        """``Metran.decompose_simulation`` (metran.py:885-942): DataFrame with the specific dynamic component
        ``sdf`` (carrying the series mean) and one column ``cdf<k>`` per common factor of series ``name``."""
        from pandas import DataFrame

        j = self._series(r, name)
        out = self._run(self._method(method), alpha)
        key = ("decomp", bool(standardized))
        if key not in out:
            states = out["S" if method == "smoother" else "F"]
            out[key] = self.kf.decompose(self._observation_matrix(standardized), states)
        sdf, cdf = out[key]
        L = int(self.batch.lengths[r])
        cols = {"sdf": sdf[r, :L, j].cpu().numpy() + (0.0 if standardized else float(self._mean[r, j]))}
        for k in range(int(self.nfactors[r])):
            cols["cdf%d" % (k + 1)] = cdf[r, k, :L, j].cpu().numpy()
        return DataFrame(cols, index=self.batch.index[r])

    # ------------------------------------------------------------------ states
    def _state_columns(self, r):
        return [str(n) + "_sdf" for n in self.batch.names[r]] + ["cdf%d" % (k + 1) for k in range(self.K)]

    def get_state_means(self, r, alpha=None, method="smoother"):
        """``Metran.get_state_means`` (metran.py:655-681) of model ``r``: DataFrame [T, N+K] with the reference's
        column names (``<series>_sdf`` ..., ``cdf1`` ...)."""
        from pandas import DataFrame

        out = self._run(self._method(method), alpha)
        L = int(self.batch.lengths[r])
        return DataFrame(out["S" if method == "smoother" else "F"][r, :L].cpu().numpy(), index=self.batch.index[r],
                         columns=self._state_columns(r))

    def get_state_variances(self, r, alpha=None, method="smoother"):
        """``Metran.get_state_variances`` (metran.py:683-711): the diagonals of the state covariances."""
        import torch
        from pandas import DataFrame

        out = self._run(self._method(method), alpha)
        L = int(self.batch.lengths[r])
        var = out["var"][r, :L] if method == "smoother" else torch.diagonal(out["Pf"][r, :L], dim1=1, dim2=2)
        return DataFrame(var.cpu().numpy(), index=self.batch.index[r], columns=self._state_columns(r))

    def get_state(self, r, i, alpha=None, ci=0.05, method="smoother"):
        """``Metran.get_state`` (metran.py:713-756): state ``i`` of model ``r`` with its 1-ci band."""
        self._check_state(i)
        mean = self.get_state_means(r, alpha, method).iloc[:, i]
        return self._band(mean, self.get_state_variances(r, alpha, method).iloc[:, i] if ci is not None else None, ci)

"""Test infrastructure: ``OracleEngine`` (tests/oracle_engine.py) with the slice of ``BatchedKalman`` that the intervention
accessors of ``MetranBatch`` touch -- ``regression`` answered by the numpy restatement (tests/regress_ref.py) in float64,
``adjust_observations`` / ``unadjust_observations`` and ``mask_observations`` / ``unmask_observations`` with the engine's own
bookkeeping of the kept originals, ``loglik`` by the C oracle on whatever records are current -- so that the host layer runs
without a GPU.  The product never sees it."""
import numpy as np
import torch

import regress_ref
from oracle_engine import OracleEngine


class RegressEngine(OracleEngine):
    status_bits = 0
    shift_records = 0   # WRONG on purpose when not 0: instance b answers with the effects of record (b + shift) % R

    def __init__(self, obs=None, loadings=None, adjoint=True, log=None):
        super().__init__(obs, loadings, adjoint, log)
        self.calls = 0
        self._unmasked = self._unadjusted = None

    @property
    def obs(self):
        return torch.from_numpy(self.obs_np)

    def _table(self, effects):
        ef = np.asarray(effects, dtype=np.int64)
        if ef.ndim == 2:
            ef = np.broadcast_to(ef, (self.R,) + ef.shape)
        if ef.ndim != 3 or ef.shape[0] != self.R or not 1 <= ef.shape[1] <= 16 or ef.shape[2] != 4:
            raise ValueError("effects must be [%d,M,4] (or [M,4]) integers (series, kind, t0, t1), 1 <= M <= 16" % self.R)
        return ef

    def regression(self, phi, q, effects, t_first=1, x0=None, P0=None, buffers=None):
        if int(t_first) < 0:
            raise ValueError("t_first must be >= 0")
        ef = self._table(effects)
        self.calls += 1
        phi, q = self._dev(phi).numpy(), self._dev(q).numpy()
        B = phi.shape[0]
        rows = [regress_ref.regression(self.obs_np[r], phi[i], q[i], self.load_np[r], None, None if x0 is None else np.asarray(x0)[i],
                                       None if P0 is None else np.asarray(P0)[i], ef[(r + self.shift_records) % self.R], int(t_first),
                                       dtype=np.float64) for i, r in enumerate(self._records(B))]
        out = {k: torch.from_numpy(np.stack([np.asarray(row[k], dtype=np.float64) for row in rows])) for k in ("beta", "cov", "gain", "normal")}
        out["support"] = torch.from_numpy(np.stack([row["support"] for row in rows]))
        out["dropped"] = torch.tensor([sum(1 << m for m, gone in enumerate(row["dropped"]) if gone) for row in rows], dtype=torch.int32)
        out["status"] = torch.full((B,), self.status_bits, dtype=torch.int32)
        return out

    def mask_observations(self, mask):
        base = self._unmasked if self._unmasked is not None else self.obs_np
        self._unmasked, self.obs_np = base, np.where(np.asarray(mask) != 0, np.nan, base)
        return self

    def unmask_observations(self):
        if self._unmasked is not None:
            self.obs_np, self._unmasked = self._unmasked, None
        return self

    def adjust_observations(self, effects, beta):
        ef = self._table(effects)
        beta = np.asarray(beta, dtype=np.float64)
        base, base_unmasked = self._unadjusted if self._unadjusted is not None else (self.obs_np, self._unmasked)
        adjusted = lambda a: None if a is None else np.stack([regress_ref.adjusted(a[r], ef[r], beta[r]) for r in range(self.R)])  # noqa: E731
        self._unadjusted = (base, base_unmasked)
        self.obs_np, self._unmasked = adjusted(base), adjusted(base_unmasked)
        return self

    def unadjust_observations(self):
        if self._unadjusted is not None:
            (self.obs_np, self._unmasked), self._unadjusted = self._unadjusted, None
        return self

"""Test infrastructure: ``OracleEngine`` (tests/oracle_engine.py) with the slice of ``BatchedKalman`` that the score accessors of
``MetranBatch`` touch -- ``scores`` and ``scores_alpha`` answered by the numpy restatement (tests/score_ref.py) in float64, the
Hessian's gradients by the adjoint restatement the base class already has -- so that the host layer runs without a GPU.  The
product never sees it."""
import numpy as np
import torch

import score_ref
from oracle_engine import OracleEngine


class ScoreEngine(OracleEngine):
    status_bits = 0
    shift_records = 0   # WRONG on purpose when not 0: instance b answers from the record (b + shift) % R

    def __init__(self, obs=None, loadings=None, adjoint=True, log=None):
        super().__init__(obs, loadings, adjoint, log)
        self.calls = 0

    @property
    def obs(self):
        return torch.from_numpy(self.obs_np)

    def scores(self, phi, q, dphi, dq, t_first=1, x0=None, P0=None, buffers=None):
        if int(t_first) < 0:
            raise ValueError("t_first must be >= 0")
        self.calls += 1
        phi, q, dphi, dq = (self._dev(a).numpy() for a in (phi, q, dphi, dq))
        B = phi.shape[0]
        rows = []
        for i, r in enumerate(self._records(B)):
            r = (r + self.shift_records) % self.R
            rows.append(score_ref.scores(self.obs_np[r], phi[i], q[i], self.load_np[r], None, None if x0 is None else np.asarray(x0)[i],
                                         None if P0 is None else np.asarray(P0)[i], dphi=dphi[i], dq=dq[i], t_first=int(t_first),
                                         dtype=np.float64))
        out = {k: torch.from_numpy(np.stack([np.asarray(row[k], dtype=np.float64) for row in rows])) for k in score_ref.OUTPUTS}
        out["count"] = torch.tensor([row["count"] for row in rows], dtype=torch.int64)
        out["status"] = torch.full((B,), self.status_bits, dtype=torch.int32)
        return out

    def scores_alpha(self, alpha, dt=1.0, t_first=1):
        alpha = self._dev(alpha)
        phi, q = self.params_from_alpha(alpha, dt)
        rec = self._records(alpha.shape[0])
        c = np.concatenate([1.0 - np.sum(self.load_np ** 2, axis=2), np.ones((self.R, self.K))], axis=1)[rec]
        dphi = phi * float(dt) / (alpha * alpha)
        dq = -2.0 * phi * dphi * torch.from_numpy(c)
        return self.scores(phi, q, dphi, dq, t_first=t_first)

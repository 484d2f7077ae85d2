"""Test infrastructure: the slice of ``BatchedKalman`` that the residual diagnostics of ``MetranBatch`` touch (``innovations``,
``innovation_stats``, ``residual_series``, ``residual_cross``) on the CPU, answered by the numpy restatements (tests/innov_ref.py,
tests/resid_ref.py).  ``cells``: ``(v, f)`` ``[R,T,N]`` to hand out INSTEAD of the filter's innovations, so that a test can put
known residuals behind the facade.  ``log`` counts the calls."""
import numpy as np
import torch

import innov_ref
import resid_ref
from oracle_engine import OracleEngine


class ResidEngine(OracleEngine):
    def __init__(self, obs=None, loadings=None, adjoint=True, log=None, cells=None):
        super().__init__(obs, loadings, adjoint, log)
        self.scale = self.offset = None
        self.cells = cells

    def set_scaling(self, scale=None, offset=None):
        self.scale = None if scale is None else np.asarray(scale, float)
        self.offset = None if offset is None else np.asarray(offset, float)
        return self

    def innovations(self, phi, q):
        phi, q = self._dev(phi).numpy(), self._dev(q).numpy()
        B = phi.shape[0]
        self.log.append(("innovations", B))
        rows = [innov_ref.innovations(self.obs_np[r], phi[i], q[i], self.load_np[r], None, None, None,
                                      None if self.scale is None else self.scale[r], None if self.offset is None else self.offset[r])
                for i, r in enumerate(self._records(B))]
        out = {k: torch.from_numpy(np.stack([row[k].astype(np.float64) for row in rows])) for k in ("v", "f", "pred_mean", "pred_var")}
        if self.cells is not None:
            out["v"], out["f"] = torch.from_numpy(np.array(self.cells[0], float)), torch.from_numpy(np.array(self.cells[1], float))
        out["status"] = torch.zeros(B, dtype=torch.int32)
        return out

    def innovation_stats(self, v, f, nlags=10, t_first=0):
        self.log.append(("innovation_stats", int(v.shape[0])))
        return torch.from_numpy(np.stack([innov_ref.stats(v[b].numpy(), f[b].numpy(), nlags, t_first).astype(np.float64)
                                          for b in range(v.shape[0])]))

    def residual_series(self, v, f, t_first=0):
        self.log.append(("residual_series", int(v.shape[0])))
        return torch.from_numpy(np.stack([resid_ref.series(v[b].numpy(), f[b].numpy(), t_first).astype(np.float64)
                                          for b in range(v.shape[0])]))

    def residual_cross(self, v, f, stats, nlags=10, t_first=0):
        self.log.append(("residual_cross", int(v.shape[0])))
        rows = [resid_ref.cross(v[b].numpy(), f[b].numpy(), nlags, t_first) for b in range(v.shape[0])]
        return (torch.from_numpy(np.stack([c for c, _ in rows])), torch.from_numpy(np.stack([s.astype(np.float64) for _, s in rows])))

"""Test infrastructure: ``OracleEngine`` (tests/oracle_engine.py) with the slice of ``BatchedKalman`` that the window-mean accessors
of ``MetranBatch`` touch -- ``set_scaling`` and ``functionals``, answered by the float64 recursion of tests/functional_ref.py from
the C oracle's records -- so that the host layer runs without a GPU.  The product never sees it."""
import numpy as np
import torch

import call_forms as cf
import functional_ref as fr
from oracle_engine import OracleEngine


class FunctionalEngine(OracleEngine):
    status_bits = 0

    def __init__(self, obs=None, loadings=None, adjoint=True, log=None):
        super().__init__(obs, loadings, adjoint, log)
        self.calls = 0
        self.scale = self.offset = None
        self.scalings = []          # what was set when ``functionals`` ran: "none" or "set"

    def set_scaling(self, scale=None, offset=None):
        self.scale = None if scale is None else np.asarray(scale, dtype=np.float64)
        self.offset = None if offset is None else np.asarray(offset, dtype=np.float64)
        return self

    def functionals(self, phi, q, windows, contrasts=None, x0=None, P0=None, buffers=None):
        wn = np.asarray(windows, dtype=np.int64)
        if wn.ndim == 2:
            wn = np.broadcast_to(wn, (self.R,) + wn.shape)
        if wn.ndim != 3 or wn.shape[0] != self.R or wn.shape[1] < 1 or wn.shape[2] != 4:
            raise ValueError("windows must be [%d,W,4] (or [W,4]) integers (t0, t1, t2, t3), W >= 1" % self.R)
        table = None
        if contrasts is not None:
            table = np.asarray(contrasts, dtype=np.float64)
            if table.ndim == 2:
                table = np.broadcast_to(table, (self.R,) + table.shape)
            if table.ndim != 3 or table.shape[0] != self.R or not 1 <= table.shape[1] <= 64 or table.shape[2] != self.N:
                raise ValueError("contrasts must be [%d,C,%d] (or [C,%d]) weights of the series" % (self.R, self.N, self.N))
        self.calls += 1
        self.scalings.append("none" if self.scale is None else "set")
        phi, q = self._dev(phi).numpy(), self._dev(q).numpy()
        B = phi.shape[0]
        assert B % self.R == 0
        g = cf.variant(dict(N=self.N, K=self.K, T=self.T, R=self.R, B=B, obs=self.obs_np, loadings=self.load_np, obsvar=None, scale=self.scale,
                            offset=self.offset, phi=phi, q=q, x0=None if x0 is None else np.asarray(x0), P0=None if P0 is None else np.asarray(P0)))
        C = self.N if table is None else table.shape[1]
        mean, var = np.empty((B, wn.shape[1], C)), np.empty((B, wn.shape[1], C))
        for i in range(B):
            rows = fr.contrast_rows(g, i, table)
            for w, win in enumerate(wn[i % self.R]):
                for k, c in enumerate(rows):
                    mean[i, w, k], var[i, w, k] = fr.functional_walk(g, i, win, c)
        return {"mean": torch.from_numpy(mean), "var": torch.from_numpy(var), "status": torch.full((B,), self.status_bits, dtype=torch.int32)}

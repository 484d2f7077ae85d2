"""Test infrastructure: ``OracleEngine`` (tests/oracle_engine.py) with the slice of ``BatchedKalman`` that the gap accessors of
``MetranBatch`` touch -- ``block_predict`` answered by the numpy restatement of the kernels' recursion (tests/block_ref.py) in
float64, ``loo_predict`` by the leave-one-out restatement (tests/loo_ref.py), ``set_scaling`` and ``subset`` -- so that the host
layer runs without a GPU.  The product never sees it."""
import numpy as np
import torch

import block_ref
import loo_ref
from oracle_engine import OracleEngine


class BlockEngine(OracleEngine):
    block_max_cells = block_ref.MAX_CELLS
    obsvar = None

    def __init__(self, obs=None, loadings=None, adjoint=True, log=None):
        super().__init__(obs, loadings, adjoint, log)
        self.scale = self.offset = None
        self.calls = []                 # (what, instances, blocks per record) of every call

    @property
    def obs(self):
        return torch.from_numpy(self.obs_np)

    def set_scaling(self, scale, offset):
        self.scale = None if scale is None else np.asarray(scale, dtype=np.float64)
        self.offset = None if offset is None else np.asarray(offset, dtype=np.float64)
        return self

    def subset(self, index):
        idx = np.asarray(index)
        sub = BlockEngine(self.obs_np[idx], self.load_np[idx], self._adjoint, self.log)
        sub.calls = self.calls
        if self.scale is not None:
            sub.set_scaling(self.scale[idx], self.offset[idx])
        return sub

    def _reader_stride(self, name, refuse=False):
        n = self.n
        return n * (n + 1) + self.N * ((n + 3) & ~1) + self.N

    def _group(self, phi, q, x0=None, P0=None):
        phi, q = self._dev(phi).numpy(), self._dev(q).numpy()
        B = phi.shape[0]
        assert B % self.R == 0
        return dict(N=self.N, K=self.K, T=self.T, R=self.R, S=B // self.R, B=B, obs=self.obs_np, loadings=self.load_np, obsvar=None,
                    scale=self.scale, offset=self.offset, phi=phi, q=q, x0=x0, P0=P0, _cache={})

    def block_predict(self, phi, q, blocks, x0=None, P0=None, buffers=None):
        bl = np.asarray(blocks, dtype=np.int64)
        if bl.ndim == 2:
            bl = np.broadcast_to(bl, (self.R,) + bl.shape)
        if bl.ndim != 3 or bl.shape[0] != self.R or bl.shape[1] < 1 or bl.shape[2] != 3:
            raise ValueError("blocks must be [%d,W,3] (or [W,3]) integers (series, t0, t1), W >= 1" % self.R)
        used = bl[..., 0] >= 0
        length = int(((bl[..., 2] - bl[..., 1]) * used).max()) if used.any() else 1
        if length > self.block_max_cells:
            raise ValueError("blocks: a block of %d steps is longer than the limit of %d" % (length, self.block_max_cells))
        L = max(length, 1)
        g = self._group(phi, q, x0, P0)
        B, W = g["B"], bl.shape[1]
        self.calls.append(("block_predict", B, W))
        means, variances = np.full((B, W, L), np.nan), np.full((B, W, L), np.nan)
        summary, flags = np.full((B, W, 4), np.nan), np.zeros((B, W), dtype=np.int32)
        for i in range(B):
            for w, blk in enumerate(bl[i % self.R]):
                row = block_ref.recursion(g, i, blk)
                if row is None:
                    continue
                k = len(row["means"])
                summary[i, w, 0] = row["m"]
                if row.get("degenerate"):
                    flags[i, w] = 1
                    continue
                means[i, w, :k], variances[i, w, :k] = row["means"], row["vars"]
                summary[i, w, 1:] = row["quad"], row["logdet"], row["ovo"]
        out = {"means": means, "vars": variances, "summary": summary}
        out = {k: torch.from_numpy(v) for k, v in out.items()}
        out["flags"] = torch.from_numpy(flags)
        out["status"] = torch.zeros(B, dtype=torch.int32)
        return out

    def loo_predict(self, phi, q, x0=None, P0=None, buffers=None):
        phi, q = self._dev(phi).numpy(), self._dev(q).numpy()
        B = phi.shape[0]
        self.calls.append(("loo_predict", B, 0))
        means, variances = np.empty((B, self.T, self.N)), np.empty((B, self.T, self.N))
        for i, r in enumerate(self._records(B)):
            m, v = loo_ref.loo_tape(self.obs_np[r], phi[i], q[i], self.load_np[r], None, None, None)
            scale = np.ones(self.N) if self.scale is None else self.scale[r]
            offset = np.zeros(self.N) if self.offset is None else self.offset[r]
            means[i], variances[i] = m * scale + offset, np.maximum(v, 0.0) * scale ** 2
        return {"loo_means": torch.from_numpy(means), "loo_vars": torch.from_numpy(variances), "status": torch.zeros(B, dtype=torch.int32)}

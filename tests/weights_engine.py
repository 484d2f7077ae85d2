"""Test infrastructure: ``OracleEngine`` (tests/oracle_engine.py) with the slice of ``BatchedKalman`` that the observation-weight
accessors of ``MetranBatch`` touch -- ``set_scaling``, ``obs``, ``observation_weights`` answered by the numpy restatement
(tests/weights_ref.py) in float64, and ``simulate_smoothed`` answered by the C oracle's filter, smoother and projection (what
``get_simulation`` reads, for the reconstruction identity) -- so that the host layer runs without a GPU.  The product never sees
it."""
import numpy as np
import torch

import oracle
import weights_ref
from oracle_engine import OracleEngine


def oracle_simulation(y, phi, q, G, R=None, x0=None, P0=None, scale=None, offset=None):
    """(means, variances) [T,N] of the projected smoothed states of one model through the oracle's own ``seqkalmanfilter``,
    ``kalmansmoother`` and ``simulate``, Z = diag(scale) [I | G], plus ``offset``."""
    y = np.asarray(y, float)
    T, N = y.shape
    K = G.shape[1]
    n = N + K
    Z = np.concatenate([np.eye(N), np.asarray(G, float)], axis=1)
    ob, oi, oc = oracle.set_observations(y)
    ph = np.asarray(phi, float)
    _, _, _, F, Pf, Xp, Pp = oracle.seqkalmanfilter(ob, np.diag(ph), np.diag(np.asarray(q, float)), Z, np.zeros(N) if R is None else np.asarray(R, float),
                                                    oi, oc, np.zeros(n) if x0 is None else np.asarray(x0, float),
                                                    np.eye(n) if P0 is None else np.asarray(P0, float))
    S, Ps = oracle.kalmansmoother(F, Pf, Xp, Pp, np.diag(ph))
    sm, sv = oracle.simulate(Z if scale is None else Z * np.asarray(scale, float)[:, None], S, Ps)
    return (sm if offset is None else sm + np.asarray(offset, float)), sv


class WeightsEngine(OracleEngine):
    status_bits = 0
    shift_records = 0   # WRONG on purpose when not 0: instance b answers with the targets of record (b + shift) % R

    def __init__(self, obs=None, loadings=None, adjoint=True, log=None):
        super().__init__(obs, loadings, adjoint, log)
        self.calls = 0
        self.scale = self.offset = None
        self._parent = None

    def subset(self, index):
        """The records ``index`` alone; the calls of the subset are counted on this engine."""
        idx = np.asarray(index)
        sub = WeightsEngine(self.obs_np[idx], self.load_np[idx], self._adjoint, self.log)
        sub._parent = self._parent or self
        sub.shift_records = self.shift_records
        if self.scale is not None:
            sub.set_scaling(self.scale[idx], self.offset[idx])
        return sub

    @property
    def obs(self):
        return torch.from_numpy(self.obs_np)

    def set_scaling(self, scale=None, offset=None):
        self.scale = None if scale is None else np.asarray(scale, float)
        self.offset = None if offset is None else np.asarray(offset, float)
        return self

    def simulate_smoothed(self, phi, q, warmup=1, x0=None, P0=None, buffers=None):
        phi, q = self._dev(phi).numpy(), self._dev(q).numpy()
        B = phi.shape[0]
        rows = [oracle_simulation(self.obs_np[r], phi[i], q[i], self.load_np[r], None, None if x0 is None else np.asarray(x0)[i],
                                  None if P0 is None else np.asarray(P0)[i], None if self.scale is None else self.scale[r],
                                  None if self.offset is None else self.offset[r]) for i, r in enumerate(self._records(B))]
        return {"sim_means": torch.from_numpy(np.stack([m for m, _ in rows])), "sim_vars": torch.from_numpy(np.stack([v for _, v in rows])),
                "status": torch.full((B,), self.status_bits, dtype=torch.int32)}

    def observation_weights(self, phi, q, targets, what="series", x0=None, P0=None, buffers=None):
        if what not in ("series", "states"):
            raise ValueError("what must be 'series' or 'states'")
        tg = np.asarray(targets, dtype=np.int64)
        if tg.ndim == 2:
            tg = np.broadcast_to(tg, (self.R,) + tg.shape)
        if tg.ndim != 3 or tg.shape[0] != self.R or tg.shape[1] < 1 or tg.shape[2] != 2:
            raise ValueError("targets must be [%d,M,2] (or [M,2]) integers (step, column), M >= 1" % self.R)
        (self._parent or self).calls += 1
        phi, q = self._dev(phi).numpy(), self._dev(q).numpy()
        B = phi.shape[0]
        ws, ics = [], []
        for i, r in enumerate(self._records(B)):
            w, ic = weights_ref.weights(self.obs_np[r], phi[i], q[i], self.load_np[r], None, None if x0 is None else np.asarray(x0)[i],
                                        None if P0 is None else np.asarray(P0)[i], tg[(r + self.shift_records) % self.R], what,
                                        dtype=np.float64)
            ws.append(w)
            ics.append(ic)
        return {"weights": torch.from_numpy(np.stack(ws)), "intercept": torch.from_numpy(np.stack(ics)),
                "status": torch.full((B,), self.status_bits, dtype=torch.int32)}

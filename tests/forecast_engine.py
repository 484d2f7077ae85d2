"""Test infrastructure: ``OracleEngine`` (tests/oracle_engine.py) with the slice of ``BatchedKalman`` that the forecast
accessors of ``MetranBatch`` touch -- ``set_scaling``, ``obs`` and ``forecast``, answered by the numpy restatement
(tests/forecast_ref.py) in float64 -- so that the host layer runs without a GPU.  The product never sees it."""
import numpy as np
import torch

import forecast_ref
from oracle_engine import OracleEngine


class ForecastEngine(OracleEngine):
    status_bits = 0

    def __init__(self, obs=None, loadings=None, adjoint=True, log=None):
        super().__init__(obs, loadings, adjoint, log)
        self.calls = 0
        self.scale = self.offset = None

    @property
    def obs(self):
        return torch.from_numpy(self.obs_np)

    def set_scaling(self, scale=None, offset=None):
        self.scale = None if scale is None else np.asarray(scale, float)
        self.offset = None if offset is None else np.asarray(offset, float)
        return self

    def forecast(self, phi, q, x0=None, P0=None, horizon=14, outputs=("fan", "skill"), origins=None, track_horizon=1, t_first=1,
                 coverage=0.95, buffers=None):
        from scipy.stats import norm

        outputs = tuple(outputs)
        if not outputs or any(k not in ("fan", "track", "skill") for k in outputs):
            raise ValueError("outputs must be a non-empty subset of ('fan', 'track', 'skill')")
        if not 1 <= int(horizon) <= 32:
            raise ValueError("horizon must be in 1..32")
        self.calls += 1
        phi, q = self._dev(phi).numpy(), self._dev(q).numpy()
        B = phi.shape[0]
        z = float(norm.ppf(0.5 + 0.5 * coverage))
        rows = {}
        for i, r in enumerate(self._records(B)):
            f = forecast_ref.forecast(self.obs_np[r], phi[i], q[i], self.load_np[r], None, None if x0 is None else np.asarray(x0)[i],
                                      None if P0 is None else np.asarray(P0)[i], None if self.scale is None else self.scale[r],
                                      None if self.offset is None else self.offset[r], horizon=horizon,
                                      origin=None if origins is None else int(np.asarray(origins)[r]),
                                      track_horizon=track_horizon if "track" in outputs else 1, t_first=t_first, z=z, dtype=np.float64)
            for key in outputs:
                for name in ((key,) if key == "skill" else (key + "_mean", key + "_var")):
                    rows.setdefault(name, []).append(f[name])
        res = {k: torch.from_numpy(np.stack(v)) for k, v in rows.items()}
        res["status"] = torch.full((B,), self.status_bits, dtype=torch.int32)
        return res

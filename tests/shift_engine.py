"""Test infrastructure: ``BlockEngine`` (tests/block_engine.py) with the slice of ``BatchedKalman`` that the level-shift accessors
of ``MetranBatch`` touch -- ``level_shifts`` answered by the numpy restatement of the kernel's recursion (tests/shift_ref.py) in
float64; ``regression``, ``adjust_observations`` and ``unadjust_observations`` answered as the regression stand-in answers them
(tests/regress_engine.py: the same restatement, the same bookkeeping of the kept originals) -- so that the host layer runs
without a GPU.  The product never sees it."""
import numpy as np
import torch

import regress_ref
import shift_ref
from block_engine import BlockEngine
from regress_engine import RegressEngine


class ShiftEngine(BlockEngine):
    status_bits = 0
    shift_records = 0
    fail_regression_at = None       # the number of the ``regression`` call that raises (1 = the first), for the restore tests
    fail_scan_at = None             # ... and of the ``level_shifts`` call

    def __init__(self, obs=None, loadings=None, adjoint=True, log=None):
        super().__init__(obs, loadings, adjoint, log)
        self._unmasked = self._unadjusted = None
        self.regressions = self.scans = 0

    _table = RegressEngine._table
    adjust_observations = RegressEngine.adjust_observations
    unadjust_observations = RegressEngine.unadjust_observations

    @property
    def observations_adjusted(self):
        return self._unadjusted is not None

    def regression(self, phi, q, effects, t_first=1, x0=None, P0=None, buffers=None):
        ef = self._table(effects)
        self.regressions += 1
        if self.fail_regression_at == self.regressions:
            raise RuntimeError("regression call %d fails on purpose" % self.regressions)
        phi, q = self._dev(phi).numpy(), self._dev(q).numpy()
        B = phi.shape[0]
        self.calls.append(("regression", B, ef.shape[1]))
        rows = [regress_ref.regression(self.obs_np[r], phi[i], q[i], self.load_np[r], None, None, None, ef[r], int(t_first), dtype=np.float64)
                for i, r in enumerate(self._records(B))]
        out = {k: torch.from_numpy(np.stack([np.asarray(row[k], dtype=np.float64) for row in rows])) for k in ("beta", "cov", "gain", "normal")}
        out["support"] = torch.from_numpy(np.stack([row["support"] for row in rows]))
        out["dropped"] = torch.tensor([sum(1 << m for m, gone in enumerate(row["dropped"]) if gone) for row in rows], dtype=torch.int32)
        out["status"] = torch.zeros(B, dtype=torch.int32)
        return out

    def level_shifts(self, phi, q, x0=None, P0=None, buffers=None):
        self.scans += 1
        if self.fail_scan_at == self.scans:
            raise RuntimeError("level_shifts call %d fails on purpose" % self.scans)
        g = self._group(phi, q, x0, P0)
        B = g["B"]
        self.calls.append(("level_shifts", B, 0))
        rows = [shift_ref.recursion(g, i) for i in range(B)]
        return {"num": torch.from_numpy(np.stack([row["num"] for row in rows])), "den": torch.from_numpy(np.stack([row["den"] for row in rows])),
                "status": torch.zeros(B, dtype=torch.int32)}


def raw_facade(engine, models, loadings):
    """A ``MetranBatch`` of ``models`` over ``engine(records, loadings)`` that holds the records AS THEY ARE -- scale 1, offset 0,
    through the facade's construction seam (``MetranBatch._assemble``) -- for records simulated from a model with known
    parameters: the sample mean and standard deviation of a hundred strongly autocorrelated steps are far from 0 and 1 (0.5 to 2
    in tests/shift_ref.py's planted batch), and records standardised by them no longer follow the parameters they were drawn
    with.  ``engine`` may build the stand-in or a ``BatchedKalman``."""
    from metran_amd.batch import MetranBatch
    from metran_amd.ingest import ObservationBatch

    batch = ObservationBatch(models)
    kf = engine(np.array(batch.obs, dtype=np.float64), loadings)
    one = torch.ones(batch.obs.shape[0], batch.obs.shape[2], dtype=torch.float64, device=kf.device)
    return MetranBatch.__new__(MetranBatch)._assemble(batch, kf, one, torch.zeros_like(one), loadings)

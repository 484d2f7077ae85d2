"""Test infrastructure: a ``MetranBatch`` over a stand-in engine (the constructor itself needs a GPU), built through the facade's
own construction seam (``MetranBatch._assemble``), and the two-model data set the host tiers of the accessors share."""
import numpy as np
import pandas as pd
import torch


def two_models():
    """(models, loadings): 2 models x 3 series ``s0 .. s2`` x 1 factor on 40 days, about 30 % missing; every series of the
    second model is four observations shorter, so its record is padded."""
    rng = np.random.default_rng(4)
    idx = pd.date_range("2001-01-01", periods=40, freq="D")
    models = []
    for r in range(2):
        cols = []
        for j in range(3):
            s = pd.Series(10.0 * (j + 1) + (2.0 + j) * np.cumsum(rng.normal(size=40)) / 3.0, index=idx, name="s%d" % j)
            cols.append(s[rng.random(40) > 0.3])
        models.append(cols if r == 0 else [c.iloc[: len(c) - 4] for c in cols])
    G = np.broadcast_to(np.array([[0.6], [0.5], [-0.4]]), (2, 3, 1)).copy()
    return models, G


def stand_in(engine, models, loadings):
    """A MetranBatch of ``models`` whose engine is ``engine(standardised records, loadings)`` -- a subclass of
    ``oracle_engine.OracleEngine`` that answers the calls of the accessors under test."""
    from metran_amd.batch import MetranBatch
    from metran_amd.ingest import ObservationBatch

    batch = ObservationBatch(models)
    mean = np.nanmean(batch.obs, axis=1)
    std = np.nanstd(batch.obs, axis=1, ddof=1)
    kf = engine((batch.obs - mean[:, None]) / std[:, None], loadings)
    return MetranBatch.__new__(MetranBatch)._assemble(batch, kf, torch.from_numpy(std), torch.from_numpy(mean), loadings)

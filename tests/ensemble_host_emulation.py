"""Test infrastructure: the kernels of metran_amd/csrc/ensemble_kernels.hip compiled FOR THE HOST, unchanged, on the prelude of
tests/draw_host_emulation.py (a workgroup is 256 std::threads, ``__syncthreads`` a std::barrier, the dynamic LDS a NaN-filled
array per block, blocks run one after the other through the file's own launchers).  The CPU tier runs the kernels' walk over
the windows, their indexing in both layouts, the compaction, the sorting network and the barrier placement against the numpy
restatement (tests/ensemble_ref.py); compiled without fused multiply-adds, so the summary agrees to the bit here as well."""
import ctypes
import os
import subprocess

import numpy as np

from draw_host_emulation import CSRC, PRELUDE, ptr

ENTRY = r"""
extern "C" int run_path_functionals(long SB, long B, long R, long T, int Wd, int tm, long W, const double *paths, const int64_t *windows,
                                    const double *thresholds, double *out)
{
    mk::PathFunctionalArgs a;
    memset(&a, 0, sizeof(a));
    a.SB = SB; a.B = B; a.R = R; a.T = T; a.Wd = Wd; a.time_major = tm; a.W = W;
    a.paths = paths; a.windows = windows; a.thresholds = thresholds; a.out = out;
    return mk::launch_path_functionals(a, 0);
}
extern "C" int run_ensemble_summary(long S, long cells, int nprobs, const double *probs, const double *values, double *out)
{
    mk::EnsembleSummaryArgs a;
    memset(&a, 0, sizeof(a));
    a.S = S; a.cells = cells; a.nprobs = nprobs;
    for (int k = 0; k < nprobs; ++k) a.probs[k] = probs[k];
    a.values = values; a.out = out;
    return mk::launch_ensemble_summary(a, 0);
}
extern "C" int max_draws() { return mk::ensemble_max_draws; }
"""


def build(directory):
    """Compile the emulation into ``directory`` and return the bound library."""
    hdr = open(os.path.join(CSRC, "ensemble_kernels.h")).read()
    src = open(os.path.join(CSRC, "ensemble_kernels.hip")).read()
    hooks = ((hdr, "#include <hip/hip_runtime.h>"), (hdr, "#pragma once"), (src, '#include "ensemble_kernels.h"'),
             (src, "extern __shared__ double lds[];"))
    for text, old in hooks:
        assert old in text, "ensemble_kernels: %r is gone -- the emulation's one textual hook" % old
    hdr = hdr.replace("#include <hip/hip_runtime.h>", "").replace("#pragma once", "")
    src = src.replace('#include "ensemble_kernels.h"', "").replace("extern __shared__ double lds[];", "double *lds = g_lds;")
    cpp = os.path.join(str(directory), "ensemble_kernels_host.cpp")
    lib = os.path.join(str(directory), "libensemble_kernels_host.so")
    open(cpp, "w").write(PRELUDE + hdr + src + ENTRY)
    # no fused multiply-add: the restatement is plain numpy
    subprocess.check_call(["g++", "-O1", "-std=c++20", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", cpp, "-o", lib])
    L = ctypes.CDLL(lib)
    vp, lg, it = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
    L.run_path_functionals.argtypes = [lg, lg, lg, lg, it, it, lg, vp, vp, vp, vp]
    L.run_ensemble_summary.argtypes = [lg, lg, it, vp, vp, vp]
    return L


def path_functionals(L, paths, windows, thresholds, time_major):
    """The kernel on ``paths [S,B,T,Wd]`` stored in the asked layout -> ``[S,B,Wd,W,5]`` (NaN-poisoned before the launch)."""
    S, B, T, Wd = paths.shape
    windows = np.ascontiguousarray(windows, dtype=np.int64)
    R, W = windows.shape[:2]
    flat = paths.reshape(S * B, T, Wd)
    stored = np.ascontiguousarray(flat.transpose(1, 0, 2) if time_major else flat)
    thr = None if thresholds is None else np.ascontiguousarray(thresholds, dtype=np.float64)
    out = np.full((S, B, Wd, W, 5), -777.0)
    assert L.run_path_functionals(S * B, B, R, T, Wd, int(time_major), W, ptr(stored), ptr(windows), ptr(thr), ptr(out)) == 0
    return out


def ensemble_summary(L, values, probs):
    values = np.ascontiguousarray(values, dtype=np.float64)
    probs = np.ascontiguousarray(probs, dtype=np.float64)
    S, cells = values.shape
    out = np.full((cells, 5 + probs.size), -777.0)
    assert L.run_ensemble_summary(S, cells, probs.size, ptr(probs), ptr(values), ptr(out)) == 0
    return out

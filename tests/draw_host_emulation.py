"""Test infrastructure: the kernels of metran_amd/csrc/draw_kernels.hip compiled FOR THE HOST, unchanged -- a workgroup is 256
std::threads and ``__syncthreads`` a std::barrier, the dynamic LDS a NaN-filled array per block, blocks run one after the
other through the file's own launchers (so tile sizes, group sizes and grids are the shipped ones).  It lets the CPU tier run
the kernels' generator, indexing, tiling and barrier placement against the numpy restatement; the math library is the
host's, so agreement is to rounding, not the GPU tier's business of the device's log / sincos."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metran_amd", "csrc")

PRELUDE = r"""
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <limits>
#include <thread>
#include <vector>
using std::isfinite;
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1) : x(a), y(1), z(1) {} };
static thread_local dim3 threadIdx, blockIdx;
static dim3 gridDim;
static std::barrier<> *g_bar;
static double *g_lds;
#define __syncthreads() g_bar->arrive_and_wait()
#define __global__
#define __launch_bounds__(x)
#define __device__
#define __forceinline__ inline
typedef int hipError_t;
typedef int hipStream_t;
enum { hipSuccess = 0, hipErrorInvalidValue = 1 };
static int hipGetLastError() { return 0; }
static inline void host_sincos(double x, double *s, double *c) { *s = sin(x); *c = cos(x); }
#define sincos host_sincos
static void emulate(std::function<void()> body, dim3 grid, dim3 block, size_t ldsbytes)
{
    gridDim = grid;
    for (unsigned b = 0; b < grid.x; ++b) {
        std::vector<double> lds(ldsbytes / 8 + 1, std::numeric_limits<double>::quiet_NaN());
        g_lds = lds.data();
        std::barrier<> bar(block.x);
        g_bar = &bar;
        std::vector<std::thread> th;
        for (unsigned i = 0; i < block.x; ++i)
            th.emplace_back([&body, i, b]() { threadIdx = dim3(i); blockIdx = dim3(b); body(); });
        for (auto &t : th) t.join();
    }
}
#define hipLaunchKernelGGL(kern, grid, block, ldsbytes, stream, ...) emulate([&]() { kern(__VA_ARGS__); }, grid, block, ldsbytes)
"""

ENTRY = r"""
extern "C" int run_perturb(long B, long R, long T, int N, int K, long S, int tm, uint64_t seed, long fi, long fd, int anti,
                           const double *obs, const double *phi, const double *q, const double *load, const double *obsvar,
                           const double *L0, double *ystar, double *zx, double *xp)
{
    mk::DrawArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.R = R; a.T = T; a.N = N; a.K = K; a.S = S;
    a.bs = tm ? 1 : T; a.ts = tm ? S * B : 1; a.obs_bs = tm ? 1 : T; a.obs_ts = tm ? R : 1;
    a.seed = seed; a.first_instance = fi; a.first_draw = fd; a.antithetic = anti;
    a.obs = obs; a.phi = phi; a.q = q; a.loadings = load; a.obsvar = obsvar; a.L0 = L0;
    a.ystar = ystar; a.zxplus = zx; a.xplus = xp;
    return mk::launch_draw_perturb(a, 0);
}
extern "C" int run_combine(long SB, long B, long R, long T, int W, int tm, const double *scale, const double *plus, double *inout)
{
    mk::DrawCombineArgs a;
    a.SB = SB; a.B = B; a.R = R; a.T = T; a.W = W; a.time_major = tm; a.scale = scale; a.plus = plus; a.inout = inout;
    return mk::launch_draw_combine(a, 0);
}
extern "C" int run_normals(uint64_t seed, long fi, long ni, long fd, long nd, long T, int ncomp, int anti, int raw, double *out)
{
    mk::DrawNormalsArgs a;
    a.seed = seed; a.first_instance = fi; a.ninstances = ni; a.first_draw = fd; a.ndraws = nd; a.T = T;
    a.ncomp = ncomp; a.antithetic = anti; a.raw = raw; a.out = out;
    return mk::launch_draw_normals(a, 0);
}
"""


def build(directory):
    """Compile the emulation into ``directory`` and return the bound library."""
    hdr = open(os.path.join(CSRC, "draw_kernels.h")).read()
    src = open(os.path.join(CSRC, "draw_kernels.hip")).read()
    for text, old, new in ((hdr, "#include <hip/hip_runtime.h>", ""), (hdr, "#pragma once", ""),
                           (src, '#include "draw_kernels.h"', ""), (src, "extern __shared__ double lds[];", "double *lds = g_lds;")):
        assert old in text, "draw_kernels: %r is gone -- the emulation's one textual hook" % old
    hdr = hdr.replace("#include <hip/hip_runtime.h>", "").replace("#pragma once", "")
    src = src.replace('#include "draw_kernels.h"', "").replace("extern __shared__ double lds[];", "double *lds = g_lds;")
    cpp = os.path.join(str(directory), "draw_kernels_host.cpp")
    lib = os.path.join(str(directory), "libdraw_kernels_host.so")
    open(cpp, "w").write(PRELUDE + hdr + src + ENTRY)
    # no fused multiply-add: the restatement is plain numpy
    subprocess.check_call(["g++", "-O1", "-std=c++20", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", cpp, "-o", lib])
    L = ctypes.CDLL(lib)
    vp, lg, it = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
    L.run_perturb.argtypes = [lg, lg, lg, it, it, lg, it, ctypes.c_uint64, lg, lg, it] + [vp] * 9
    L.run_combine.argtypes = [lg, lg, lg, lg, it, it, vp, vp, vp]
    L.run_normals.argtypes = [ctypes.c_uint64, lg, lg, lg, lg, lg, it, it, it, vp]
    return L


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)

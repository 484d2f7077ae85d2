// draw_kernels.h -- the simulation smoother's device half (draw_kernels.hip): argument blocks shared with the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mk {

struct DrawArgs {
    long B, R, T;            // instances of the caller's problem, its records, steps
    int N, K;
    long S;                  // draws of this launch: the outputs hold S * B paths, path id = s * B + i
    long bs, ts;             // outputs: block (id, t) at row id*bs + t*ts (rows of N resp. n doubles)
    long obs_bs, obs_ts;     // observations: record (r, t) at row r*obs_bs + t*obs_ts
    uint64_t seed;
    long first_instance, first_draw;
    int antithetic;
    const double *obs, *phi, *q, *loadings, *obsvar; // as in mk_problem
    const double *L0;        // [B,n,n] lower Cholesky factor of P0, or NULL = identity
    double *ystar;           // [S*B,T,N] perturbed records
    double *zxplus;          // [S*B,T,N] unscaled projection of the unconditional path, or NULL
    double *xplus;           // [S*B,T,n] unconditional path, or NULL
};

struct DrawCombineArgs {
    long SB, B, R, T;
    int W;                   // row width: N (series) or n (states)
    int time_major;
    const double *scale;     // series: [R,N] or NULL = 1; states: NULL
    const double *plus;
    double *inout;
};

struct DrawNormalsArgs {
    uint64_t seed;
    long first_instance, ninstances, first_draw, ndraws, T;
    int ncomp, antithetic, raw;
    double *out;             // [ndraws, ninstances, T + 1, ncomp]; time index 0 is the initial state (counter word 0 = 0)
};

hipError_t launch_draw_perturb(const DrawArgs &a, hipStream_t s);
hipError_t launch_draw_combine(const DrawCombineArgs &a, hipStream_t s);
hipError_t launch_draw_normals(const DrawNormalsArgs &a, hipStream_t s);

} // namespace mk

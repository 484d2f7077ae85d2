// shift_kernels.h -- the level-shift scan (shift_kernels.hip): argument block shared with the C ABI.  The gain tape is the one of
// weights_kernels.h, the innovations are the scores' row behind it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mk {

constexpr int shift_max_states = 64; // n = N + K served by the kernel (one state per lane)

struct ShiftArgs {
    long B, R, T;
    int N, K;
    long bs, ts;             // block (b, t) of the workspace and of the outputs at b*bs + t*ts
    long gs;                 // gain tape: cell (b, t, j) at ((b*bs + t*ts)*N + j)*gs doubles
    long obs_bs, obs_ts;     // as in mk_problem (the observations are in the tape already: not read)
    const double *obs, *phi, *q, *loadings, *obsvar, *x0, *P0; // as in mk_problem (only phi and the loadings are read)
    const double *gain;      // gain tape written by innov_step_kernel, zero at the cells that are not observed
    const double *v;         // innovations written by innov_step_kernel: cell (b, t, j) at (b*bs + t*ts)*N + j
    double *num, *den;       // [B,T,N] in the workspace's layout: A = x'u and D = x'Mx of the shift of series j from step t on
};

hipError_t launch_shift_scan(const ShiftArgs &a, hipStream_t s);

} // namespace mk

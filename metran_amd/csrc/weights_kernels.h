// weights_kernels.h -- observation weights of smoothed series and states (weights_kernels.hip): argument block shared with the
// C ABI, and the layout of the gain tape that innov_step_kernel writes for it (InnovArgs.gain).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mk {

constexpr int weights_max_states = 64; // n = N + K served by weights_walk_kernel (one state per lane)

// doubles of one gain-tape slot [ d(n) | 1/f | pad ]: even, so that every slot starts on a 16-byte boundary
constexpr long weights_slot_stride(long n) { return (n + 3) & ~1L; }

struct WeightsArgs {
    long B, R, T, M;
    int N, K;
    int states;              // 0: column = series j*, c = z_j*;  1: column = state i, c = e_i
    long bs, ts, rs;         // filtered records: (b, t) at (b*bs + t*ts)*rs doubles; the tape's cells use the same (bs, ts)
    long gs;                 // gain tape: cell (b, t, j) at ((b*bs + t*ts)*N + j)*gs doubles
    long obs_bs, obs_ts;     // observations: record (r, t) at row r*obs_bs + t*obs_ts
    const double *obs, *phi, *q, *loadings, *obsvar, *x0, *P0; // as in mk_problem (obsvar is in 1/f already: not read)
    const double *F;         // filtered record array written by the recording forward pass
    const double *gain;      // gain tape written by innov_step_kernel, zero at the cells that are not observed
    const int64_t *targets;  // [R,M,2] = (step, column); instance b uses the targets of record b % R
    double *weights;         // [B,M,T,N]
    double *intercept;       // [B,M] or NULL
};

hipError_t launch_weights_walk(const WeightsArgs &a, hipStream_t s);

} // namespace mk

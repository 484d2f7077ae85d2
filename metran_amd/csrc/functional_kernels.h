// functional_kernels.h -- exact window means, changes and contrasts of the smoothed signal (functional_kernels.hip): argument block
// shared with the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mk {

constexpr int functional_max_states = 64;    // n = N + K served by functional_walk_kernel (one state per lane)
constexpr int functional_max_contrasts = 64; // C per call

struct FunctionalArgs {
    long B, R, T, W, C;
    int N, K;
    long bs, ts, rs;         // filtered and smoothed records: (b, t) at (b*bs + t*ts)*rs doubles, [ mean(n) | covariance(n*n) | pad ]
    const double *phi, *q, *loadings, *scale, *offset; // as in mk_problem (scale / offset NULL = 1 / 0)
    const double *F;         // filtered record array written by the recording forward pass
    const double *S;         // smoothed record array written by the smoother
    const int64_t *windows;  // [R,W,4] = (t0, t1, t2, t3); instance b uses the windows of record b % R
    const double *contrasts; // [R,C,N] or NULL = the N unit contrasts (C = N)
    double *mean, *var;      // [B,W,C]
    unsigned *status;        // [B] or NULL: the pivot bits of the walk are ORed in
};

hipError_t launch_functional_walk(const FunctionalArgs &a, hipStream_t s);

} // namespace mk

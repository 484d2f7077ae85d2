// walk_prims.h -- the backward (r, N) walk over the gain tape, shared by the kernels that run it (block_kernels.hip: the
// checkpoint and the block walk; shift_kernels.hip: the level-shift scan): the LDS of one lane group and the three device
// functions of a cell and a step.  One spelling, so that the walks of these kernels give the same numbers bit for bit.  Notation
// as in block_kernels.hip's header; lane = state.  Include it behind `#pragma clang fp contract(off)`.
#pragma once
#include <hip/hip_runtime.h>

#include "mk_prims.h" // wave_lds_sync
#include "reader_prims.h"

namespace mk {

__host__ __device__ inline long even(long x) { return (x + 1) & ~1L; }
// doubles of LDS of the (r, N) walk of one lane group: the loadings, N (rows of n | 1), and k, g, phi (64 each)
__host__ __device__ inline long walk_lds_doubles(int N, int K)
{
    const int n = N + K;
    return even((long)N * K) + even((long)n * (n | 1)) + 3 * 64;
}

struct WalkLds {
    double *Gm, *Nm, *kv, *gv, *ph;
    int ns;
};
__device__ __forceinline__ WalkLds carve_walk(double *base, int N, int K)
{
    const int n = N + K;
    WalkLds w;
    w.Gm = base;
    w.Nm = w.Gm + even((long)N * K);
    w.kv = w.Nm + even((long)n * (n | 1));
    w.gv = w.kv + 64;
    w.ph = w.gv + 64;
    w.ns = n | 1;
    return w;
}

// One cell (t, j) of the backward walk: lane = state (act: lane < n; the others carry zeros).  d = the lane's entry of the
// slot, z = the lane's entry of z_j.  Leaves k in kv and g in gv for the caller; returns u_s and M_ss in every lane.
template <int G>
__device__ __forceinline__ void cell_products(const WalkLds &w, int lane, bool act, int n, double d, double rf, double v, double r,
                                              double &g, double &us, double &mss)
{
    const double k = d * rf;
    w.kv[lane] = k;
    wave_lds_sync();
    g = 0.0;
    if (act) { // the loads of four terms go out together; the sum keeps its order
#pragma unroll 4
        for (int c = 0; c < n; ++c) g = fma(w.Nm[lane * w.ns + c], w.kv[c], g);
    }
    const double kr = group_sum<G>(k * r);
    mss = rf + group_sum<G>(k * g);
    us = fma(v, rf, -kr);
    w.gv[lane] = g;
    wave_lds_sync();
}
// r += z_j' u_s and N += -z_j g' - g z_j' + M_ss z_j' z_j: the columns where z_j is not zero in every row, the others in the rows
// where it is not; one formula for both, so that N stays symmetric bit for bit
__device__ __forceinline__ void cell_update(const WalkLds &w, int lane, bool act, int N, int K, int j, double z, double g, double us,
                                            double mss, double &r)
{
    r = fma(z, us, r);
    if (act) {
        double *row = w.Nm + lane * w.ns;
        row[j] = fma(mss, z, row[j] - (z * w.gv[j] + g));
        for (int l = 0; l < K; ++l) {
            const double zc = w.Gm[j * K + l];
            row[N + l] = fma(mss, z * zc, row[N + l] - (z * w.gv[N + l] + g * zc));
        }
        if (lane == j || lane >= N)
            for (int c = 0; c < N; ++c)
                if (c != j) row[c] = row[c] - z * w.gv[c];
    }
    wave_lds_sync();
}
__device__ __forceinline__ void pull_back(const WalkLds &w, int lane, bool act, int n, double phi_r, double &r)
{
    r = phi_r * r;
    if (act) {
#pragma unroll 4
        for (int c = 0; c < n; ++c) w.Nm[lane * w.ns + c] = w.Nm[lane * w.ns + c] * (phi_r * w.ph[c]);
    }
    wave_lds_sync();
}

} // namespace mk

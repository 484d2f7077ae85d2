// reader_prims.h -- device helpers shared by the kernels that read the filtered records: the scaling of a forecast (innov_kernels.hip,
// forecast_kernels.hip: one spelling of what the two must agree on bit for bit, a track of horizon 1 is pred_mean / pred_var) and
// the fixed-tree sum over a lane group (weights_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace mk {

// a forecast's mean and variance in the caller's units (mk_problem's scale / offset); a variance that rounding took below zero
// is stored as zero
__device__ __forceinline__ double scaled_mean(double pm, double sc, double of) { return fma(pm, sc, of); }
__device__ __forceinline__ double scaled_var(double pv, double sc) { return (pv < 0.0 ? 0.0 : pv) * sc * sc; }

// the sum of x over the G lanes of a lane group (G = 16 or 64, the groups aligned in the wavefront), bit-identical in every lane:
// at each stage two lanes that exchange their values add the same two numbers -- a fixed tree, whatever runs in the other
// groups.  Inside a row of 16 lanes the exchanges are DPP moves, no LDS round trip: lane ^ 1 and lane ^ 2 (quad permutations), then
// the mirror images within 8 and within 16 lanes (after the first two stages every quad holds one value, so a mirror pairs
// each quad with the other one); across the four rows of a wavefront lane ^ 16 and lane ^ 32.
__device__ __forceinline__ double row_sum(double x)
{
    x += __builtin_amdgcn_update_dpp(0.0, x, 0xB1, 0xf, 0xf, true);  // quad_perm:[1,0,3,2]
    x += __builtin_amdgcn_update_dpp(0.0, x, 0x4E, 0xf, 0xf, true);  // quad_perm:[2,3,0,1]
    x += __builtin_amdgcn_update_dpp(0.0, x, 0x141, 0xf, 0xf, true); // row_half_mirror
    x += __builtin_amdgcn_update_dpp(0.0, x, 0x140, 0xf, 0xf, true); // row_mirror
    return x;
}
template <int G>
__device__ __forceinline__ double group_sum(double x)
{
    static_assert(G == 16 || G == 64, "a row of 16 lanes or a wavefront");
    x = row_sum(x);
    if constexpr (G == 64) {
        x += __shfl_xor(x, 16, 64);
        x += __shfl_xor(x, 32, 64);
    }
    return x;
}

} // namespace mk

// Sums inside groups of 2^gshift consecutive lanes of a wave by DPP moves: shared by attention.hip and norm.hip.
#pragma once
#include "common.h"

template <int CTRL>
__device__ inline float dpp_move(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
__device__ inline float read_lane(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// Sum over each group of 2^gshift consecutive lanes, every lane of a group gets it; gshift is wave-uniform and EVERY lane of
// the wave is active (the callers' control flow is scalar). Steps 1, 2: quad_perm [1,0,3,2] and [2,3,0,1]; 4: row_half_mirror
// (lane k <-> 7 - k of its half row: the two quads there already hold their sums); 8: row_mirror; 16, 32: the four row sums.
__device__ inline float group_sum(float v, int gshift, int lane) {
    if (gshift >= 1) v = v + dpp_move<0xB1>(v);
    if (gshift >= 2) v = v + dpp_move<0x4E>(v);
    if (gshift >= 3) v = v + dpp_move<0x141>(v);
    if (gshift >= 4) v = v + dpp_move<0x140>(v);
    if (gshift >= 5) {
        const float lo = read_lane(v, 0) + read_lane(v, 16), hi = read_lane(v, 32) + read_lane(v, 48);
        v = gshift == 5 ? (lane < 32 ? lo : hi) : lo + hi;
    }
    return v;
}

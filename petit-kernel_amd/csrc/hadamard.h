// hadamard.h -- the block-Hadamard rotation "petit-had/1" (include/petit_amd.h "Block-Hadamard rotation"), its butterfly stated once.
// Plain C++ that is also device code (PETIT_HD, as numfmt.h): the kernels hold 8 consecutive k per lane and run the strides 1, 2 and 4 with
// hadamard8 below, then exchange lanes for the strides 8 .. B / 2 (qact_hadamard.inc); the host twins run hadamard8 on every 8 elements and
// the same pair rule across them (hadamard_block_host).  Every sum and every difference is ONE f32 operation and nothing is fused: the
// translation units that include this file compile with floating-point contraction off, and there is no product in here to fuse with.
#pragma once

#include "layout.h" // PETIT_HD

namespace petit_amd {

// the butterfly of the definition: (a, b) <- (a + b, a - b)
PETIT_HD void hadamard_pair(float &a, float &b) {
    const float s = a + b, d = a - b;
    a = s, b = d;
}

// stages s = 0, 1, 2 (d = 1, 2, 4) on 8 consecutive elements, in this order
PETIT_HD void hadamard8(float (&v)[8]) {
#pragma unroll
    for (int d = 1; d < 8; d <<= 1)
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if ((i & d) == 0)
                hadamard_pair(v[i], v[i + d]);
}

#if defined(__HIP_DEVICE_COMPILE__)
// The value lane ^ BIT holds, BIT = 1, 2, 4 or 8: a data-parallel-primitive move inside the row of 16 lanes, which the compiler folds into the
// add that follows -- no LDS crossbar and no address register, where __shfl_xor is a ds_bpermute_b32 per value.  ^1 and ^2 are quad
// permutations, ^8 is the row rotated by 8, and ^4 is the half-row mirror (^7) followed by the quad reversed (^3).  The 16 lanes of a k-tile
// are live or masked together, so every lane read here is live.
template <int CTRL> __device__ __forceinline__ float hadamard_dpp(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true));
}
template <int BIT> __device__ __forceinline__ float hadamard_lane_xor(float x) {
    static_assert(BIT == 1 || BIT == 2 || BIT == 4 || BIT == 8, "an exchange inside a row of 16 lanes");
    if constexpr (BIT == 1)
        return hadamard_dpp<0xB1>(x); // quad_perm:[1,0,3,2]
    else if constexpr (BIT == 2)
        return hadamard_dpp<0x4E>(x); // quad_perm:[2,3,0,1]
    else if constexpr (BIT == 4)
        return hadamard_dpp<0x1B>(hadamard_dpp<0x141>(x)); // row_half_mirror, then quad_perm:[3,2,1,0]
    else
        return hadamard_dpp<0x128>(x); // row_ror:8
}
// the stage of stride 8 BIT across lanes: the lane whose bit is clear keeps mine + other, the lane whose bit is set keeps other - mine
template <int BIT> __device__ __forceinline__ void hadamard_lane_stage(float (&v)[8], unsigned lane) {
    const unsigned flip = (lane & BIT) ? 0x80000000u : 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float other = hadamard_lane_xor<BIT>(v[i]);
        v[i] = other + __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v[i]) ^ flip); // (a + b and b + a are the same bits)
    }
}
#endif

constexpr bool hadamard_block_ok(unsigned block) { return block == 0 || block == 32 || block == 128; }
constexpr int hadamard_log2(unsigned block) { return block == 128 ? 7 : 5; }

// one block of B = 32 or 128 consecutive elements in place, the stages in ascending order; host only
inline void hadamard_block_host(float *z, unsigned B) {
    for (unsigned c = 0; c < B; c += 8)
        hadamard8(*reinterpret_cast<float (*)[8]>(z + c));
    for (unsigned d = 8; d < B; d <<= 1)
        for (unsigned i = 0; i < B; ++i)
            if ((i & d) == 0)
                hadamard_pair(z[i], z[i + d]);
}
// a row of k elements, k a multiple of B
inline void hadamard_row_host(float *z, unsigned k, unsigned B) {
    for (unsigned b = 0; b < k; b += B)
        hadamard_block_host(z + b, B);
}

} // namespace petit_amd

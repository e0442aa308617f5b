// gemm_native_decode.hpp -- the decode GEMM on the native image (include/petit_amd.h "Decode on the native image"): 1 <= M <= 32 rows against
// a "petit-cdna4-nv6/1" image (layout.h) as a pure weight stream.  The image's registers ARE the FP6 operand of
// v_mfma_scale_f32_32x32x64_f8f6f4, so nothing is unpacked; the M <= 32 activation rows are the instruction's other 32-wide operand, so the
// weight stream and the MFMA count do not move with M.
//
// Work split: grid = blocks x P.  A workgroup owns ONE block of 32 weight rows (gated: gate block b and up block b + n / 64) and part p of the
//   k-tiles, [p T / P, (p + 1) T / P) of T = k / 128; its W <= 4 waves take contiguous runs of that part, wave w the k-tiles
//   [w t / W, (w + 1) t / W) of the part's t.  W = min(4, T / P, 16 / P) (decode_waves): every wave has a k-tile, and W P <= 16 -- the number of
//   f32 partial sums an output is added from, which the class's bound allows.
// Weights: a block's image is one contiguous run of 3 KiB per k-tile; a lane issues the three 16-byte loads of its units (planes 0, 1, 2 of
//   nv6_unit_offset) non-temporal through a descriptor that ends with the wave's run, into a register ring kDecodeRing k-tiles deep (gated:
//   half as deep for each of the two blocks, the same bytes in flight) that is refilled as soon as the k-tile has left it.  No LDS and no
//   barrier in the K loop.  The two E8M0 bytes of the k-tile (nv6_scale_offset, q = 0, 1) ride in the same ring.
// Activations: lane 32 h + r holds row r.  Quantised input ("petit-qact/1"): the lane's units and the row's scale dword of the k-tile, as the
//   invariant split kernel reads them.  16-bit input: the lane loads its own 64 bytes per instruction (a ring of its own, 2 k-tiles deep: the
//   rows come from the L2, and a k-tile of them is 32 registers) and quantises them in registers with the
//   quantisers' arithmetic (qact_column.inc, qact_block6.inc: the block maximum, act_scale_byte, the same hardware converts) -- bit for bit
//   what petit_quantize_activations writes.  MXFP6 / MXFP4: the lane's operand is k 32 h .. 32 h + 31 of the instruction, exactly one 32-k
//   block, no cross-lane traffic.  MXFP8: the instruction's e4m3 operand of lane h is k 16 h .. 16 h + 15 and 32 + 16 h .. 32 + 16 h + 15 (the
//   layout probed in gemm_native32.hpp), one half of each of two blocks, so the two half-block maxima cross to lane ^ 32 once (two
//   ds_bpermute per instruction; no LDS memory).  Rows >= M are out of the descriptor's range: they load zeros and are never stored.
// Reduction: the W accumulator tiles meet in LDS (W x 4 KiB per block) and are added in ascending wave order, thread (u, lane) taking the
//   lane's registers 4 u .. 4 u + 3 = four consecutive output columns.  P = 1: that thread runs the epilogue.  P > 1: it stores the f32x4 into
//   slab p of [P][m][n], and invariant_fold_kernel (gemm_invariant.hpp) adds the slabs in ascending p and runs the same epilogue.
// Epilogue: the class's plain one (invariant_finish4: a multiply by gs when given, an add of the bias when given, one rounding) or the gated
//   ones (finish4_silu_mul).  Rows < M and columns < N only; vector stores only.
#pragma once

#include <hip/hip_runtime.h>

#include "gemm_native_invariant.hpp"

namespace petit_amd {

constexpr unsigned kDecodeMaxM = 32;      // rows of the instruction's activation operand
constexpr unsigned kDecodeMaxWaves = 4;   // W
constexpr unsigned kDecodeMaxSums = 16;   // W P: the partial sums of one output ("<= 16 cross-wave / cross-slice f32 additions", petit_amd.h)
constexpr int kDecodeRing = 4;            // weight k-tiles in flight per wave (gated: two of each block)

// W of a launch with P parts over T k-tiles (0: P is not legal -- a part without a k-tile, or more than 16 parts)
PETIT_HD unsigned decode_waves(unsigned ktiles, unsigned parts) {
    if (parts == 0 || parts > kDecodeMaxSums || ktiles / parts == 0)
        return 0;
    const unsigned t = ktiles / parts, cap = kDecodeMaxSums / parts;
    const unsigned w = t < kDecodeMaxWaves ? t : kDecodeMaxWaves;
    return w < cap ? w : cap;
}

struct NativeDecodeArgs {
    void *c;         // [m][n] (gated: [m][n/2]) 16-bit
    const void *a;   // 16-bit [m][k], or the "petit-qact/1" bytes of (m, k, ACT)
    const void *w;   // the image's elements
    const void *s;   // the image's scale region
    const float *gs; // device pointer to one float, or null: no multiply
    const void *bias; // [n] in c's type, or null: no add
    float *slabs;    // parts > 1: [parts][m][n] fp32
    unsigned m, n, k;
    unsigned parts;  // P
    unsigned act;    // PETIT_ACTIVATION_*
};

// 16-bit input: the lane's raw bytes of one k-tile -- per instruction q four 16-byte units: MXFP6 / MXFP4 the 32 elements from k = 64 q + 32 h on;
// MXFP8 the 16 elements from 64 q + 16 h on (units 0, 1) and the 16 from 64 q + 32 + 16 h on (units 2, 3)
struct DecodeRawA {
    u32x4 u[2][4];
};

// 8 consecutive elements of a 16-byte unit as f32 (exact)
template <class AT> __device__ __forceinline__ void decode_unit_f32(const u32x4 raw, float (&v)[8]) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const unsigned w = raw[d];
        if constexpr (AT::kType == kDataTypeBf16) {
            const unsigned lo = w << 16, hi = w & 0xffff0000u;
            v[2 * d] = __builtin_bit_cast(float, lo);
            v[2 * d + 1] = __builtin_bit_cast(float, hi);
        } else {
            const f16x2 p = __builtin_bit_cast(f16x2, w);
            v[2 * d] = (float)p[0];
            v[2 * d + 1] = (float)p[1];
        }
    }
}

// The lane's operand units of one k-tile (the order native_inv_aop reads) and its scale bytes for P1 / P2 from the raw 16-bit elements: the
// quantisers' arithmetic on the lane's own block(s).
template <class AT, int ACT>
__device__ __forceinline__ void decode_quantize(const DecodeRawA &raw, const unsigned h, u32x4 (&a)[native_inv_frag_units<ACT>()],
                                                unsigned (&a_sc)[2]) {
    constexpr bool BF16 = AT::kType == kDataTypeBf16;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        if constexpr (ACT == 6) { // qact_block6.inc: the maximum on the 16-bit patterns, the 32-element convert
            unsigned mx = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const unsigned w = raw.u[q][j][d] & 0x7fff7fffu;
                    const unsigned lo = w & 0xffffu, hi = w >> 16;
                    mx = mx > lo ? mx : lo;
                    mx = mx > hi ? mx : hi;
                }
            const unsigned sbyte = act_scale_byte<6>(h16_f32<BF16>(mx));
            const float scale = bits_f32(sbyte << 23);
            const u32x4 r0 = raw.u[q][0], r1 = raw.u[q][1], r2 = raw.u[q][2], r3 = raw.u[q][3];
            const u32x16 packed = u32x16{r0[0], r0[1], r0[2], r0[3], r1[0], r1[1], r1[2], r1[3], r2[0], r2[1], r2[2], r2[3], r3[0], r3[1], r3[2], r3[3]};
            const u32x6 c = cvt_pk32_fp6_16bit<BF16>(packed, scale); // (early-clobber form: device_common.hpp)
            a[q] = u32x4{c[0], c[1], c[2], c[3]};
            a[2][2 * q] = c[4], a[2][2 * q + 1] = c[5];
            a_sc[q] = sbyte;
        } else { // qact_column.inc, on the four 8-element columns the lane holds
            float v[4][8];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                decode_unit_f32<AT>(raw.u[q][j], v[j]);
            float amax[2] = {0.f, 0.f}; // MXFP4: [0] is the block's; MXFP8: the lane's halves of blocks 2 q and 2 q + 1
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    amax[ACT == 8 ? j >> 1 : 0] = fmaxf(amax[ACT == 8 ? j >> 1 : 0], fabsf(v[j][i]));
            if constexpr (ACT == 8) {
                unsigned sb[2];
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    amax[b] = fmaxf(amax[b], __shfl_xor(amax[b], 32)); // the other half of the block: the same row at lane ^ 32
                    sb[b] = act_scale_byte<8>(amax[b]);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float inv = bits_f32((254u - sb[j >> 1]) << 23); // 2^-(sbyte - 127)
                    int q0 = 0, q1 = 0;
                    q0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[j][0] * inv, v[j][1] * inv, q0, false);
                    q0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[j][2] * inv, v[j][3] * inv, q0, true);
                    q1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[j][4] * inv, v[j][5] * inv, q1, false);
                    q1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[j][6] * inv, v[j][7] * inv, q1, true);
                    a[2 * q + (j >> 1)][2 * (j & 1)] = (unsigned)q0, a[2 * q + (j >> 1)][2 * (j & 1) + 1] = (unsigned)q1;
                }
                a_sc[q] = h ? sb[1] : sb[0]; // lane h supplies the byte of block 2 q + h
            } else {
                const unsigned sbyte = act_scale_byte<4>(amax[0]);
                const float scale = bits_f32(sbyte << 23); // 2^(sbyte - 127)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    unsigned c = 0;
                    c = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(c, v[j][0], v[j][1], scale, 0);
                    c = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(c, v[j][2], v[j][3], scale, 1);
                    c = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(c, v[j][4], v[j][5], scale, 2);
                    c = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(c, v[j][6], v[j][7], scale, 3);
                    a[q][j] = c;
                }
                a_sc[q] = sbyte;
            }
        }
    }
}

// The waves' tiles in red[wave][nb][register][lane] (gemm_native_decode_kloop.inc) added in ascending wave order: thread (u, lane) takes the
// lane's registers 4 u .. 4 u + 3 of each block.
template <int NB> __device__ __forceinline__ void decode_sum4(const float *red, const unsigned waves, const unsigned u, const unsigned lane, f32x4 (&sum)[NB]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            sum[nb][i] = red[(nb * 16u + 4u * u + i) * 64u + lane];
        for (unsigned w = 1; w < waves; ++w) // ascending wave order
#pragma unroll
            for (int i = 0; i < 4; ++i)
                sum[nb][i] = sum[nb][i] + red[((w * NB + nb) * 16u + 4u * u + i) * 64u + lane];
    }
}

// AT: Bf16 / Fp16.  ACT: 8 / 6 / 4.  QIN: A is "petit-qact/1" bytes (else 16-bit).  GATED: two blocks per workgroup and a gated epilogue.
// blockDim.x = 64 W (decode_waves), grid = (blocks, P).
template <class AT, int ACT, bool QIN, bool GATED> __global__ __launch_bounds__(256) void native_decode_kernel(const NativeDecodeArgs p) {
#pragma clang fp contract(off)
    constexpr int NB = GATED ? 2 : 1, NA = native_inv_frag_units<ACT>();
    constexpr unsigned kRowB = native_inv_row_bytes<ACT>();
    __shared__ __attribute__((aligned(16))) float red[kDecodeMaxWaves * NB * 1024];
    const unsigned tid = threadIdx.x, lane = tid & 63u, r = lane & 31u, h = lane >> 5;
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6), waves = blockDim.x >> 6;
    const unsigned ktiles = p.k / kTileK, ks = (unsigned)span_tiles_for_k(p.k);
    const unsigned part = blockIdx.y;
    const unsigned pk0 = part * ktiles / p.parts, pk1 = (part + 1u) * ktiles / p.parts, pt = pk1 - pk0;
    const unsigned kt0 = pk0 + wave * pt / waves, kt1 = pk0 + (wave + 1u) * pt / waves, run = kt1 - kt0; // (run >= 1: decode_waves)
    unsigned blk[NB];
    blk[0] = blockIdx.x;
    if constexpr (GATED)
        blk[1] = blockIdx.x + p.n / 64u;

    // the wave's run of each block's stream: 3 KiB of elements per k-tile from k-tile kt0 on; loads past the run's end read zeros.  The scale
    // region of the block: 128 bytes per k-tile, span records (nv6_scale_offset)
    __amdgpu_buffer_rsrc_t w_rsrc[NB], s_rsrc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        w_rsrc[nb] = make_rsrc((const char *)p.w + ((size_t)blk[nb] * ktiles + kt0) * kNv6TileBytes, run * kNv6TileBytes);
        s_rsrc[nb] = make_rsrc((const char *)p.s + (size_t)blk[nb] * ktiles * 128, ktiles * 128);
    }
    const unsigned char *const qa = (const unsigned char *)p.a;
    const unsigned char *const qa_hi = qa + qact_hi_offset(p.m, p.k); // (MXFP6; "petit-qact/1": layout.h)
    const unsigned char *const qs = qa + qact_elem_bytes(p.m, p.k, ACT);
    const __amdgpu_buffer_rsrc_t a16_rsrc = make_rsrc(p.a, QIN ? 0u : p.m * p.k * 2u); // rows >= m: out of range -> zeros
    const unsigned a16_voff = r * p.k * 2u + h * (ACT == 8 ? 32u : 64u);

    const unsigned qa_m = p.m, qa_m0 = 0u, qa_rows = p.m; // the m-tile is the whole image: rows >= m are out of range -> zeros
    // the K loop: rings, MFMA, the waves' tiles into red (shared with the routed-expert form, gemm_native_moe_decode.hpp)
#include "gemm_native_decode_kloop.inc"
    // lane (r, h) holds row r; register 4 u + i is column 16 (u >> 1) + 8 (u & 1) + 4 h + i of the block's 32
    if (r >= p.m)
        return;
    for (unsigned u = wave; u < 4u; u += waves) {
        f32x4 sum[NB];
        decode_sum4<NB>(red, waves, u, lane, sum);
        const unsigned nl = (u >> 1) * 16u + (u & 1u) * 8u + 4u * h;
        if (p.parts > 1u) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const unsigned n = blk[nb] * 32u + nl;
                if (n < p.n)
                    *reinterpret_cast<f32x4 *>(p.slabs + ((size_t)part * p.m + r) * p.n + n) = sum[nb];
            }
        } else if constexpr (GATED) {
            const unsigned n_half = p.n / 2u, n = blk[0] * 32u + nl; // (n_half % 32 == 0: every column of the block exists)
            const float g = p.gs ? *p.gs : 1.0f;
            *reinterpret_cast<uint2 *>((char *)p.c + ((size_t)r * n_half + n) * 2) = finish4_silu_mul<AT>(sum[0], sum[1], g, p.bias, n, n_half, p.act);
        } else {
            const unsigned n = blk[0] * 32u + nl;
            if (n < p.n)
                *reinterpret_cast<uint2 *>((char *)p.c + ((size_t)r * p.n + n) * 2) = invariant_finish4<AT>(sum[0], p.gs, p.bias, n);
        }
    }
}

// one 16-bit type's launches; instantiated by gemm_native_decode_{bf16,f16}.hip
template <class AT, int ACT, bool QIN> void native_decode_launch_fmt(const NativeDecodeArgs &p, hipStream_t stream) {
    const unsigned waves = decode_waves(p.k / kTileK, p.parts);
    const dim3 grid(p.act ? p.n / 64u : (p.n + 31u) / 32u, p.parts), block(64u * waves);
    if (p.act)
        hipLaunchKernelGGL((native_decode_kernel<AT, ACT, QIN, true>), grid, block, 0, stream, p);
    else
        hipLaunchKernelGGL((native_decode_kernel<AT, ACT, QIN, false>), grid, block, 0, stream, p);
    if (p.parts > 1u) { // the slabs' fold: the exact class's, with P as its slice count
        InvariantArgs f{};
        f.c = p.c, f.gs = p.gs, f.bias = p.bias, f.slabs = p.slabs, f.m = p.m, f.n = p.n, f.k = p.k, f.slices = p.parts, f.act = p.act;
        const size_t count = (size_t)p.m * ((p.act ? p.n / 2u : p.n) / 4u);
        hipLaunchKernelGGL((invariant_fold_kernel<AT>), dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, f);
    }
}
template <class AT> void native_decode_launch(const NativeDecodeArgs &p, int act_format, bool quantized, hipStream_t stream) {
    if (act_format == 8)
        quantized ? native_decode_launch_fmt<AT, 8, true>(p, stream) : native_decode_launch_fmt<AT, 8, false>(p, stream);
    else if (act_format == 6)
        quantized ? native_decode_launch_fmt<AT, 6, true>(p, stream) : native_decode_launch_fmt<AT, 6, false>(p, stream);
    else
        quantized ? native_decode_launch_fmt<AT, 4, true>(p, stream) : native_decode_launch_fmt<AT, 4, false>(p, stream);
}

} // namespace petit_amd

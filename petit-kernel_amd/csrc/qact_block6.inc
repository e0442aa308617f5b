// qact_block6.inc -- one 32-k block of a row into the "petit-qact/1" image (layout.h) in MXFP6 (e2m3), stated once: the block maximum on the
// 16-bit patterns, the scale byte (act_scale_byte, numfmt.h), the hardware's 32-element convert (v_cvt_scalef32_pk32_fp6_{bf16,f16}: RNE of
// src / scale, saturating at 7.5), the two stores, and the k-tile's four scale bytes as one dword from the k-tile's first lane.  Included by
// quantize_act32_fp6_kernel (gemm_native32.hpp) and by norm_quant_tail (rmsnorm_quant.hip); a text fragment for qact_column.inc's reason.  It reads
//   BF16       constexpr bool: the 16-bit type
//   raw        u32x4[4]: the block's 32 elements, two per dword
//   blk        the block of the row; consecutive lanes hold consecutive blocks, and the four lanes of a k-tile are live or masked together
//   qa, qa_hi, qs   the image, its second image and its scale region (unsigned char *); m, row: the image's row count and this row
{
    // block maximum on the 16-bit patterns (sign cleared: bf16 and fp16 magnitudes order like their bit patterns), exponent from its f32 value
    unsigned mx = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const unsigned w = raw[j][d] & 0x7fff7fffu;
            const unsigned lo = w & 0xffffu, hi = w >> 16;
            mx = mx > lo ? mx : lo;
            mx = mx > hi ? mx : hi;
        }
    const unsigned sbyte = act_scale_byte<6>(h16_f32<BF16>(mx));
    const float scale = bits_f32(sbyte << 23);
    const u32x16 packed = u32x16{raw[0][0], raw[0][1], raw[0][2], raw[0][3], raw[1][0], raw[1][1], raw[1][2], raw[1][3],
                                 raw[2][0], raw[2][1], raw[2][2], raw[2][3], raw[3][0], raw[3][1], raw[3][2], raw[3][3]};
    const u32x6 q = cvt_pk32_fp6_16bit<BF16>(packed, scale); // (early-clobber form: device_common.hpp)
    const unsigned kt = blk / 4, b = blk % 4;
    const size_t tile_row = qact_tile_row(m, kt, row);
    *reinterpret_cast<u32x4 *>(qa + tile_row * qact_row_bytes(6) + 16 * b) = u32x4{q[0], q[1], q[2], q[3]};
    uint2 tail;
    tail.x = q[4], tail.y = q[5];
    *reinterpret_cast<uint2 *>(qa_hi + tile_row * kQactHiRowBytes + 8 * qact_fp6_hi_slot(b)) = tail;
    // the four scale bytes of a row's k-tile leave as one dword (the first lane of the four collects them)
    const unsigned s1 = __shfl_down(sbyte, 1, 4), s2 = __shfl_down(sbyte, 2, 4), s3 = __shfl_down(sbyte, 3, 4);
    if (b == 0)
        *reinterpret_cast<unsigned *>(qs + tile_row * kQactScaleRowBytes) = sbyte | (s1 << 8) | (s2 << 16) | (s3 << 24);
}

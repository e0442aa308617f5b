// qact_column.inc -- one 8-element column of a row into the "petit-qact/1" image (layout.h) in MXFP8 / MXFP4, stated once: the block maximum
// over the quad of lanes that share the column's 32-k block, the scale byte (act_scale_byte, numfmt.h), the hardware converts, the store, and
// the k-tile's four scale bytes as one dword from the k-tile's first lane.  Included by quantize_act32_kernel (gemm_native32.hpp) and by
// norm_quant_tail (rmsnorm_quant.hip), inside their loops over a thread's columns.  A text fragment and not a function: behind a call, inlined
// or not, the address arithmetic is no longer shared across the unrolled columns (profiles/qact_single_definition.md).  It reads
//   ACT        8 or 4
//   v          float[8]: elements 8 c8 .. 8 c8 + 7 of the row
//   c8         the column; consecutive lanes hold consecutive columns, so a quad of lanes is a 32-k block and 16 lanes a k-tile, and the
//              lanes of a k-tile are live or masked together (every shuffle below stays among live lanes)
//   qa, qs     the image and its scale region (unsigned char *); m, row: the image's row count and this row
{
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        amax = fmaxf(amax, fabsf(v[i]));
    amax = fmaxf(amax, __shfl_xor(amax, 1));
    amax = fmaxf(amax, __shfl_xor(amax, 2));
    const unsigned sbyte = act_scale_byte<ACT>(amax);
    const unsigned kt = c8 / 16, col16 = c8 % 16;
    if constexpr (ACT == 8) {
        const float inv = bits_f32((254u - sbyte) << 23); // 2^-(sbyte-127)
        int q0 = 0, q1 = 0;
        q0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[0] * inv, v[1] * inv, q0, false);
        q0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[2] * inv, v[3] * inv, q0, true);
        q1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[4] * inv, v[5] * inv, q1, false);
        q1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[6] * inv, v[7] * inv, q1, true);
        const unsigned u16 = col16 >> 1, half = col16 & 1u; // the column's 16-k unit and its half of it
        const unsigned pos = qact_fp8_unit_pos(u16);
        uint2 o;
        o.x = (unsigned)q0, o.y = (unsigned)q1;
        *reinterpret_cast<uint2 *>(qa + qact_tile_row(m, kt, row) * qact_row_bytes(8) + pos * 16 + half * 8) = o;
    } else {
        // hardware RNE conversion to e2m1 with saturation: dst nibbles = cvt(src / scale)
        const float scale = bits_f32(sbyte << 23); // 2^(sbyte-127)
        unsigned q = 0;
        q = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(q, v[0], v[1], scale, 0);
        q = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(q, v[2], v[3], scale, 1);
        q = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(q, v[4], v[5], scale, 2);
        q = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(q, v[6], v[7], scale, 3);
        *reinterpret_cast<unsigned *>(qa + qact_tile_row(m, kt, row) * qact_row_bytes(4) + col16 * 4) = q;
    }
    // the four scale bytes of a row's k-tile leave as ONE dword (byte stores are the slow path of the memory pipeline): the 16 lanes of a
    // k-tile are consecutive, the first lane of each quad holds the quad's byte
    const unsigned s1 = __shfl_down(sbyte, 4, 16), s2 = __shfl_down(sbyte, 8, 16), s3 = __shfl_down(sbyte, 12, 16);
    if (col16 == 0)
        *reinterpret_cast<unsigned *>(qs + qact_scale_dword(m, kt, row) * kQactScaleRowBytes) = sbyte | (s1 << 8) | (s2 << 16) | (s3 << 24);
}

// qact_hadamard.inc -- the block-Hadamard rotation "petit-had/1" (hadamard.h; include/petit_amd.h "Block-Hadamard rotation") of a row held in
// qact_column.inc's thread map, in place and in registers: included just before that fragment by the rotating quantisers, and by the
// rotation to 16 bit.  A text fragment as qact_column.inc is, and for its reason.  It reads
//   HAD        0 (nothing happens), 32 or 128: the rotation block
//   v          float[8]: elements 8 c8 .. 8 c8 + 7 of the row, replaced by the same elements of the rotated row
//   c8         the column; a quad of consecutive lanes is a 32-k block and 16 lanes a 128-k tile, live or masked together, so the strides
//              1, 2, 4 stay in the lane, 8 and 16 exchange with lanes ^1 and ^2, and 32 and 64 (HAD = 128) with lanes ^4 and ^8
if constexpr (HAD != 0) {
    static_assert(HAD == 32 || HAD == 128, "the rotation block is 32 or 128");
    hadamard8(v);
    hadamard_lane_stage<1>(v, c8);
    hadamard_lane_stage<2>(v, c8);
    if constexpr (HAD == 128) {
        hadamard_lane_stage<4>(v, c8);
        hadamard_lane_stage<8>(v, c8);
    }
}

// gemm_invariant_moe_nv_bf16.hip -- the batch-invariant MoE GEMM's kernels (gemm_invariant_moe.hpp) for one (format, type) pair: kFmtNv weights, Bf16 activations.
#include "gemm_invariant_moe.hpp"

namespace petit_amd {
template void invariant_moe_launch<Bf16, kFmtNv>(InvariantMoeArgs, const invariant::Plan &, hipStream_t);
} // namespace petit_amd

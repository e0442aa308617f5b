"""petit_kernel -- drop-in Python surface of the MI355X (gfx950) build.

Same names, signatures and tensor contracts as the reference package
(petit_kernel/__init__.py:8-79 of causalflow-ai/petit-kernel v0.0.3):
SGLang / vLLM call sites (`repack_nvfp4`, `process_nvfp4_scales`,
`mul_nvfp4_a16(..., solution_id=-1)`) work unchanged.  The packed tensors
returned by `repack_*` / `process_*_scales` keep the reference's shapes and
dtypes but use the gfx950 layout (petit-kernel_amd/csrc/layout.h); they are
opaque and only meaningful to `mul_*_a16` of this build.
"""
import enum

import torch

from . import compiled, gptoss, offline, ops, tuning
from .gptoss import GptOssExperts, prepare_gptoss_experts
from .moe import fp4_moe, fp4_moe_fused, fp4_moe_native, fp4_moe_routed, moe_align
from .ops import QuantizedActivations, mul_fp4_a16_grouped, mul_mxfp4_native, quantize_activations, rmsnorm_quantize
from .ops import attach_nvfp4_native, mul_nvfp4_native, nvfp4_native_image, nvfp4_native_images
from .tuning import tune, tune_tensors
from .ops import SOLUTION_AUTO, SOLUTION_AUTO_NATIVE_MXFP4, SOLUTION_AUTO_NATIVE_MXFP6, SOLUTION_AUTO_NATIVE_MXFP8, PetitSolutionHints
from ._lib import MXFP4_F16RANGE_SCALE_MAX, MXFP4_F16RANGE_SCALE_MIN

# operator layer: the compiled torch.library binding when it is built and loads (csrc/torch_binding.cpp), else the
# ctypes layer; both are thin shims over the same C ABI (there is no other compute path)
_impl = compiled if compiled.available() else ops


class DataType(enum.Enum):
    # numbering of the reference's Python enum (petit_kernel/__init__.py:8-15)
    int4 = 0
    float8_e4m3fn = 1
    float4_e2m1 = 2
    float16 = 3
    bfloat16 = 4
    float8_e5m2fn = 5
    mxfloat4_e2m1 = 6


# Round 3's extension value for PetitSolutionHints.b_type ("MXFP4 whose every e8m0 scale byte lies in 114..140"): still accepted, and means plain
# MXFP4 -- the fp16 x MXFP4 kernels test the range themselves (include/petit_amd.h), there is nothing to promise any more.
DTYPE_MXFP4_E2M1_F16RANGE = 8


def repack_nvfp4(qw: torch.Tensor, size_n: int, size_k: int) -> torch.Tensor:
    return _impl.repack_nvfp4(qw, size_n, size_k)


def process_nvfp4_scales(scales: torch.Tensor, size_n: int, size_k: int) -> torch.Tensor:
    return _impl.process_nvfp4_scales(scales, size_n, size_k)


def repack_mxfp4(qw: torch.Tensor, size_n: int, size_k: int) -> torch.Tensor:
    # weight packing is format-independent, as in the reference (:27-28)
    return _impl.repack_nvfp4(qw, size_n, size_k)


def process_mxfp4_scales(scales: torch.Tensor, size_n: int, size_k: int) -> torch.Tensor:
    # (no look at the values, no host sync, nothing attached to the tensor: the GEMM kernels decide per wave and span whether the scales they
    # hold allow the single-MFMA fp16 body -- nn.Parameter-wrapped, copied or overwritten scale tensors all get the right kernel)
    return _impl.process_mxfp4_scales(scales, size_n, size_k)


def hadamard_rotate(x: torch.Tensor, block: int, log2_scale: int = 0, out: torch.Tensor = None) -> torch.Tensor:
    # every row of x [..., k] times the unnormalised Hadamard block H_block (32 / 128) along k, times 2^log2_scale, rounded once to x's type
    # (include/petit_amd.h "Block-Hadamard rotation"); out may be x.  Host twin: offline.hadamard_rotate_cpu
    return _impl.hadamard_rotate(x, block, log2_scale, out)


def quantize_nvfp4(w: torch.Tensor, global_scale: torch.Tensor = None, hadamard: int = 0):
    # 16-bit weights [N, K] or [E, N, K] -> (b, s, global_scale) on the device (include/petit_amd.h "Weight quantiser"): the packed tensors
    # repack_nvfp4 / process_nvfp4_scales return for the stacked [E * N, K] tensor and float32 [E] global scales (amax / 2688 per expert, or the
    # caller's), for mul_nvfp4_a16, the MoE launches, fp4_moe* and nvfp4_native_image(s).  Host twin: offline.quantize_nvfp4_cpu
    # hadamard = 32 / 128: exactly quantize_nvfp4(hadamard_rotate(w, B, -log2 B)) -- the weights for activations quantised with the same hadamard
    return _impl.quantize_nvfp4(w, global_scale, hadamard)


def quantize_mxfp4(w: torch.Tensor, hadamard: int = 0):
    # the same for MXFP4 (one e8m0 scale per 32 k, global_scale = 1); num_experts * N must be a multiple of 32, as process_mxfp4_scales asks
    return _impl.quantize_mxfp4(w, hadamard)


def mxfp4_scales_in_fp16_range(raw_scales: torch.Tensor) -> bool:
    """A diagnostic, not an input of any call: True when every e8m0 byte of the RAW (unprocessed) MXFP4 scale tensor lies in 114..140, i.e. when
    fp16 activations run the single-MFMA body in every wave (a wave that meets a byte outside that range finishes its K range in the exact
    fallback body, which is slower).  Synchronises with the device."""
    if raw_scales.numel() == 0:
        return False
    lo, hi = torch.aminmax(raw_scales)
    return bool(int(lo) >= MXFP4_F16RANGE_SCALE_MIN and int(hi) <= MXFP4_F16RANGE_SCALE_MAX)


def mul_nvfp4_a16(a: torch.Tensor, b: torch.Tensor, s: torch.Tensor, global_scale: torch.Tensor,
                  size_m: int, size_n: int, size_k: int, solution_id: int = -1, *, bias: torch.Tensor = None,
                  activation: str = None) -> torch.Tensor:
    # `bias` / `activation` are extensions (keyword-only, default None = the reference's behaviour):
    #   bias       [size_n] of a.dtype, added before the single rounding to 16 bit
    #   activation "silu_mul": returns [size_m, size_n/2] = silu(y[:, :n/2]) * y[:, n/2:]  (gate_up of a gated MLP)
    #   activation "swiglu_oai": the same shape with gpt-oss's clamped form, g = min(gate, 7), u = clamp(up, -7, 7): g * sigmoid(1.702 g) * (u + 1)
    return _impl.mul_nvfp4_a16(a, b, s, global_scale, size_m, size_n, size_k, solution_id, bias, activation)


def mul_mxfp4_a16(a: torch.Tensor, b: torch.Tensor, s: torch.Tensor, global_scale: torch.Tensor,
                  size_m: int, size_n: int, size_k: int, solution_id: int = -1, *, bias: torch.Tensor = None,
                  activation: str = None, f16_range: bool = None) -> torch.Tensor:
    # fp16 activations are an extension (the reference's MXFP4 path takes bf16 only, gemm_fp4_fp16_grid.cc:55-64); any negative solution_id
    # is the library default as in the reference (fp4.cc:240) -- the native class is reached through mul_mxfp4_native only.
    # f16_range: round 3's promise "every block scale lies in 114..140"; ignored since round 4 (the kernels test it), accepted for one more round
    if f16_range is not None:
        import warnings
        warnings.warn("mul_mxfp4_a16(f16_range=...) is ignored: the fp16 x MXFP4 kernels test the scale range themselves", DeprecationWarning, stacklevel=2)
    return _impl.mul_mxfp4_a16(a, b, s, global_scale, size_m, size_n, size_k, solution_id, bias, activation)


def mul_nvfp4_a16_invariant(a: torch.Tensor, b: torch.Tensor, s: torch.Tensor, global_scale: torch.Tensor, size_m: int, size_n: int, size_k: int,
                            bias: torch.Tensor = None, activation: str = None) -> torch.Tensor:
    # mul_nvfp4_a16 by the batch-invariant entry (include/petit_amd.h "Batch-invariant GEMM"): every output row is a pure function of its
    # activation row, the weights, the scales and the bias -- the same bits alone (size_m = 1), inside any batch and at any position of it.
    # Opt-in: slower than the default pick (profiles/gemm_invariant.md), no solution_id (nothing is picked).  global_scale may be None.
    return _impl.mul_nvfp4_a16_invariant(a, b, s, global_scale, size_m, size_n, size_k, bias, activation)


def mul_mxfp4_a16_invariant(a: torch.Tensor, b: torch.Tensor, s: torch.Tensor, global_scale: torch.Tensor, size_m: int, size_n: int, size_k: int,
                            bias: torch.Tensor = None, activation: str = None) -> torch.Tensor:
    # the same for MXFP4 weights; bfloat16 activations only (float16 x MXFP4 has no batch-invariant kernel)
    return _impl.mul_mxfp4_a16_invariant(a, b, s, global_scale, size_m, size_n, size_k, bias, activation)


def invariant_geometry(size_n: int, size_k: int, dtype: torch.dtype = torch.bfloat16, kind: str = "nvfp4"):
    # (S, L): the slices of K whose partial sums the batch-invariant GEMM adds in order -- functions of (n, k, types) alone
    return ops.invariant_geometry(size_n, size_k, dtype, kind)


def invariant_slabs(size_m: int, size_n: int, size_k: int, dtype: torch.dtype = torch.bfloat16, kind: str = "nvfp4") -> int:
    # S when size_m rows run in the split form (two launches, slabs in scratch), 1 in the whole form
    return ops.invariant_slabs(size_m, size_n, size_k, dtype, kind)


def invariant_workspace_bytes(size_m: int, size_n: int, size_k: int, dtype: torch.dtype = torch.bfloat16, kind: str = "nvfp4") -> int:
    # bytes of scratch the batch-invariant call allocates per call (the Python layers do it themselves); 0 in the whole form
    return ops.invariant_workspace_bytes(size_m, size_n, size_k, dtype, kind)


def mul_mxfp4_native_invariant(a, b: torch.Tensor, s: torch.Tensor, global_scale: torch.Tensor, size_m: int, size_n: int, size_k: int,
                               fmt: str = "mxfp8", bias: torch.Tensor = None, activation: str = None) -> torch.Tensor:
    # the native class (MXFP4 weights on the block-scaled MFMA, activations quantised to fmt) by its batch-invariant entry (include/petit_amd.h
    # "Batch-invariant GEMM on the native class"): the same bits for a row alone, in any batch and at any position.  a: a 16-bit tensor
    # (quantised by the call) or QuantizedActivations of the same fmt (quantize_activations / rmsnorm_quantize) -- the same bits either way.
    return _impl.mul_mxfp4_native_invariant(a, b, s, global_scale, size_m, size_n, size_k, fmt, bias, activation)


def native_invariant_slabs(size_m: int, size_n: int, size_k: int, dtype: torch.dtype = torch.bfloat16) -> int:
    # S when size_m rows run in the split form (two launches, slabs in scratch), 1 in the whole form
    return ops.native_invariant_slabs(size_m, size_n, size_k, dtype)


def native_invariant_workspace_bytes(size_m: int, size_n: int, size_k: int, dtype: torch.dtype = torch.bfloat16, fmt: str = "mxfp8",
                                     quantized: bool = False) -> int:
    # bytes of scratch the call allocates per call: the quantised bytes of a 16-bit input plus the split form's slabs
    return ops.native_invariant_workspace_bytes(size_m, size_n, size_k, dtype, fmt, quantized)


def mul_nvfp4_a16_moe_invariant(a: torch.Tensor, b: torch.Tensor, s: torch.Tensor, global_scales: torch.Tensor, expert_offsets: torch.Tensor,
                                size_m: int, size_n: int, size_k: int, num_experts: int, a_row_index: torch.Tensor = None,
                                c_row_index: torch.Tensor = None, c_rows: int = None, bias: torch.Tensor = None, activation: str = None,
                                out: torch.Tensor = None) -> torch.Tensor:
    # mul_nvfp4_a16_moe_indexed by the batch-invariant entry (include/petit_amd.h "Batch-invariant MoE launch"): every written row equals,
    # bit for bit, mul_nvfp4_a16_invariant(size_m=1) on its A row with its expert's tensors, global scale and bias -- whatever the batch,
    # the routing and the row's position.  Opt-in: slower than the default pick (profiles/moe_invariant.md), no solution_id.
    return _impl.mul_nvfp4_a16_moe_invariant(a, b, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index,
                                             c_rows, bias, activation, out)


def mul_mxfp4_a16_moe_invariant(a: torch.Tensor, b: torch.Tensor, s: torch.Tensor, global_scales: torch.Tensor, expert_offsets: torch.Tensor,
                                size_m: int, size_n: int, size_k: int, num_experts: int, a_row_index: torch.Tensor = None,
                                c_row_index: torch.Tensor = None, c_rows: int = None, bias: torch.Tensor = None, activation: str = None,
                                out: torch.Tensor = None) -> torch.Tensor:
    # the same for MXFP4 experts; bfloat16 activations only
    return _impl.mul_mxfp4_a16_moe_invariant(a, b, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index,
                                             c_rows, bias, activation, out)


def mul_mxfp4_native_moe_invariant(a, b: torch.Tensor, s: torch.Tensor, global_scales: torch.Tensor, expert_offsets: torch.Tensor, size_m: int,
                                   size_n: int, size_k: int, num_experts: int, a_row_index: torch.Tensor = None,
                                   c_row_index: torch.Tensor = None, c_rows: int = None, fmt: str = "mxfp8", bias: torch.Tensor = None,
                                   activation: str = None) -> torch.Tensor:
    # the native class's routed-expert launch by its batch-invariant entry (include/petit_amd.h "Batch-invariant MoE launch on the native
    # class"): every written row equals, bit for bit, mul_mxfp4_native_invariant(size_m=1) on its row with its expert's tensors, global scale
    # and bias.  a: a 16-bit [a_rows, size_k] tensor (gathered and quantised by the call) or QuantizedActivations of the size_m grouped rows
    # (quantize_activation_rows) -- the same bits either way.  Opt-in (profiles/native_moe_invariant.md), no solution_id.
    return _impl.mul_mxfp4_native_moe_invariant(a, b, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index,
                                                c_row_index, c_rows, fmt, bias, activation)


def native_moe_invariant_form(size_m: int, num_experts: int) -> int:
    # the form a native-class batch-invariant MoE call gets: 1 split, 0 whole -- a function of these two arguments alone
    return ops.native_moe_invariant_form(size_m, num_experts)


def native_moe_invariant_workspace_bytes(num_experts: int, size_m: int, size_n: int, size_k: int, dtype: torch.dtype = torch.bfloat16,
                                         fmt: str = "mxfp8", quantized: bool = False) -> int:
    # bytes of scratch the call allocates per call: the quantised bytes of a 16-bit input plus the split form's slabs
    return ops.native_moe_invariant_workspace_bytes(num_experts, size_m, size_n, size_k, dtype, fmt, quantized)


def mul_nvfp4_native_invariant(a, image: torch.Tensor, global_scale: torch.Tensor, size_m: int, size_n: int, size_k: int, fmt: str = "mxfp8",
                               bias: torch.Tensor = None, activation: str = None) -> torch.Tensor:
    # mul_mxfp4_native_invariant for NVFP4 weights on their native image (nvfp4_native_image; include/petit_amd.h "Batch-invariant native-class
    # GEMM and MoE launch on NVFP4 images"): the same bits for a row alone, in any batch and at any position.  native_invariant_slabs and
    # native_invariant_workspace_bytes answer for it too.  Opt-in (profiles/nvfp4_native_invariant.md), no solution_id.
    return _impl.mul_nvfp4_native_invariant(a, image, global_scale, size_m, size_n, size_k, fmt, bias, activation)


def mul_nvfp4_native_moe_invariant(a, images: torch.Tensor, global_scales: torch.Tensor, expert_offsets: torch.Tensor, size_m: int, size_n: int,
                                   size_k: int, num_experts: int, a_row_index: torch.Tensor = None, c_row_index: torch.Tensor = None,
                                   c_rows: int = None, fmt: str = "mxfp8", bias: torch.Tensor = None, activation: str = None) -> torch.Tensor:
    # the routed-expert launch of the same on the experts' images (nvfp4_native_images): every written row equals, bit for bit,
    # mul_nvfp4_native_invariant(size_m=1) on its row with its expert's image, global scale and bias
    return _impl.mul_nvfp4_native_moe_invariant(a, images, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index,
                                                c_row_index, c_rows, fmt, bias, activation)


def moe_invariant_form(size_m: int, num_experts: int) -> int:
    # the form a batch-invariant MoE call gets: 1 split (slabs in scratch, two launches), 0 whole -- a function of these two arguments alone
    return ops.moe_invariant_form(size_m, num_experts)


def moe_invariant_workspace_bytes(num_experts: int, size_m: int, size_n: int, size_k: int, dtype: torch.dtype = torch.bfloat16,
                                  kind: str = "nvfp4") -> int:
    # bytes of scratch the batch-invariant MoE call allocates per call (the Python layers do it themselves); 0 in the whole form
    return ops.moe_invariant_workspace_bytes(num_experts, size_m, size_n, size_k, dtype, kind)


def mul_nvfp4_a16_moe(a: torch.Tensor, b: torch.Tensor, s: torch.Tensor, global_scales: torch.Tensor, expert_offsets: torch.Tensor,
                      size_m: int, size_n: int, size_k: int, num_experts: int, solution_id: int = -1, bias: torch.Tensor = None,
                      activation: str = None) -> torch.Tensor:
    # all experts of a MoE layer in one launch (include/petit_amd.h "Routed-expert (MoE) launch"): rows expert_offsets[e] .. expert_offsets[e+1]-1
    # of `a` (grouped by expert, int32 [E + 1] on the GPU, never read by the host) times expert e's weights; b / s hold the experts' packed
    # tensors back to back, global_scales is float32 [E], bias [E, size_n]; activation "silu_mul" takes each expert's weight as [gate; up]
    return _impl.mul_nvfp4_a16_moe(a, b, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, solution_id, bias, activation)


def mul_mxfp4_a16_moe(a: torch.Tensor, b: torch.Tensor, s: torch.Tensor, global_scales: torch.Tensor, expert_offsets: torch.Tensor,
                      size_m: int, size_n: int, size_k: int, num_experts: int, solution_id: int = -1, bias: torch.Tensor = None,
                      activation: str = None) -> torch.Tensor:
    return _impl.mul_mxfp4_a16_moe(a, b, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, solution_id, bias, activation)


def mul_nvfp4_a16_moe_indexed(a: torch.Tensor, b: torch.Tensor, s: torch.Tensor, global_scales: torch.Tensor, expert_offsets: torch.Tensor,
                              size_m: int, size_n: int, size_k: int, num_experts: int, a_row_index: torch.Tensor = None,
                              c_row_index: torch.Tensor = None, c_rows: int = None, solution_id: int = -1, bias: torch.Tensor = None,
                              activation: str = None, out: torch.Tensor = None) -> torch.Tensor:
    # the MoE launch on gathered rows of `a` ([a_rows, size_k]: grouped row r reads a[a_row_index[r]]) writing scattered rows of the output
    # ([c_rows, n_out]: grouped row r writes row c_row_index[r]); None is the identity; int32 [size_m] device indices, never read by the host.
    # An index outside the matrix reads zeros / stores nothing.  out: write into this tensor (rows no index names stay untouched).
    return _impl.mul_nvfp4_a16_moe_indexed(a, b, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index,
                                           c_rows, solution_id, bias, activation, out)


def mul_mxfp4_a16_moe_indexed(a: torch.Tensor, b: torch.Tensor, s: torch.Tensor, global_scales: torch.Tensor, expert_offsets: torch.Tensor,
                              size_m: int, size_n: int, size_k: int, num_experts: int, a_row_index: torch.Tensor = None,
                              c_row_index: torch.Tensor = None, c_rows: int = None, solution_id: int = -1, bias: torch.Tensor = None,
                              activation: str = None, out: torch.Tensor = None) -> torch.Tensor:
    return _impl.mul_mxfp4_a16_moe_indexed(a, b, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index,
                                           c_rows, solution_id, bias, activation, out)


def moe_align_device(topk_ids: torch.Tensor, num_experts: int):
    # moe_align on the device: (sorted_pos, expert_offsets, token_index), int32; ids outside [0, E) are not routed
    return _impl.moe_align_device(topk_ids, num_experts)


def moe_combine(slot_out: torch.Tensor, topk_weights: torch.Tensor, topk_ids: torch.Tensor, num_experts: int) -> torch.Tensor:
    # the deterministic top-k reduce of a MoE layer (fp32, fixed order, no FMA contraction, one RNE rounding)
    return _impl.moe_combine(slot_out, topk_weights, topk_ids, num_experts)


def moe_combine_rmsnorm(slot_out: torch.Tensor, topk_weights: torch.Tensor, topk_ids: torch.Tensor, num_experts: int, weight: torch.Tensor,
                        eps: float = 1e-6, fmt: str = None, *, residual: torch.Tensor = None, weight_offset: float = 0.0,
                        return_normed: bool = None, return_hidden: bool = None, inplace_residual: bool = False):
    # moe_combine, the residual add, the RMSNorm and (with fmt) quantize_activations in ONE launch (include/petit_amd.h "Top-k combine into the
    # norm"; ops.moe_combine_rmsnorm has the return convention): the end of a routed-expert layer and the head of the next block
    return _impl.moe_combine_rmsnorm(slot_out, topk_weights, topk_ids, num_experts, weight, eps, fmt, residual=residual,
                                     weight_offset=weight_offset, return_normed=return_normed, return_hidden=return_hidden,
                                     inplace_residual=inplace_residual)


def _no_slots(expert_map, num_local_experts, num_shared, shared_weight, shared_gate_logits) -> bool:
    # every slot-list argument of moe_route / moe_route_align at its default: the call is the plain route
    return expert_map is None and num_local_experts is None and num_shared == 0 and shared_weight == 1.0 and shared_gate_logits is None


def moe_route(router_logits: torch.Tensor, topk: int, *, scoring: str = "softmax", renormalize: bool = True, bias: torch.Tensor = None,
              n_group: int = 1, topk_group: int = 1, routed_scaling_factor: float = 1.0, return_keys: bool = False,
              expert_map: torch.Tensor = None, num_local_experts: int = None, num_shared: int = 0, shared_weight: float = 1.0,
              shared_gate_logits: torch.Tensor = None):
    # router logits [T, E] (float32 / bfloat16 / float16) -> (topk_weights float32, topk_ids int32[, keys float32 [T, E]]) in one launch
    # (include/petit_amd.h "Routing on the device, from the router's logits").  scoring "softmax" (Mixtral, Qwen3-MoE, gpt-oss with renormalize)
    # or "sigmoid" (DeepSeek-V3: bias = e_score_correction_bias, n_group / topk_group, routed_scaling_factor).  Larger key first, the LOWER index
    # among equal keys: a routing is a pure function of the logits.
    # The complete slot list of a layer with expert parallelism and shared experts, in the same launch (include/petit_amd.h "The complete slot
    # list in the route launch"): expert_map int32 [E] maps the selected global ids to local ones (a value outside [0, num_local_experts) is
    # written as -1; the weights stay those of the global selection); num_shared appends slots with ids num_local_experts + s and weight
    # shared_weight (0 is read as 1), times sigmoid(shared_gate_logits[t, s]) when given ([T, num_shared], router_logits' dtype).  Outputs are
    # then [T, topk + num_shared]
    if _no_slots(expert_map, num_local_experts, num_shared, shared_weight, shared_gate_logits):
        return _impl.moe_route(router_logits, topk, scoring, renormalize, bias, n_group, topk_group, routed_scaling_factor, return_keys)
    return _impl.moe_route_ex(router_logits, topk, scoring, renormalize, bias, n_group, topk_group, routed_scaling_factor, return_keys,
                              expert_map, num_local_experts, num_shared, shared_weight, shared_gate_logits)


def moe_route_align(router_logits: torch.Tensor, topk: int, *, scoring: str = "softmax", renormalize: bool = True, bias: torch.Tensor = None,
                    n_group: int = 1, topk_group: int = 1, routed_scaling_factor: float = 1.0, return_keys: bool = False,
                    expert_map: torch.Tensor = None, num_local_experts: int = None, num_shared: int = 0, shared_weight: float = 1.0,
                    shared_gate_logits: torch.Tensor = None):
    # moe_route, then moe_align_device on its ids, bit for bit: (topk_weights, topk_ids, sorted_pos, expert_offsets, token_index[, keys]);
    # ONE launch when T * topk <= 1024, four above.  With moe_route's slot-list arguments: the align of the T * (topk + num_shared) slots over
    # num_local_experts + num_shared experts, ONE launch when T * (topk + num_shared) <= 1024
    if _no_slots(expert_map, num_local_experts, num_shared, shared_weight, shared_gate_logits):
        return _impl.moe_route_align(router_logits, topk, scoring, renormalize, bias, n_group, topk_group, routed_scaling_factor, return_keys)
    return _impl.moe_route_align_ex(router_logits, topk, scoring, renormalize, bias, n_group, topk_group, routed_scaling_factor, return_keys,
                                    expert_map, num_local_experts, num_shared, shared_weight, shared_gate_logits)


def moe_router_logits(hidden: torch.Tensor, router_weight: torch.Tensor, router_bias: torch.Tensor = None) -> torch.Tensor:
    # the router's linear: hidden [T, K] . router_weight [E, K]^T (+ router_bias float32 [E]) -> float32 [T, E] (include/petit_amd.h "The
    # router's GEMM").  bfloat16 or float16, both alike, contiguous, the weight as the checkpoint stores it.  fp32 accumulation in an order that
    # (E, K) alone fix: a token's logits -- and so its experts -- do not depend on the batch it sits in
    return _impl.moe_router_logits(hidden, router_weight, router_bias)


def moe_route_hidden(hidden: torch.Tensor, router_weight: torch.Tensor, topk: int, *, router_bias: torch.Tensor = None, align: bool = True,
                     scoring: str = "softmax", renormalize: bool = True, bias: torch.Tensor = None, n_group: int = 1, topk_group: int = 1,
                     routed_scaling_factor: float = 1.0, return_keys: bool = False, expert_map: torch.Tensor = None,
                     num_local_experts: int = None, num_shared: int = 0, shared_weight: float = 1.0, shared_gate_logits: torch.Tensor = None):
    # the routing from the hidden state: what moe_route_align (align=True) or moe_route (align=False) return on
    # moe_router_logits(hidden, router_weight, router_bias), bit for bit, without the logits being stored: TWO launches for a decode batch
    # (the router GEMM, then route + align on its partial sums).  `bias` is the sigmoid scoring's correction bias, `router_bias` the linear's own;
    # shared_gate_logits is float32 [T, num_shared] here
    return _impl.moe_route_hidden(hidden, router_weight, topk, router_bias, align, scoring, renormalize, bias, n_group, topk_group,
                                  routed_scaling_factor, return_keys, expert_map, num_local_experts, num_shared, shared_weight,
                                  shared_gate_logits)


def mul_mxfp4_native_moe(a, b: torch.Tensor, s: torch.Tensor, global_scales: torch.Tensor, expert_offsets: torch.Tensor, size_m: int, size_n: int,
                         size_k: int, num_experts: int, a_row_index: torch.Tensor = None, c_row_index: torch.Tensor = None, c_rows: int = None,
                         solution_id: int = SOLUTION_AUTO_NATIVE_MXFP8, bias: torch.Tensor = None, activation: str = None, out_quantized: str = None):
    # the MoE launch on the native class (include/petit_amd.h "Native-class MoE launch"): `a` 16-bit [a_rows, size_k] (gathered through
    # a_row_index, quantised by the call) or QuantizedActivations of the size_m grouped rows; solution_id a native sentinel or a native id with
    # a MoE form; out_quantized (activation "silu_mul") returns the grouped rows quantised for the next launch
    return _impl.mul_mxfp4_native_moe(a, b, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index, c_rows,
                                      solution_id, bias, activation, out_quantized)


def mul_nvfp4_native_moe(a, images: torch.Tensor, global_scales: torch.Tensor, expert_offsets: torch.Tensor, size_m: int, size_n: int, size_k: int,
                         num_experts: int, a_row_index: torch.Tensor = None, c_row_index: torch.Tensor = None, c_rows: int = None,
                         solution_id: int = SOLUTION_AUTO_NATIVE_MXFP8, bias: torch.Tensor = None, activation: str = None, out_quantized: str = None):
    # NVFP4 experts on the native class: `images` = nvfp4_native_images of the stacked packed tensors (E images back to back)
    return _impl.mul_nvfp4_native_moe(a, images, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index, c_rows,
                                      solution_id, bias, activation, out_quantized)


def mul_nvfp4_native_moe_transient(a, b: torch.Tensor, s: torch.Tensor, global_scales: torch.Tensor, expert_offsets: torch.Tensor, size_m: int,
                                   size_n: int, size_k: int, num_experts: int, a_row_index: torch.Tensor = None, c_row_index: torch.Tensor = None,
                                   c_rows: int = None, solution_id: int = SOLUTION_AUTO_NATIVE_MXFP8, bias: torch.Tensor = None,
                                   activation: str = None, out_quantized: str = None, workspace: torch.Tensor = None):
    # NVFP4 experts on the native class WITHOUT resident images (include/petit_amd.h "Without resident images"): b / s are the stacked packed
    # tensors of mul_nvfp4_a16_moe; each call builds the images of the experts that have rows into a per-call workspace (one launch) and runs on
    # them -- bit for bit mul_nvfp4_native_moe on nvfp4_native_images(b, s, ...).  workspace: the caller's scratch instead (uint8, at least
    # nvfp4_native_moe_transient_workspace_bytes), which several calls may share one after the other
    return _impl.mul_nvfp4_native_moe_transient(a, b, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index,
                                                c_row_index, c_rows, solution_id, bias, activation, out_quantized, workspace)


def nvfp4_native_moe_transient_workspace_bytes(num_experts: int, size_m: int, size_n: int, size_k: int,
                                               solution_id: int = SOLUTION_AUTO_NATIVE_MXFP8, dtype: torch.dtype = torch.bfloat16,
                                               activation: str = None, a_format: str = None, out_quantized: str = None) -> int:
    # the per-call workspace of mul_nvfp4_native_moe_transient: num_experts images, then the native launch's own scratch
    return ops.nvfp4_native_moe_transient_workspace_bytes(num_experts, size_m, size_n, size_k, solution_id, dtype, activation, a_format,
                                                          out_quantized)


def mul_nvfp4_native_transient(a, b: torch.Tensor, s: torch.Tensor, global_scale: torch.Tensor, size_m: int, size_n: int, size_k: int,
                               solution_id: int = SOLUTION_AUTO_NATIVE_MXFP8, bias: torch.Tensor = None, activation: str = None,
                               out_quantized: str = None):
    # NVFP4 weights on the native class WITHOUT a resident image (include/petit_amd.h "Without a resident image"): b / s are the packed tensors of
    # mul_nvfp4_a16; each call builds the image into a per-call workspace and runs on it -- bit for bit mul_nvfp4_a16(..., -2 / -3 / -4) with the image
    # attached, or mul_nvfp4_native on the image; `a` a 16-bit tensor or QuantizedActivations
    return _impl.mul_nvfp4_native_transient(a, b, s, global_scale, size_m, size_n, size_k, solution_id, bias, activation, out_quantized)


def nvfp4_native_transient_workspace_bytes(size_m: int, size_n: int, size_k: int, solution_id: int = SOLUTION_AUTO_NATIVE_MXFP8,
                                           dtype: torch.dtype = torch.bfloat16, activation: str = None, a_format: str = None,
                                           out_quantized: str = None) -> int:
    # the per-call workspace of mul_nvfp4_native_transient: the image (rounded up to 256 bytes), then the native call's own scratch
    return ops.nvfp4_native_transient_workspace_bytes(size_m, size_n, size_k, solution_id, dtype, activation, a_format, out_quantized)


def quantize_activation_rows(a: torch.Tensor, fmt: str = "mxfp8", row_index: torch.Tensor = None, rows: int = None,
                             hadamard: int = 0) -> QuantizedActivations:
    # quantize_activations of the rows row_index names (None: all rows); an index outside the matrix gives a zero row
    return ops.quantize_activation_rows(a, fmt, row_index, rows, hadamard)


def native_moe_resolve_solution(hints: PetitSolutionHints, num_experts: int, size_m: int, size_n: int, size_k: int,
                                solution_id: int = SOLUTION_AUTO_NATIVE_MXFP8, activation: str = None, a_format: str = None,
                                out_quantized: str = None) -> int:
    return ops.native_moe_resolve_solution(hints, num_experts, size_m, size_n, size_k, solution_id, activation, a_format, out_quantized)


def moe_resolve_solution(hints: PetitSolutionHints, num_experts: int, size_m: int, size_n: int, size_k: int, solution_id: int = -1,
                         activation: str = None) -> int:
    return ops.moe_resolve_solution(hints, num_experts, size_m, size_n, size_k, solution_id, activation)


def get_fp4_solutions(size_m: int, size_n: int, size_k: int, a_type, c_type) -> list:
    return ops.get_fp4_solutions(size_m, size_n, size_k, a_type, c_type)


__all__ = [
    "repack_nvfp4",
    "repack_mxfp4",
    "process_nvfp4_scales",
    "process_mxfp4_scales",
    "quantize_nvfp4",
    "quantize_mxfp4",
    "hadamard_rotate",
    "mul_nvfp4_a16",
    "mul_mxfp4_a16",
    "mul_nvfp4_a16_invariant",
    "mul_mxfp4_a16_invariant",
    "invariant_geometry",
    "invariant_slabs",
    "invariant_workspace_bytes",
    "mul_mxfp4_native_invariant",
    "native_invariant_slabs",
    "native_invariant_workspace_bytes",
    "mul_nvfp4_a16_moe_invariant",
    "mul_mxfp4_a16_moe_invariant",
    "moe_invariant_form",
    "moe_invariant_workspace_bytes",
    "mul_mxfp4_native_moe_invariant",
    "mul_nvfp4_native_invariant",
    "mul_nvfp4_native_moe_invariant",
    "native_moe_invariant_form",
    "native_moe_invariant_workspace_bytes",
    "get_fp4_solutions",
    "mxfp4_scales_in_fp16_range",
    "DataType",
    "PetitSolutionHints",
    "tune",
    "tune_tensors",
    "quantize_activations",
    "rmsnorm_quantize",
    "mul_fp4_a16_grouped",
    "mul_nvfp4_a16_moe",
    "mul_mxfp4_a16_moe",
    "moe_resolve_solution",
    "moe_align",
    "fp4_moe",
    "fp4_moe_fused",
    "mul_nvfp4_a16_moe_indexed",
    "mul_mxfp4_a16_moe_indexed",
    "moe_align_device",
    "moe_combine",
    "moe_combine_rmsnorm",
    "moe_route",
    "moe_route_align",
    "moe_router_logits",
    "moe_route_hidden",
    "fp4_moe_routed",
    "fp4_moe_native",
    "mul_mxfp4_native_moe",
    "mul_nvfp4_native_moe",
    "quantize_activation_rows",
    "nvfp4_native_images",
    "native_moe_resolve_solution",
    "mul_mxfp4_native",
    "nvfp4_native_image",
    "attach_nvfp4_native",
    "mul_nvfp4_native",
    "mul_nvfp4_native_transient",
    "mul_nvfp4_native_moe_transient",
    "nvfp4_native_moe_transient_workspace_bytes",
    "nvfp4_native_transient_workspace_bytes",
    "QuantizedActivations",
    "SOLUTION_AUTO",
    "SOLUTION_AUTO_NATIVE_MXFP8",
    "SOLUTION_AUTO_NATIVE_MXFP4",
    "SOLUTION_AUTO_NATIVE_MXFP6",
    "prepare_gptoss_experts",
    "GptOssExperts",
]

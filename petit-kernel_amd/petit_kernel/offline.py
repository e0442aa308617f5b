"""petit_kernel.offline -- checkpoint-side format tooling.

Convert the native NVFP4 / MXFP4 tensors of a checkpoint into the packed gfx950 layout on the CPU,
so the load-time GPU repack (`repack_nvfp4`, `process_*_scales`) becomes optional: the outputs are
bit-identical to what those produce on the device (tests/test_layout_and_abi.py,
tests/test_gpu_parity.py::test_offline_repack_matches_device) and can be saved with the
checkpoint and copied to the GPU as they are.  The reference has no counterpart: its repack exists
only as GPU kernels (quantization_utils.cu:208-304).

This is format tooling, not a CPU fallback: only the GPU kernels consume the packed tensors.
"""
import torch

from . import _lib
from .ops import _B_TYPES, _LAYOUT_M, _LAYOUT_N, _PACK, _QFORMATS, _a_type, _check, _opt_ptr, _ptr, _quantize_operands, _quantize_outputs, _raise_on
from .ops import _raise_quantize, _rmsnorm_operands, _rmsnorm_outputs, _rmsnorm_result
from .ops import QuantizedActivations, _HADAMARD_FP6, _hadamard_block, _hadamard_operands, _rotated_weights
from .ops import _combine_norm_operands, _combine_norm_outputs, _combine_norm_result, _combine_norm_returns


def _cpu(t: torch.Tensor, name: str) -> None:
    _check(not t.is_cuda, f"{name} must be a CPU tensor (use petit_kernel.repack_* for GPU tensors)")
    _check(t.is_contiguous(), f"{name} is not contiguous")


def repack_nvfp4_cpu(qw: torch.Tensor, size_n: int, size_k: int) -> torch.Tensor:
    """CPU twin of repack_nvfp4 / repack_mxfp4: int32 [N, K/8] -> int32 [N/16, 2K]."""
    _check(size_k % _LAYOUT_M == 0, f"size_k = {size_k} is not divisible by tile_k_size = {_LAYOUT_M}")
    _check(size_n % _LAYOUT_N == 0, f"size_n = {size_n} is not divisible by tile_n_size = {_LAYOUT_N}")
    _check(qw.dim() == 2 and qw.size(0) == size_n and qw.size(1) == size_k // _PACK,
           f"qw must be [size_n, size_k / {_PACK}]")
    _check(qw.dtype == torch.int32, "qw type is not kInt")
    _cpu(qw, "qw")
    out = torch.empty((size_n // _LAYOUT_N, size_k * _LAYOUT_N // _PACK), dtype=torch.int32)
    _raise_on(_lib.lib.petit_repack_nvfp4_weights_host(out.data_ptr(), qw.data_ptr(), size_k, size_n), "repack_nvfp4_cpu")
    return out


repack_mxfp4_cpu = repack_nvfp4_cpu


def process_nvfp4_scales_cpu(scales: torch.Tensor, size_n: int, size_k: int) -> torch.Tensor:
    """CPU twin of process_nvfp4_scales: e4m3 [N, K/16] -> e4m3 [N, K/16]."""
    _check(size_k % (2 * _LAYOUT_M) == 0, f"size_k = {size_k} is not divisible by tile_k_size = {2 * _LAYOUT_M}")
    _check(size_n % _LAYOUT_N == 0, f"size_n = {size_n} is not divisible by tile_n_size = {_LAYOUT_N}")
    _check(scales.dim() == 2 and scales.size(0) == size_n and scales.size(1) * 16 == size_k,
           "Only groupsize = 16 is supported.")
    _check(scales.dtype == torch.float8_e4m3fn, "scales type is not float8_e4m3fn")
    _cpu(scales, "scales")
    out = torch.empty_like(scales)
    _raise_on(_lib.lib.petit_repack_nvfp4_scales_host(out.data_ptr(), scales.data_ptr(), size_k, size_n),
              "process_nvfp4_scales_cpu")
    return out


def process_mxfp4_scales_cpu(scales: torch.Tensor, size_n: int, size_k: int) -> torch.Tensor:
    """CPU twin of process_mxfp4_scales: e8m0 uint8 [N, K/32] -> uint8 [N/32, K]."""
    _check(size_k % (2 * _LAYOUT_M) == 0, f"size_k = {size_k} is not divisible by tile_k_size = {2 * _LAYOUT_M}")
    _check(size_n % 32 == 0, f"size_n = {size_n} is not divisible by 32")
    _check(scales.dim() == 2 and scales.size(0) == size_n and scales.size(1) * 32 == size_k,
           "Only groupsize = 32 is supported.")
    _check(scales.dtype == torch.uint8, "scales type is not uint8")
    _cpu(scales, "scales")
    out = torch.empty((size_n // 32, size_k), dtype=torch.uint8)
    _raise_on(_lib.lib.petit_repack_mxfp4_scales_host(out.data_ptr(), scales.data_ptr(), size_k, size_n),
              "process_mxfp4_scales_cpu")
    return out


# --- 16-bit weights -> the packed tensors, offline (include/petit_amd.h "Weight quantiser") ------------------------------------------------------

def _quantize_weights_cpu(kind: str, w: torch.Tensor, global_scale=None):
    E, n, k = _quantize_operands(kind, w, global_scale, on_gpu=False)
    b, s, gs = _quantize_outputs(kind, E, n, k, w.device)
    rc = _lib.lib.petit_quantize_weights_host(w.data_ptr(), _a_type(w.dtype), _B_TYPES[kind], E, n, k,
                                              None if global_scale is None else global_scale.data_ptr(), b.data_ptr(), s.data_ptr(), gs.data_ptr())
    _raise_quantize(rc, "quantize_%sfp4_cpu" % kind, E, n, k)
    return b, s, gs


def hadamard_rotate_cpu(x: torch.Tensor, block: int, log2_scale: int = 0, out: torch.Tensor = None) -> torch.Tensor:
    """CPU twin of petit_kernel.hadamard_rotate (petit_hadamard_rows_host): the same arguments on CPU tensors, the same bits."""
    rows, k, out = _hadamard_operands(x, block, log2_scale, out, on_gpu=False)
    _raise_on(_lib.lib.petit_hadamard_rows_host(_ptr(out), _ptr(x), rows, k, _a_type(x.dtype), int(block), int(log2_scale)), "hadamard_rotate_cpu")
    return out


def quantize_nvfp4_cpu(w: torch.Tensor, global_scale: torch.Tensor = None, hadamard: int = 0):
    """CPU twin of petit_kernel.quantize_nvfp4: bf16 / fp16 [N, K] or [E, N, K] -> (b, s, global_scale), bit-identical to the device's."""
    return _quantize_weights_cpu("nv", _rotated_weights(w, hadamard, hadamard_rotate_cpu), global_scale)


def quantize_mxfp4_cpu(w: torch.Tensor, hadamard: int = 0):
    """CPU twin of petit_kernel.quantize_mxfp4."""
    return _quantize_weights_cpu("mx", _rotated_weights(w, hadamard, hadamard_rotate_cpu))


# --- the activation quantiser, on the CPU (petit_quantize_activations_host / _rot_host) -------------------------------------------------------------

def quantize_activations_cpu(a: torch.Tensor, fmt: str = "mxfp4", hadamard: int = 0) -> QuantizedActivations:
    """CPU twin of petit_kernel.quantize_activations: the same arguments on a CPU tensor, the same bytes."""
    _check(fmt in _QFORMATS, "fmt must be 'mxfp8', 'mxfp6' or 'mxfp4'")
    _check(_hadamard_block(hadamard) == 0 or fmt != "mxfp6", _HADAMARD_FP6)
    _check(not a.is_cuda and a.is_contiguous() and a.dim() == 2 and a.dtype in (torch.bfloat16, torch.float16),
           "a must be a contiguous 2-D bfloat16 / float16 CPU tensor")
    m, k = a.shape
    qa = torch.empty(int(_lib.lib.petit_quantized_activation_bytes(m, k, _QFORMATS[fmt])), dtype=torch.uint8)
    rc = _lib.lib.petit_quantize_activations_rot_host(_ptr(qa), _ptr(a), m, k, _a_type(a.dtype), _QFORMATS[fmt], hadamard)
    if rc == _lib.PETIT_ERROR_PROBLEM_SHAPE:
        raise RuntimeError(f"Incompatible problem shape (m={m}, k={k})")
    _raise_on(rc, "quantize_activations_cpu")
    return QuantizedActivations(qa, m, k, fmt, a.dtype, hadamard)


# --- RMSNorm into quantised activations, on the CPU (include/petit_amd.h "RMSNorm into quantised activations") ----------------------------------

def rmsnorm_quantize_cpu(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6, fmt: str = "mxfp8", *, residual: torch.Tensor = None,
                         weight_offset: float = 0.0, return_normed: bool = False, inplace_residual: bool = False, hadamard: int = 0):
    """CPU twin of petit_kernel.rmsnorm_quantize (the C ABI's host twin): the same arguments on CPU tensors, the same results bit for bit."""
    m, k = _rmsnorm_operands(x, weight, eps, fmt, residual, weight_offset, on_gpu=False, hadamard=hadamard)
    qa, res_out, y16 = _rmsnorm_outputs(x, fmt, residual, return_normed, inplace_residual)
    rc = _lib.lib.petit_rmsnorm_quantize_rot_host(_ptr(qa), _opt_ptr(y16), _opt_ptr(res_out), _ptr(x), _opt_ptr(residual), _ptr(weight),
                                                  float(eps), float(weight_offset), m, k, _a_type(x.dtype), _QFORMATS[fmt], hadamard)
    return _rmsnorm_result(rc, "rmsnorm_quantize_cpu", x, fmt, qa, res_out, y16, hadamard)


def moe_combine_rmsnorm_cpu(slot_out: torch.Tensor, topk_weights: torch.Tensor, topk_ids: torch.Tensor, num_experts: int, weight: torch.Tensor,
                            eps: float = 1e-6, fmt: str = None, *, residual: torch.Tensor = None, weight_offset: float = 0.0,
                            return_normed: bool = None, return_hidden: bool = None, inplace_residual: bool = False):
    """CPU twin of petit_kernel.moe_combine_rmsnorm (the C ABI's host twin): the same arguments on CPU tensors, the same results bit for bit."""
    T, topk, k = _combine_norm_operands(slot_out, topk_weights, topk_ids, num_experts, weight, eps, fmt, residual, weight_offset, on_gpu=False)
    want_h, want_y = _combine_norm_returns(fmt, residual, return_normed, return_hidden, inplace_residual)
    qa, res_out, y16 = _combine_norm_outputs(slot_out, T, k, fmt, residual, want_h, want_y, inplace_residual)
    rc = _lib.lib.petit_moe_combine_rmsnorm_host(_opt_ptr(qa), _opt_ptr(y16), _opt_ptr(res_out), _ptr(slot_out), _ptr(topk_weights),
                                                 _ptr(topk_ids), int(topk_ids.dtype == torch.int64), _opt_ptr(residual), _ptr(weight), float(eps),
                                                 float(weight_offset), T, topk, k, int(num_experts), _a_type(slot_out.dtype),
                                                 _QFORMATS[fmt] if fmt else 0)
    return _combine_norm_result(rc, "moe_combine_rmsnorm_cpu", slot_out.dtype, T, topk, k, num_experts, fmt, qa, res_out, y16)


# --- tensors already packed by the REFERENCE wheel -> this build's layout (include/petit_amd.h, petit_convert_reference_*) -----

def from_reference_packed_weights(b_packed: torch.Tensor, size_n: int, size_k: int) -> torch.Tensor:
    """int32 [N/16, 2K] as returned by the REFERENCE's repack_nvfp4 / repack_mxfp4 -> the same shape in this build's layout."""
    _check(size_k % _LAYOUT_M == 0 and size_n % 32 == 0, "needs size_k % 128 == 0 and size_n % 32 == 0")
    _check(b_packed.dtype == torch.int32 and b_packed.numel() * 4 == size_n * size_k // 2, "b_packed does not hold size_n * size_k 4-bit weights")
    _cpu(b_packed, "b_packed")
    out = torch.empty((size_n // _LAYOUT_N, size_k * _LAYOUT_N // _PACK), dtype=torch.int32)
    _raise_on(_lib.lib.petit_convert_reference_weights_host(out.data_ptr(), b_packed.contiguous().data_ptr(), size_k, size_n),
              "from_reference_packed_weights")
    return out


def from_reference_packed_nvfp4_scales(s_packed: torch.Tensor, size_n: int, size_k: int) -> torch.Tensor:
    """[N, K/16] bytes as returned by the REFERENCE's process_nvfp4_scales ("e5m3" bytes in its layout) -> float8_e4m3fn
    [N, K/16] in this build's layout."""
    _check(size_k % (2 * _LAYOUT_M) == 0 and size_n % 64 == 0, "needs size_k % 256 == 0 and size_n % 64 == 0")
    _check(s_packed.numel() * s_packed.element_size() == size_n * size_k // 16, "s_packed does not hold size_n * size_k / 16 scale bytes")
    _cpu(s_packed, "s_packed")
    out = torch.empty((size_n, size_k // 16), dtype=torch.uint8)
    _raise_on(_lib.lib.petit_convert_reference_nvfp4_scales_host(out.data_ptr(), s_packed.contiguous().data_ptr(), size_k, size_n),
              "from_reference_packed_nvfp4_scales")
    return out.view(torch.float8_e4m3fn)


def from_reference_packed_mxfp4_scales(s_packed: torch.Tensor, size_n: int, size_k: int) -> torch.Tensor:
    """uint8 [N/32, K] as returned by the REFERENCE's process_mxfp4_scales -> the same shape in this build's layout."""
    _check(size_k % (2 * _LAYOUT_M) == 0 and size_n % 32 == 0, "needs size_k % 256 == 0 and size_n % 32 == 0")
    _check(s_packed.dtype == torch.uint8 and s_packed.numel() == size_n * size_k // 32, "s_packed does not hold size_n * size_k / 32 scale bytes")
    _cpu(s_packed, "s_packed")
    out = torch.empty((size_n // 32, size_k), dtype=torch.uint8)
    _raise_on(_lib.lib.petit_convert_reference_mxfp4_scales_host(out.data_ptr(), s_packed.contiguous().data_ptr(), size_k, size_n),
              "from_reference_packed_mxfp4_scales")
    return out


# --- the MFMA-native image of NVFP4 weights, offline (include/petit_amd.h "NVFP4 weights on the native class") ---------------------------

def nvfp4_native_image_cpu(b_packed: torch.Tensor, s_packed: torch.Tensor, size_n: int, size_k: int) -> torch.Tensor:
    """CPU twin of petit_kernel.nvfp4_native_image: the PACKED tensors (repack_nvfp4_cpu / process_nvfp4_scales_cpu) -> the image, uint8, bit-identical
    to what the device kernel builds; save it with the checkpoint and copy it to the GPU as it is."""
    nbytes = int(_lib.lib.petit_nvfp4_native_image_bytes(size_k, size_n))
    _check(nbytes > 0, f"Incompatible problem shape (n={size_n}, k={size_k})")
    _check(b_packed.numel() * b_packed.element_size() == size_n * size_k // 2, "b_packed does not hold size_n * size_k 4-bit weights")
    _check(s_packed.numel() * s_packed.element_size() == size_n * size_k // 16, "s_packed does not hold size_n * size_k / 16 scales")
    _cpu(b_packed, "b_packed")
    _cpu(s_packed, "s_packed")
    image = torch.empty(nbytes, dtype=torch.uint8)
    _raise_on(_lib.lib.petit_nvfp4_native_image_host(image.data_ptr(), b_packed.data_ptr(), s_packed.data_ptr(), size_k, size_n), "nvfp4_native_image_cpu")
    return image


def nvfp4_native_image_dequant_cpu(image: torch.Tensor, size_n: int, size_k: int) -> torch.Tensor:
    """Dense expansion of an image on the CPU (test / debug aid): f32 [N, K] = element x 2^(scale - 127), WITHOUT the global scale."""
    _check(image.dtype == torch.uint8 and image.numel() == int(_lib.lib.petit_nvfp4_native_image_bytes(size_k, size_n)) and image.numel() > 0,
           "image does not hold the native image of size_n x size_k NVFP4 weights")
    _cpu(image, "image")
    out = torch.empty((size_n, size_k), dtype=torch.float32)
    _raise_on(_lib.lib.petit_nvfp4_native_image_dequant_host(out.data_ptr(), image.data_ptr(), size_k, size_n), "nvfp4_native_image_dequant_cpu")
    return out

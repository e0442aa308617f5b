"""petit_kernel.compiled -- the compiled operator layer: `torch.ops.petit_kernel.*` (csrc/torch_binding.cpp,
lib/libpetit_torch.so), the counterpart of the reference's ATen extension (lib/pybind/fp4.cc, pybind.cc:8-26).

Same functions and argument order as petit_kernel.ops (the ctypes layer); both call the same C ABI of libpetit_amd.so.
The package front end (petit_kernel/__init__.py) uses this layer when the library is present (it costs a third of
the ctypes layer's host time per call, see bench.py `host_us_per_call`) and the ctypes layer otherwise;
$PETIT_AMD_BINDING=ctypes|compiled forces one.
"""
from __future__ import annotations

import os
from pathlib import Path

import torch

from . import _lib  # loads libpetit_amd.so first (the binding links against it)
from .ops import _rotated_weights
from .ops import QuantizedActivations, _a_type, _activation as _act, _activation_operand, _quantized_format
from .ops import _check_invariant, _check_route_hidden, _check_router, _combine_norm_operands, _combine_norm_returns
from .ops import invariant_geometry, invariant_slabs, invariant_workspace_bytes  # (queries: plain C calls, no op behind them)
from .ops import moe_invariant_form, moe_invariant_workspace_bytes
from .ops import _QFORMATS, native_invariant_slabs, native_invariant_workspace_bytes
from .ops import native_moe_invariant_form, native_moe_invariant_workspace_bytes

LIB_PATH = Path(_lib.LIB_PATH).parent / "libpetit_torch.so"
_loaded = False
_error = None


def available() -> bool:
    """True once lib/libpetit_torch.so is loaded into torch's dispatcher."""
    global _loaded, _error
    if _loaded:
        return True
    if _error is not None or os.environ.get("PETIT_AMD_BINDING", "") == "ctypes":
        return False
    if not LIB_PATH.exists():
        _error = f"{LIB_PATH} not built (python petit-kernel_amd/build.py)"
        return False
    try:
        torch.ops.load_library(str(LIB_PATH))
        _loaded = True
    except Exception as exc:  # noqa: BLE001 -- e.g. a torch ABI mismatch: the ctypes layer still works
        _error = repr(exc)
    return _loaded


def why_unavailable() -> str:
    return _error or ""


def _sid(solution_id: int, native: bool = False) -> int:
    """Python id -> the signed 64-bit value the op schema carries (`int` = int64).  Ids are unsigned 64-bit patterns with
    the K split in bits 60-63, so a split of 8..15 does not fit a signed int64 as such: it crosses as its two's-complement
    value and the binding reinterprets it.  Any negative id means "library default" (reference: fp4.cc:189-191).
    native: for the native ops, which read every negative value but -2 / -3 / -4 as the library default: an id of 2^63 or more goes to them
    as it is, and the schema's int64 refuses it."""
    solution_id = int(solution_id)
    if solution_id < 0:
        # -2 / -3 / -4 cross as they are.  The native ops read them as the native-class sentinels (the caller has opted in by calling them); the
        # reference's ops do so ONLY for NVFP4 weights that have an MFMA-native image attached (attach_nvfp4_native: the caller's opt-in), and
        # as the library default everywhere else -- the reference's meaning of any negative id
        return solution_id if solution_id >= -4 else -1
    if native:
        return solution_id
    if solution_id >= 1 << 64:
        raise RuntimeError(f"No kernel implementation for solution_id={solution_id}.")
    return solution_id - (1 << 64) if solution_id >= 1 << 63 else solution_id


def repack_nvfp4(b_q_weight, size_n, size_k):
    return torch.ops.petit_kernel.repack_nvfp4(b_q_weight, size_n, size_k)


def process_nvfp4_scales(scales, size_n, size_k):
    return torch.ops.petit_kernel.process_nvfp4_scales(scales, size_n, size_k)


def process_mxfp4_scales(scales, size_n, size_k):
    return torch.ops.petit_kernel.process_mxfp4_scales(scales, size_n, size_k)


def hadamard_rotate(x, block, log2_scale=0, out=None):
    if out is None:
        return torch.ops.petit_kernel.hadamard_rotate(x, block, log2_scale)
    torch.ops.petit_kernel.hadamard_rotate_out(x, block, log2_scale, out)
    return out


def quantize_nvfp4(w, global_scale=None, hadamard=0):
    return torch.ops.petit_kernel.quantize_weights(_rotated_weights(w, hadamard, hadamard_rotate), _lib.CXX_DTYPE_FP4_E2M1, global_scale)


def quantize_mxfp4(w, hadamard=0):
    return torch.ops.petit_kernel.quantize_weights(_rotated_weights(w, hadamard, hadamard_rotate), _lib.CXX_DTYPE_MXFP4_E2M1, None)


def mul_nvfp4_a16(A, B, s, global_scale, size_m, size_n, size_k, solution_id, bias=None, activation=None):
    return torch.ops.petit_kernel.mul_nvfp4_a16(A, B, s, global_scale, size_m, size_n, size_k, _sid(solution_id), bias, _act(activation))


def mul_mxfp4_a16(A, B, s, global_scale, size_m, size_n, size_k, solution_id, bias=None, activation=None):
    return torch.ops.petit_kernel.mul_mxfp4_a16(A, B, s, global_scale, size_m, size_n, size_k, _sid(solution_id), bias, _act(activation))


def mul_nvfp4_a16_invariant(A, B, s, global_scale, size_m, size_n, size_k, bias=None, activation=None):
    act = _check_invariant(A, B, s, global_scale, size_m, size_n, size_k, bias, activation, "nv")[3]
    return torch.ops.petit_kernel.mul_nvfp4_a16_invariant(A, B, s, global_scale, int(size_m), int(size_n), int(size_k), bias, act)


def mul_mxfp4_a16_invariant(A, B, s, global_scale, size_m, size_n, size_k, bias=None, activation=None):
    act = _check_invariant(A, B, s, global_scale, size_m, size_n, size_k, bias, activation, "mx")[3]
    return torch.ops.petit_kernel.mul_mxfp4_a16_invariant(A, B, s, global_scale, int(size_m), int(size_n), int(size_k), bias, act)


def mul_mxfp4_native_invariant(A, B, s, global_scale, size_m, size_n, size_k, fmt="mxfp8", bias=None, activation=None):
    a, dtype, quantized, act = _check_invariant(A, B, s, global_scale, size_m, size_n, size_k, bias, activation, "mx", fmt)[:4]
    return torch.ops.petit_kernel.mul_mxfp4_native_invariant(a, B, s, global_scale, int(size_m), int(size_n), int(size_k), _QFORMATS[fmt],
                                                             bool(quantized), dtype == torch.bfloat16, bias, act)


def mul_nvfp4_a16_moe(A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, solution_id=-1, bias=None, activation=None):
    return torch.ops.petit_kernel.mul_nvfp4_a16_moe(A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, _sid(solution_id),
                                                    bias, _act(activation))


def mul_mxfp4_a16_moe(A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, solution_id=-1, bias=None, activation=None):
    return torch.ops.petit_kernel.mul_mxfp4_a16_moe(A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, _sid(solution_id),
                                                    bias, _act(activation))


def _mul_moe_indexed(kind, A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index, c_rows,
                     solution_id, bias, activation, out):
    c_rows = -1 if c_rows is None else int(c_rows)
    args = (A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index, c_rows, _sid(solution_id), bias,
            _act(activation))
    if out is None:
        return getattr(torch.ops.petit_kernel, f"mul_{kind}fp4_a16_moe_indexed")(*args)
    getattr(torch.ops.petit_kernel, f"mul_{kind}fp4_a16_moe_indexed_out")(out, *args)
    return out


def mul_nvfp4_a16_moe_indexed(A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index=None, c_row_index=None,
                              c_rows=None, solution_id=-1, bias=None, activation=None, out=None):
    return _mul_moe_indexed("nv", A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index, c_rows,
                            solution_id, bias, activation, out)


def mul_mxfp4_a16_moe_indexed(A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index=None, c_row_index=None,
                              c_rows=None, solution_id=-1, bias=None, activation=None, out=None):
    return _mul_moe_indexed("mx", A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index, c_rows,
                            solution_id, bias, activation, out)


def _mul_moe_invariant(kind, A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index, c_rows, bias,
                       activation, out):
    _, _, _, act, E, _, c_rows = _check_invariant(A, B, s, global_scales, size_m, size_n, size_k, bias, activation, kind,
                                                  experts=(expert_offsets, num_experts, a_row_index, c_row_index, c_rows, out))
    args = (A, B, s, global_scales, expert_offsets, int(size_m), int(size_n), int(size_k), E, a_row_index, c_row_index, int(c_rows), bias, act)
    if out is None:
        return getattr(torch.ops.petit_kernel, f"mul_{kind}fp4_a16_moe_invariant")(*args)
    getattr(torch.ops.petit_kernel, f"mul_{kind}fp4_a16_moe_invariant_out")(out, *args)
    return out


def mul_nvfp4_a16_moe_invariant(A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index=None,
                                c_row_index=None, c_rows=None, bias=None, activation=None, out=None):
    return _mul_moe_invariant("nv", A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index,
                              c_rows, bias, activation, out)


def mul_mxfp4_a16_moe_invariant(A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index=None,
                                c_row_index=None, c_rows=None, bias=None, activation=None, out=None):
    return _mul_moe_invariant("mx", A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index,
                              c_rows, bias, activation, out)


def mul_nvfp4_native_invariant(A, image, global_scale, size_m, size_n, size_k, fmt="mxfp8", bias=None, activation=None):
    a, dtype, quantized, act = _check_invariant(A, image, None, global_scale, size_m, size_n, size_k, bias, activation, "nv", fmt)[:4]
    return torch.ops.petit_kernel.mul_nvfp4_native_invariant(a, image, global_scale, int(size_m), int(size_n), int(size_k), _QFORMATS[fmt],
                                                             bool(quantized), dtype == torch.bfloat16, bias, act)


def mul_nvfp4_native_moe_invariant(A, images, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index=None,
                                   c_row_index=None, c_rows=None, fmt="mxfp8", bias=None, activation=None):
    a, dtype, quantized, act, E, _, c_rows = _check_invariant(A, images, None, global_scales, size_m, size_n, size_k, bias, activation, "nv", fmt,
                                                              (expert_offsets, num_experts, a_row_index, c_row_index, c_rows, None))
    return torch.ops.petit_kernel.mul_nvfp4_native_moe_invariant(a, images, global_scales, expert_offsets, int(size_m), int(size_n), int(size_k), E,
                                                                 a_row_index, c_row_index, int(c_rows), _QFORMATS[fmt], bool(quantized),
                                                                 dtype == torch.bfloat16, bias, act)


def mul_mxfp4_native_moe_invariant(A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index=None,
                                   c_row_index=None, c_rows=None, fmt="mxfp8", bias=None, activation=None):
    a, dtype, quantized, act, E, _, c_rows = _check_invariant(A, B, s, global_scales, size_m, size_n, size_k, bias, activation, "mx", fmt,
                                                              (expert_offsets, num_experts, a_row_index, c_row_index, c_rows, None))
    return torch.ops.petit_kernel.mul_mxfp4_native_moe_invariant(a, B, s, global_scales, expert_offsets, int(size_m), int(size_n), int(size_k), E,
                                                                 a_row_index, c_row_index, int(c_rows), _QFORMATS[fmt], bool(quantized),
                                                                 dtype == torch.bfloat16, bias, act)


def moe_align_device(topk_ids, num_experts):
    return torch.ops.petit_kernel.moe_align_device(topk_ids, num_experts)


def moe_combine(slot_out, topk_weights, topk_ids, num_experts):
    return torch.ops.petit_kernel.moe_combine(slot_out, topk_weights, topk_ids, num_experts)


def moe_combine_rmsnorm(slot_out, topk_weights, topk_ids, num_experts, weight, eps=1e-6, fmt=None, *, residual=None, weight_offset=0.0,
                        return_normed=None, return_hidden=None, inplace_residual=False):
    T, _, k = _combine_norm_operands(slot_out, topk_weights, topk_ids, num_experts, weight, eps, fmt, residual, weight_offset, on_gpu=True)
    want_h, want_y = _combine_norm_returns(fmt, residual, return_normed, return_hidden, inplace_residual)
    qa, h, y = torch.ops.petit_kernel.moe_combine_rmsnorm(slot_out, topk_weights, topk_ids, int(num_experts), weight, float(eps),
                                                          _quantized_format(fmt, "fmt must be None, 'mxfp8', 'mxfp6' or 'mxfp4'"), residual,
                                                          float(weight_offset), want_y, want_h, bool(inplace_residual))
    out = (QuantizedActivations(qa, T, k, fmt, slot_out.dtype),) if fmt else ()
    out += ((residual if inplace_residual else h),) if want_h else ()
    out += (y,) if want_y else ()
    return out[0] if len(out) == 1 else out


_SCORING = {"softmax": 0, "sigmoid": 1}


def _scoring(scoring) -> int:
    if scoring not in _SCORING:
        raise RuntimeError("scoring must be 'softmax' or 'sigmoid'")
    return _SCORING[scoring]


def moe_route(router_logits, topk, scoring="softmax", renormalize=True, bias=None, n_group=1, topk_group=1, routed_scaling_factor=1.0,
              return_keys=False):
    w, ids, keys = torch.ops.petit_kernel.moe_route(router_logits, int(topk), _scoring(scoring), bool(renormalize), bias, int(n_group),
                                                    int(topk_group), float(routed_scaling_factor), bool(return_keys))
    return (w, ids, keys) if return_keys else (w, ids)


def moe_route_align(router_logits, topk, scoring="softmax", renormalize=True, bias=None, n_group=1, topk_group=1, routed_scaling_factor=1.0,
                    return_keys=False):
    w, ids, sp, off, ti, keys = torch.ops.petit_kernel.moe_route_align(router_logits, int(topk), _scoring(scoring), bool(renormalize), bias,
                                                                       int(n_group), int(topk_group), float(routed_scaling_factor),
                                                                       bool(return_keys))
    return (w, ids, sp, off, ti, keys) if return_keys else (w, ids, sp, off, ti)


def _slots_args(expert_map, num_local_experts, num_shared, shared_weight, shared_gate_logits):
    return (expert_map, -1 if num_local_experts is None else int(num_local_experts), int(num_shared), float(shared_weight), shared_gate_logits)


def moe_route_ex(router_logits, topk, scoring="softmax", renormalize=True, bias=None, n_group=1, topk_group=1, routed_scaling_factor=1.0,
                 return_keys=False, expert_map=None, num_local_experts=None, num_shared=0, shared_weight=1.0, shared_gate_logits=None):
    w, ids, keys = torch.ops.petit_kernel.moe_route_ex(router_logits, int(topk), _scoring(scoring), bool(renormalize), bias, int(n_group),
                                                       int(topk_group), float(routed_scaling_factor), bool(return_keys),
                                                       *_slots_args(expert_map, num_local_experts, num_shared, shared_weight, shared_gate_logits))
    return (w, ids, keys) if return_keys else (w, ids)


def moe_route_align_ex(router_logits, topk, scoring="softmax", renormalize=True, bias=None, n_group=1, topk_group=1, routed_scaling_factor=1.0,
                       return_keys=False, expert_map=None, num_local_experts=None, num_shared=0, shared_weight=1.0, shared_gate_logits=None):
    w, ids, sp, off, ti, keys = torch.ops.petit_kernel.moe_route_align_ex(
        router_logits, int(topk), _scoring(scoring), bool(renormalize), bias, int(n_group), int(topk_group), float(routed_scaling_factor),
        bool(return_keys), *_slots_args(expert_map, num_local_experts, num_shared, shared_weight, shared_gate_logits))
    return (w, ids, sp, off, ti, keys) if return_keys else (w, ids, sp, off, ti)


def moe_router_logits(hidden, router_weight, router_bias=None):
    _check_router(hidden, router_weight, router_bias)
    return torch.ops.petit_kernel.moe_router_logits(hidden, router_weight, router_bias)


def moe_route_hidden(hidden, router_weight, topk, router_bias=None, align=True, scoring="softmax", renormalize=True, bias=None, n_group=1,
                     topk_group=1, routed_scaling_factor=1.0, return_keys=False, expert_map=None, num_local_experts=None, num_shared=0,
                     shared_weight=1.0, shared_gate_logits=None):
    _check_route_hidden(hidden, router_weight, topk, router_bias, scoring, bias, n_group, topk_group, expert_map, num_local_experts, num_shared,
                        shared_gate_logits)
    w, ids, sp, off, ti, keys = torch.ops.petit_kernel.moe_route_hidden(
        hidden, router_weight, router_bias, int(topk), bool(align), _scoring(scoring), bool(renormalize), bias, int(n_group), int(topk_group),
        float(routed_scaling_factor), bool(return_keys), *_slots_args(expert_map, num_local_experts, num_shared, shared_weight, shared_gate_logits))
    out = (w, ids, sp, off, ti) if align else (w, ids)
    return out + (keys,) if return_keys else out


def _native_operands(A, size_m, size_k, out_quantized):
    """What the native ops take in place of A and out_quantized: (activation tensor, a_format, a_type, out_format, 16-bit dtype)."""
    out_fmt = _quantized_format(out_quantized, "out_quantized must be None, 'mxfp8', 'mxfp6' or 'mxfp4'")
    a_t, dtype, a_fmt = _activation_operand(A, size_m, size_k)
    return a_t, a_fmt, _a_type(dtype), out_fmt, dtype


def _mul_native_moe(kind, A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index, c_rows,
                    solution_id, bias, activation, out_quantized, transient=False, workspace=None):
    a_t, a_fmt, a_type, out_fmt, dtype = _native_operands(A, size_m, size_k, out_quantized)
    op = getattr(torch.ops.petit_kernel, f"mul_{kind}fp4_native_moe" + ("_transient" if transient else ""))
    extra = (workspace,) if transient else ()
    c = op(a_t, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index,
           -1 if c_rows is None else int(c_rows), _sid(solution_id, native=True), bias, _act(activation), a_fmt, a_type, out_fmt, *extra)
    return QuantizedActivations(c, size_m, size_n // 2, out_quantized, dtype) if out_fmt else c


def mul_mxfp4_native_moe(A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index=None, c_row_index=None,
                         c_rows=None, solution_id=-2, bias=None, activation=None, out_quantized=None):
    return _mul_native_moe("mx", A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index, c_rows,
                           solution_id, bias, activation, out_quantized)


def mul_nvfp4_native_moe(A, images, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index=None, c_row_index=None,
                         c_rows=None, solution_id=-2, bias=None, activation=None, out_quantized=None):
    return _mul_native_moe("nv", A, images, None, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index,
                           c_rows, solution_id, bias, activation, out_quantized)


def mul_nvfp4_native_moe_transient(A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index=None,
                                   c_row_index=None, c_rows=None, solution_id=-2, bias=None, activation=None, out_quantized=None,
                                   workspace=None):
    return _mul_native_moe("nv", A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index, c_rows,
                           solution_id, bias, activation, out_quantized, transient=True, workspace=workspace)


def mul_nvfp4_native_transient(A, B, s, global_scale, size_m, size_n, size_k, solution_id=-2, bias=None, activation=None, out_quantized=None):
    a_t, a_fmt, a_type, out_fmt, dtype = _native_operands(A, size_m, size_k, out_quantized)
    c = torch.ops.petit_kernel.mul_nvfp4_native_transient(a_t, B, s, global_scale, size_m, size_n, size_k, _sid(solution_id, native=True),
                                                          bias, _act(activation), a_fmt, a_type, out_fmt)
    return QuantizedActivations(c, size_m, size_n // 2, out_quantized, dtype) if out_fmt else c

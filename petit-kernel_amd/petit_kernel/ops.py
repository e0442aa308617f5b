"""petit_kernel.ops -- the torch-facing operator layer.

Mirrors the reference's pybind extension `petit_kernel.ops`
(lib/pybind/pybind.cc:8-26, lib/pybind/fp4.cc): same function names, argument
order and meaning, same output shapes / dtypes, same error classes
(RuntimeError with the reference's message texts).  torch is used only for
device memory and the current stream; the compute is libpetit_amd.so.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from ._lib import SolutionHints as _CHints

_LAYOUT_N = 16        # kLayoutN, fp4.cc:18
_LAYOUT_M = 128       # kLayoutM, fp4.cc:17
_PACK = 8             # kPackFactor, fp4.cc:19


def _check(cond: bool, msg: str) -> None:
    if not cond:
        raise RuntimeError(msg)  # what TORCH_CHECK / AT_ERROR surface as in Python


def _stream(t: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ptr(t: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(t.data_ptr())


def _opt_ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _raise_on(code: int, what: str) -> None:
    if code != _lib.PETIT_OK:
        raise RuntimeError(f"{what}: {_lib.error_string(code)}")


def _raise_gemm(err: int, name: str, solution_id, shape_text: str) -> None:
    """A GEMM entry point's return code as the caller sees it: the two refusals in the reference's words, anything else in the library's."""
    if err == _lib.PETIT_ERROR_PROBLEM_SHAPE:
        raise RuntimeError(f"Incompatible problem shape ({shape_text})")
    if err == _lib.PETIT_ERROR_KERNEL_SHAPE:
        raise RuntimeError(f"No kernel implementation for solution_id={solution_id}.")
    _raise_on(err, name)


def _a_type(dtype: torch.dtype) -> int:
    return _lib.CXX_DTYPE_BF16 if dtype == torch.bfloat16 else _lib.CXX_DTYPE_FP16


def _scratch(nbytes: int, dev):
    """Per-call scratch from torch's stream-ordered caching allocator (safe with several streams and under graph capture), or None."""
    return torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None


class PetitSolutionHints:
    """PetitSolutionHints (quantization/gemm.h:112-117; bound at pybind.cc:19-25).

    The reference binds the struct but never registers its enum type, so its
    fields cannot actually be used from Python.
    Here they accept a petit_kernel.DataType, a torch dtype or a raw C++ enum
    integer.
    """

    def __init__(self) -> None:
        self.a_type = None
        self.b_type = None
        self.c_type = None
        self.require_high_precision = False

    def __repr__(self) -> str:
        return (f"PetitSolutionHints(a_type={self.a_type}, b_type={self.b_type}, "
                f"c_type={self.c_type}, require_high_precision={self.require_high_precision})")


def _cxx_dtype(x, default=None) -> int:
    """Anything that names an element type -> the reference's C++ DataType value."""
    if x is None:
        if default is None:
            raise RuntimeError("PetitSolutionHints field is not set")
        return default
    if isinstance(x, torch.dtype):
        if x == torch.bfloat16:
            return _lib.CXX_DTYPE_BF16
        if x == torch.float16:
            return _lib.CXX_DTYPE_FP16
        raise RuntimeError("A must be bfloat16 or float16.")
    name = getattr(x, "name", None)
    if name is not None:  # petit_kernel.DataType (Python numbering, __init__.py:8-15)
        table = {"float16": _lib.CXX_DTYPE_FP16, "bfloat16": _lib.CXX_DTYPE_BF16,
                 "float4_e2m1": _lib.CXX_DTYPE_FP4_E2M1, "mxfloat4_e2m1": _lib.CXX_DTYPE_MXFP4_E2M1,
                 "int4": 0, "float8_e4m3fn": 1, "float8_e5m2fn": 6}
        return table[name]
    return int(x)


def _c_hints(h: PetitSolutionHints) -> _CHints:
    a = _cxx_dtype(h.a_type)
    return _CHints(a, _cxx_dtype(h.b_type, _lib.CXX_DTYPE_FP4_E2M1), _cxx_dtype(h.c_type, a),
                   int(bool(h.require_high_precision)))


def repack_nvfp4(b_q_weight: torch.Tensor, size_n: int, size_k: int) -> torch.Tensor:
    """fp4.cc:38-78 (RepackNvFp4).  int32 [N, K/8] -> int32 [N/16, 2K]."""
    _check(size_k % _LAYOUT_M == 0, f"size_k = {size_k} is not divisible by tile_k_size = {_LAYOUT_M}")
    _check(size_n % _LAYOUT_N == 0, f"size_n = {size_n} is not divisible by tile_n_size = {_LAYOUT_N}")
    _check(b_q_weight.dim() == 2 and size_k // _PACK == b_q_weight.size(1),
           f"Shape mismatch: b_q_weight.size(1) = {b_q_weight.size(-1)}, size_k = {size_k}, pack_factor = {_PACK}")
    _check(b_q_weight.size(0) == size_n, f"b_q_weight.size(0) = {b_q_weight.size(0)} is not size_n = {size_n}")
    _check(b_q_weight.is_cuda, "b_q_weight is not on GPU")
    _check(b_q_weight.is_contiguous(), "b_q_weight is not contiguous")
    _check(b_q_weight.dtype == torch.int32, "b_q_weight type is not kInt")
    out = torch.empty((size_n // _LAYOUT_N, size_k * _LAYOUT_N // _PACK), dtype=torch.int32,
                      device=b_q_weight.device)
    with torch.cuda.device(b_q_weight.device):
        rc = _lib.lib.petit_repack_nvfp4_weights(_ptr(out), _ptr(b_q_weight), size_k, size_n, _stream(out))
    _raise_on(rc, "repack_nvfp4")
    return out


def process_nvfp4_scales(scales: torch.Tensor, size_n: int, size_k: int) -> torch.Tensor:
    """fp4.cc:80-121 (ProcessNvFp4Scales).  e4m3 [N, K/16] -> e4m3 [N, K/16]."""
    group_m = 2 * _LAYOUT_M
    _check(size_k % group_m == 0, f"size_k = {size_k} is not divisible by tile_k_size = {group_m}")
    _check(size_n % _LAYOUT_N == 0, f"size_n = {size_n} is not divisible by tile_n_size = {_LAYOUT_N}")
    _check(scales.dim() == 2 and scales.size(1) > 0 and size_k // scales.size(1) == 16 and
           size_k % scales.size(1) == 0, "Only groupsize = 16 is supported.")
    _check(scales.size(0) == size_n, f"scales.size(0) = {scales.size(0)} is not size_n = {size_n}")
    _check(scales.is_cuda, "scales is not on GPU")
    _check(scales.is_contiguous(), "scales is not contiguous")
    _check(scales.dtype == torch.float8_e4m3fn, "scales type is not float8_e4m3fn")
    out = torch.empty((scales.size(0), scales.size(1)), dtype=scales.dtype, device=scales.device)
    with torch.cuda.device(scales.device):
        rc = _lib.lib.petit_repack_nvfp4_scales(_ptr(out), _ptr(scales), size_k, size_n, _stream(out))
    _raise_on(rc, "process_nvfp4_scales")
    return out


def process_mxfp4_scales(scales: torch.Tensor, size_n: int, size_k: int) -> torch.Tensor:
    """fp4.cc:123-161 (ProcessMxFp4Scales).  uint8 [N, K/32] -> uint8 [N/32, K]."""
    group_m = 2 * _LAYOUT_M
    _check(size_k % group_m == 0, f"size_k = {size_k} is not divisible by tile_k_size = {group_m}")
    _check(size_n % _LAYOUT_N == 0, f"size_n = {size_n} is not divisible by tile_n_size = {_LAYOUT_N}")
    _check(scales.dim() == 2 and scales.size(1) > 0 and size_k // scales.size(1) == 32 and
           size_k % scales.size(1) == 0, "Only groupsize = 32 is supported.")
    _check(scales.size(0) == size_n, f"scales.size(0) = {scales.size(0)} is not size_n = {size_n}")
    _check(scales.is_cuda, "scales is not on GPU")
    _check(scales.is_contiguous(), "scales is not contiguous")
    _check(scales.dtype == torch.uint8, "scales type is not uint8")
    # The reference computes size_n / 32 with integer division (fp4.cc:145-147) and
    # would silently drop the last 16 rows; refuse instead.
    _check(size_n % 32 == 0, f"size_n = {size_n} is not divisible by the MX scale tile (32)")
    out = torch.empty((size_n // 32, size_k), dtype=scales.dtype, device=scales.device)
    with torch.cuda.device(scales.device):
        rc = _lib.lib.petit_repack_mxfp4_scales(_ptr(out), _ptr(scales), size_k, size_n, _stream(out))
    _raise_on(rc, "process_mxfp4_scales")
    return out


# --- weight quantiser (include/petit_amd.h "Weight quantiser"; no counterpart in the reference) -----------------------------------------

def _quantize_operands(kind: str, w: torch.Tensor, global_scale, on_gpu: bool = True):
    """The rules quantize_nvfp4 / quantize_mxfp4 and their CPU twins (offline.py) share -> (num_experts, size_n, size_k).  w: 16-bit
    [size_n, size_k] or [num_experts, size_n, size_k]; global_scale (NVFP4 only): None or float32 [num_experts] beside w."""
    _check(w.dtype in (torch.bfloat16, torch.float16), "w must be bfloat16 or float16.")
    _check(w.dim() in (2, 3), "w must be [size_n, size_k] or [num_experts, size_n, size_k]")
    _check(w.is_cuda == on_gpu, "w is not on GPU" if on_gpu else "w must be a CPU tensor (use petit_kernel.quantize_* for GPU tensors)")
    _check(w.is_contiguous(), "w is not contiguous")
    num_experts, (size_n, size_k) = (w.size(0) if w.dim() == 3 else 1), w.shape[-2:]
    _check(size_k % (2 * _LAYOUT_M) == 0, f"size_k = {size_k} is not divisible by tile_k_size = {2 * _LAYOUT_M}")
    _check(size_n % _LAYOUT_N == 0, f"size_n = {size_n} is not divisible by tile_n_size = {_LAYOUT_N}")
    _check(kind != "mx" or num_experts * size_n % 32 == 0,
           f"num_experts * size_n = {num_experts * size_n} is not divisible by the MX scale tile (32)")
    if global_scale is not None:
        _check(global_scale.device == w.device and global_scale.dtype == torch.float32 and global_scale.is_contiguous() and
               global_scale.dim() == 1 and global_scale.numel() == num_experts,
               "global_scale must be a contiguous float32 [num_experts] tensor on w's device")
    return num_experts, size_n, size_k


def _quantize_outputs(kind: str, num_experts: int, size_n: int, size_k: int, dev):
    """(b, s, global_scale) as repack_* / process_*_scales shape them for the stacked [num_experts * size_n, size_k] tensor."""
    rows = num_experts * size_n
    b = torch.empty((rows // _LAYOUT_N, size_k * _LAYOUT_N // _PACK), dtype=torch.int32, device=dev)
    if kind == "mx":
        s = torch.empty((rows // 32, size_k), dtype=torch.uint8, device=dev)
    else:
        s = torch.empty((rows, size_k // 16), dtype=torch.float8_e4m3fn, device=dev)
    return b, s, torch.empty(num_experts, dtype=torch.float32, device=dev)


def _raise_quantize(rc: int, name: str, num_experts: int, size_n: int, size_k: int) -> None:
    if rc == _lib.PETIT_ERROR_PROBLEM_SHAPE:
        raise RuntimeError(f"Incompatible problem shape (num_experts={num_experts}, n={size_n}, k={size_k})")
    _raise_on(rc, name)


def _quantize_weights(kind: str, w: torch.Tensor, global_scale=None):
    E, n, k = _quantize_operands(kind, w, global_scale)
    b, s, gs = _quantize_outputs(kind, E, n, k, w.device)
    ws_bytes = int(_lib.lib.petit_quantize_weights_workspace_bytes(_B_TYPES[kind], E, int(global_scale is not None)))
    ws = _scratch(ws_bytes, w.device)
    with torch.cuda.device(w.device):
        rc = _lib.lib.petit_quantize_weights(_ptr(w), _a_type(w.dtype), _B_TYPES[kind], E, n, k, _opt_ptr(global_scale), _ptr(b), _ptr(s), _ptr(gs),
                                             _opt_ptr(ws), C.c_uint64(ws_bytes), _stream(w))
    _raise_quantize(rc, "quantize_%sfp4" % kind, E, n, k)
    return b, s, gs


# --- block-Hadamard rotation (include/petit_amd.h "Block-Hadamard rotation"; no counterpart in the reference) ---------------------------

_HADAMARD_RULE = "hadamard must be 0 (no rotation), 32 or 128"


def _hadamard_block(hadamard, allow_zero: bool = True) -> int:
    """The rotation block of a `hadamard=` / `block` argument: 0 (where allowed), 32 or 128."""
    _check(isinstance(hadamard, int) and not isinstance(hadamard, bool) and hadamard in ((0, 32, 128) if allow_zero else (32, 128)),
           _HADAMARD_RULE if allow_zero else "block must be 32 or 128")
    return int(hadamard)


def _hadamard_operands(x: torch.Tensor, block, log2_scale, out, on_gpu: bool):
    """The argument checks of hadamard_rotate and of its CPU twin, stated once -> (rows, k, out)."""
    where = "GPU" if on_gpu else "CPU"
    _hadamard_block(block, allow_zero=False)
    _check(isinstance(log2_scale, int) and abs(log2_scale) <= 126, "log2_scale must be an integer in -126 .. 126")
    _check(x.is_cuda == on_gpu and x.is_contiguous() and x.dim() >= 1 and x.dtype in (torch.bfloat16, torch.float16),
           f"x must be a contiguous bfloat16 / float16 {where} tensor")
    k = x.shape[-1]
    _check(k % 256 == 0, f"Incompatible problem shape (k={k}): the rotated dimension must be a multiple of 256")
    if out is None:
        out = torch.empty_like(x)
    else:
        _check(out.device == x.device and out.dtype == x.dtype and out.shape == x.shape and out.is_contiguous(),
               "out must be a contiguous tensor of x's shape and dtype on x's device")
    return (x.numel() // k if k else 0), k, out


def hadamard_rotate(x: torch.Tensor, block: int, log2_scale: int = 0, out: torch.Tensor = None) -> torch.Tensor:
    """Every row of x [..., k] times the unnormalised Sylvester Hadamard block H_block (32 or 128) along k, times 2^log2_scale, rounded once
    to x's 16-bit type ("petit-had/1", petit_hadamard_rows).  Weights for rotated activations: hadamard_rotate(w, B, -log2(B)).  out may be x."""
    rows, k, out = _hadamard_operands(x, block, log2_scale, out, on_gpu=True)
    with torch.cuda.device(x.device):
        rc = _lib.lib.petit_hadamard_rows(_ptr(out), _ptr(x), rows, k, _a_type(x.dtype), int(block), int(log2_scale), _stream(x))
    _raise_on(rc, "hadamard_rotate")
    return out


def _rotated_weights(w: torch.Tensor, hadamard, rotate):
    """w for quantize_*(w, hadamard=B): w itself, or rotate(w, B, -log2 B) on its [E * N, K] view (checked by the quantiser afterwards)."""
    block = _hadamard_block(hadamard)
    if block == 0:
        return w
    _check(w.dtype in (torch.bfloat16, torch.float16), "w must be bfloat16 or float16.")
    _check(w.is_contiguous(), "w is not contiguous")
    return rotate(w, block, -(block.bit_length() - 1))


def quantize_nvfp4(w: torch.Tensor, global_scale: torch.Tensor = None, hadamard: int = 0):
    """16-bit weights [N, K] or [E, N, K] -> (b, s, global_scale): the packed NVFP4 tensors repack_nvfp4 / process_nvfp4_scales return for the
    stacked [E * N, K] tensor and float32 [E] global scales, straight into mul_nvfp4_a16 / mul_nvfp4_a16_moe* / fp4_moe* / nvfp4_native_image(s).
    global_scale: None (amax / 2688 per expert) or the caller's float32 [E].  hadamard = 32 / 128: exactly
    quantize_nvfp4(hadamard_rotate(w, B, -log2 B)), the weights for activations quantised with the same hadamard."""
    return _quantize_weights("nv", _rotated_weights(w, hadamard, hadamard_rotate), global_scale)


def quantize_mxfp4(w: torch.Tensor, hadamard: int = 0):
    """The same for MXFP4 (OCP MX: one e8m0 scale per 32 k, global_scale = 1): (b, s, global_scale) as repack_mxfp4 / process_mxfp4_scales shape them."""
    return _quantize_weights("mx", _rotated_weights(w, hadamard, hadamard_rotate))


_ACTIVATIONS = {None: 0, "none": 0, "silu_mul": 1, "swiglu_oai": 2}   # PETIT_ACTIVATION_* (include/petit_amd.h)
_B_TYPES = {"nv": _lib.CXX_DTYPE_FP4_E2M1, "nvfp4": _lib.CXX_DTYPE_FP4_E2M1, "mx": _lib.CXX_DTYPE_MXFP4_E2M1, "mxfp4": _lib.CXX_DTYPE_MXFP4_E2M1}
_ACTIVATION_RULE = f"activation must be one of {sorted(k for k in _ACTIVATIONS if k)} or None"


def _activation(activation, size_n=None) -> int:
    """The epilogue's activation code; with size_n, also the gated forms' shape rule."""
    _check(activation in _ACTIVATIONS, _ACTIVATION_RULE)
    act = _ACTIVATIONS[activation]
    if act and size_n is not None:
        _check(size_n % 32 == 0, f"{activation} needs size_n % 32 == 0 (gate / up halves of whole tiles), got {size_n}")
    return act


def _query_epilogue(activation):
    """The epilogue argument of the queries (of the epilogue only the activation matters to a pick): a reference, or None without one."""
    act = _ACTIVATIONS[activation]
    return C.byref(_lib.Epilogue(None, act, 0)) if act else None


def _epilogue(bias, act: int, dev, dtype, numel: int, text: str):
    """The fused epilogue c = round16(act(acc * gs + bias[n])) (include/petit_amd.h, petit_epilogue) as the C call's argument: a reference,
    or None when the call has neither part.  `text`: the rule a bias breaks when it is not `numel` contiguous elements of `dtype` on `dev`."""
    if bias is None:
        return C.byref(_lib.Epilogue(None, act, 0)) if act else None
    _check(bias.is_cuda and bias.device == dev and bias.dtype == dtype and bias.is_contiguous() and bias.numel() == numel, text)
    return C.byref(_lib.Epilogue(bias.data_ptr(), act, 0))


def _hints(kind: str, dtype: torch.dtype) -> _CHints:
    a_type = _a_type(dtype)
    return _CHints(a_type, _B_TYPES[kind], a_type, 0)

# solution_id of the Python surface: any negative value = "library default" as in the reference (fp4.cc:189-191), with two
# values reserved for the default pick INSIDE the opt-in native-FP4 class (MXFP4 weights only; petit_amd.h)
SOLUTION_AUTO = -1
SOLUTION_AUTO_NATIVE_MXFP8 = -2
SOLUTION_AUTO_NATIVE_MXFP4 = -3
SOLUTION_AUTO_NATIVE_MXFP6 = -4


def _c_solution_id(solution_id: int, native_ok: bool = False) -> int:
    """Python id -> the C ABI's uint64.  Any negative id is the library default, as in the reference (fp4.cc:189,240); the native-class
    sentinels (-2 / -3 / -4) mean themselves only where the caller has opted into that class (mul_mxfp4_native, the resolve / workspace queries)."""
    solution_id = int(solution_id)
    if native_ok and solution_id == SOLUTION_AUTO_NATIVE_MXFP8:
        return _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP8
    if native_ok and solution_id == SOLUTION_AUTO_NATIVE_MXFP4:
        return _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP4
    if native_ok and solution_id == SOLUTION_AUTO_NATIVE_MXFP6:
        return _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP6
    return _lib.PETIT_SOLUTION_AUTO if solution_id < 0 else solution_id

_ws_need_cache = {}


def _workspace_need(a_type: int, b_type: int, m: int, n: int, k: int, sid: int, act: int = 0) -> int:
    """petit_gemm_workspace_bytes_ex, memoised per problem (a pure function of its arguments; of the epilogue only the
    activation matters)."""
    key = (a_type, b_type, m, n, k, sid, act, _lib.lib.petit_tune_generation())   # (a tuned row may change what AUTO needs)
    need = _ws_need_cache.get(key)
    if need is None:
        hints = _CHints(a_type, b_type, a_type, 0)
        epi = _lib.Epilogue(None, act, 0)
        need = int(_lib.lib.petit_gemm_workspace_bytes_ex(C.byref(hints), m, n, k, C.c_uint64(sid), C.byref(epi) if act else None))
        if len(_ws_need_cache) > 4096:
            _ws_need_cache.clear()
        _ws_need_cache[key] = need
    return need


def _mul(kind: str, A, B, s, global_scale, size_m, size_n, size_k, solution_id, bias=None, activation=None) -> torch.Tensor:
    if A.dtype != torch.bfloat16 and A.dtype != torch.float16:
        raise RuntimeError("A must be bfloat16 or float16.")
    # Checks the reference leaves out but whose
    # violation would read out of bounds:
    _check(A.is_cuda and B.is_cuda and s.is_cuda and global_scale.is_cuda, "all tensors must be on GPU")
    _check(A.is_contiguous() and A.numel() == size_m * size_k, "A must be a contiguous [size_m, size_k] tensor")
    _check(B.is_contiguous() and B.numel() * B.element_size() == size_n * size_k // 2,
           "B does not hold size_n * size_k packed 4-bit weights")
    _check(global_scale.dtype == torch.float32 and global_scale.numel() >= 1, "global_scale must be float32")
    act = _activation(activation, size_n)
    c = torch.empty((size_m, size_n // 2 if act else size_n), dtype=A.dtype, device=A.device)
    # require_high_precision: the reference turns it on for arch <= gfx90a when
    # solution_id < 0 (fp4.cc:24-34,189-191); gfx950 -> False.
    hints = _hints(kind, A.dtype)
    # (NVFP4 weights with an MFMA-native image attached -- attach_nvfp4_native -- have opted into the native class: -2 / -3 / -4 then name it)
    sid = _c_solution_id(solution_id, native_ok=(kind == "nv" and int(solution_id) in (-2, -3, -4) and B.data_ptr() in _attached_images))
    epi = _epilogue(bias, act, A.device, A.dtype, size_n, "bias must be a contiguous [size_n] tensor of A's dtype on A's device")
    # Scratch for kernels that need it (cross-workgroup K split, native-FP4 path): ALWAYS per call -- the same rule as the
    # compiled binding (a workspace registered with set_workspace() serves raw C-ABI callers only: it binds to one
    # stream, and a call from a second stream -- e.g. the side stream torch.cuda.graph captures on after an eager
    # warm-up -- would otherwise drop silently to a slower no-scratch kernel).
    ws_bytes = _workspace_need(hints.a_type, hints.b_type, size_m, size_n, size_k, sid, act)
    ws = _scratch(ws_bytes, A.device)
    fn = _lib.lib.petit_gemm_fp4_fp16_grid_ws if kind == "nv" else _lib.lib.petit_gemm_mxfp4_fp16_grid_ws
    with torch.cuda.device(A.device):
        err = fn(_ptr(c), _ptr(A), _ptr(B), _ptr(s), _ptr(global_scale), size_m, size_n, size_k, C.byref(hints), C.c_uint64(sid), epi,
                 _opt_ptr(ws), C.c_uint64(ws_bytes), _stream(A))
    if err:
        _raise_gemm(err, "mul_%sfp4_a16" % kind, solution_id, f"m={size_m}, n={size_n}, k={size_k}")
    return c


def mul_nvfp4_a16(A, B, s, global_scale, size_m, size_n, size_k, solution_id, bias=None, activation=None) -> torch.Tensor:
    """fp4.cc:163-209 (MulNvFp4A16); `bias` / `activation` (optional, not in the reference) are fused into the epilogue."""
    if s.dim() != 2 or s.size(1) == 0 or size_k // s.size(1) != 16:
        raise RuntimeError(f"Only groupsize = 16 is supported. size_k = {size_k}, s.size(1) = {s.size(-1)}")
    _check(s.numel() == size_n * size_k // 16, "s does not hold size_n * size_k / 16 scales")
    return _mul("nv", A, B, s, global_scale, size_m, size_n, size_k, solution_id, bias, activation)


def mul_mxfp4_a16(A, B, s, global_scale, size_m, size_n, size_k, solution_id, bias=None, activation=None, f16_range=None) -> torch.Tensor:
    """fp4.cc:211-260 (MulMxFp4A16); `bias` / `activation` (optional, not in the reference) are fused into the epilogue.
    `f16_range` (round 3: "every e8m0 block scale lies in 114..140") is accepted and ignored, with a DeprecationWarning: the fp16 x MXFP4 kernels test
    the scale range themselves."""
    if f16_range is not None:
        import warnings
        warnings.warn("mul_mxfp4_a16(f16_range=...) is ignored: the fp16 x MXFP4 kernels test the scale range themselves", DeprecationWarning, stacklevel=2)
    _check(B.size(0) == size_n // _LAYOUT_N, f"B.size(0) = {B.size(0)} is not size_n / 16 = {size_n // _LAYOUT_N}")
    _check(B.size(1) == size_k * _LAYOUT_N // _PACK,
           f"B.size(1) = {B.size(1)} is not packed size = {size_k * _LAYOUT_N // _PACK}")
    _check(s.size(0) == size_n // 32, f"s.size(0) = {s.size(0)} is not size_n / 32 = {size_n // 32}")
    _check(s.size(1) == size_k, f"s.size(1) = {s.size(1)} is not size_k = {size_k}")
    return _mul("mx", A, B, s, global_scale, size_m, size_n, size_k, solution_id, bias, activation)


# --- the batch-invariant GEMM family (include/petit_amd.h "Batch-invariant GEMM", "Batch-invariant MoE launch" and their two "... on the native
# class" sections, and "... on NVFP4 images"; no counterpart in the reference): one check and one driver for all the entries ---------------

def _invariant_name(kind: str, native: bool, moe: bool) -> str:
    if native:
        return ("mul_%sfp4_native_moe_invariant" if moe else "mul_%sfp4_native_invariant") % kind
    return ("mul_%sfp4_a16_moe_invariant" if moe else "mul_%sfp4_a16_invariant") % kind


_INVARIANT_BIAS_TEXT = {False: "bias must be a contiguous [size_n] tensor of A's dtype on A's device",
                        True: "bias must be a contiguous [num_experts, size_n] tensor of A's dtype on A's device"}  # by `moe`


def _check_invariant(A, B, s, global_scale, size_m, size_n, size_k, bias, activation, kind="mx", fmt=None, experts=None):
    """The argument checks of the batch-invariant entries, stated here for both operator layers.  kind: the weight format, 'nv' / 'mx';
    fmt: the native class's activation format (None: the exact class), where kind 'nv' means B is the native image (nvfp4_native_image; a MoE
    call: num_experts images back to back) and s is None; experts: (expert_offsets, num_experts, a_row_index, c_row_index,
    c_rows, out) of a MoE call, whose global_scale is the [num_experts] tensor (None: a dense call).
    -> (activation tensor, 16-bit dtype, a_is_quantized, activation code, E, a_rows, c_rows), the last three None for a dense call.
    Value checks come first and device checks last, so that the texts can be read without a GPU.  The order within an entry decides which
    text an ill-formed call gets, and is each entry's own."""
    native, moe = fmt is not None, experts is not None
    name = _invariant_name(kind, native, moe)
    if native:
        _check(fmt in _QFORMATS, "fmt must be 'mxfp8', 'mxfp6' or 'mxfp4'")
    quantized = native and isinstance(A, QuantizedActivations)
    dtype = A.dtype
    _check(dtype in (torch.bfloat16, torch.float16),
           "A must be bfloat16 or float16 (or QuantizedActivations of such a tensor)." if native else "A must be bfloat16 or float16.")
    size_m, size_n, size_k = int(size_m), int(size_n), int(size_k)
    E = a_rows = c_rows = None
    if moe:
        expert_offsets, num_experts, a_row_index, c_row_index, c_rows, out = experts
        E = int(num_experts)
        if not 1 <= E <= _lib.PETIT_MOE_MAX_EXPERTS:  # (this is the per-call path of a decode step: the longer texts are built when raised)
            _check(False, f"num_experts must be in 1..{_lib.PETIT_MOE_MAX_EXPERTS}, got {E}")
    # (the exact dense entry accepts n % 16 for both kinds: MXFP4's n % 32 is its C return code's)
    n_mult = 32 if native or (moe and kind == "mx") else 16
    if not (size_n > 0 and size_n % n_mult == 0 and size_k > 0 and size_k % 256 == 0 and 0 <= size_m < 1 << 20):
        _check(False, f"Incompatible problem shape (m={size_m}, n={size_n}, k={size_k}): {name} needs n % {n_mult} == 0, k % 256 == 0, m < 2^20")
    if native:
        _check(activation in _ACTIVATIONS, _ACTIVATION_RULE)
        act = _ACTIVATIONS[activation]
        _check(not act or size_n % 64 == 0, f"{activation} needs size_n % 64 == 0 here (gate / up halves of whole tile pairs), got {size_n}")
    else:
        _check(not (kind == "mx" and dtype == torch.float16),
               f"{name}: float16 activations with MXFP4 weights have no batch-invariant kernel (use bfloat16)")
        act = _activation(activation, size_n)
    # the activation operand: quantised bytes of the [size_m, size_k] rows, a 16-bit [a_rows, size_k] matrix (MoE), or [size_m, size_k]
    if quantized:
        _check(A.fmt == fmt, f"quantised activations are {A.fmt}, the call says fmt={fmt!r}")
        _check(A.m == size_m and A.k == size_k, f"quantised activations are [{A.m}, {A.k}], the call says [{size_m}, {size_k}]")
        if moe:
            _check(a_row_index is None, f"{name}: quantised activations are the grouped rows already; a_row_index must be None")
        a, a_rows = A.data, size_m
        _check(a.dtype == torch.uint8 and a.is_contiguous() and a.numel() == int(_lib.lib.petit_quantized_activation_bytes(size_m, size_k, _QFORMATS[fmt])),
               "quantised activations do not hold the bytes of their [m, k] and format")
    elif moe:
        a = A
        _check(a.is_contiguous() and a.numel() % size_k == 0, "A must be a contiguous [a_rows, size_k] tensor")
        a_rows = a.numel() // size_k
        if not native:
            _check(a_rows * size_k * 2 <= 1 << 31, f"{name}: A holds more than 2^31 bytes (a_rows={a_rows}, k={size_k})")
    else:
        a = A
        if native:
            _check(size_m <= 65535, f"{name}: a 16-bit A of more than 65535 rows must be quantised first (quantize_activations in pieces)")
        _check(a.is_contiguous() and a.numel() == size_m * size_k, "A must be a contiguous [size_m, size_k] tensor")
    # weights and scales, of num_experts matrices back to back in a MoE call
    count, what = (E, "num_experts * ") if moe else (1, "")
    group = 16 if kind == "nv" else 32
    if native and kind == "nv":
        image_bytes = int(_lib.lib.petit_nvfp4_native_image_bytes(size_k, size_n))
        _check(B.is_contiguous() and B.dtype == torch.uint8 and B.numel() == count * image_bytes and image_bytes > 0,
               "images do not hold num_experts native images of size_n x size_k NVFP4 weights" if moe else
               "image does not hold the native image of size_n x size_k NVFP4 weights")
    else:
        _check(B.is_contiguous() and B.numel() * B.element_size() == count * size_n * size_k // 2,
               f"B does not hold {what}size_n * size_k packed 4-bit weights")
        _check(s.is_contiguous() and s.numel() * s.element_size() == count * size_n * size_k // group,
               f"s does not hold {what}size_n * size_k / {group} scales")
    if moe:
        _check(global_scale.dtype == torch.float32 and global_scale.is_contiguous() and global_scale.numel() == E,
               "global_scales must be a contiguous float32 [num_experts] tensor")
        _check(expert_offsets.dtype == torch.int32 and expert_offsets.is_contiguous() and expert_offsets.numel() == E + 1,
               "expert_offsets must be a contiguous int32 [num_experts + 1] tensor")
        for idx in (a_row_index, c_row_index):
            if idx is not None:
                _check(idx.dtype == torch.int32 and idx.is_contiguous() and idx.numel() == size_m and idx.device == a.device,
                       "row indices must be contiguous int32 [size_m] tensors on A's device")
        if out is not None:
            _check(out.device == a.device and out.dtype == dtype and out.is_contiguous() and out.dim() == 2 and
                   out.size(1) == (size_n // 2 if act else size_n), "out must be a contiguous [c_rows, n_out] tensor of A's dtype on A's device")
            _check(c_rows is None or c_rows < 0 or c_rows == out.size(0), "c_rows does not match out.size(0)")
            c_rows = out.size(0)
        else:
            c_rows = size_m if c_rows is None or c_rows < 0 else int(c_rows)
        if not ((a_row_index is not None or a_rows >= size_m) and (c_row_index is not None or c_rows >= size_m)):
            _check(False, f"{name}: without a row index the matrix must hold size_m rows (a_rows={a_rows}, c_rows={c_rows}, m={size_m})")
    elif global_scale is not None:
        _check(global_scale.dtype == torch.float32 and global_scale.numel() >= 1, "global_scale must be float32")
    if bias is not None:
        _check(bias.dtype == dtype and bias.is_contiguous() and bias.numel() == count * size_n and bias.device == a.device, _INVARIANT_BIAS_TEXT[moe])
    dev = a.device
    _check(a.is_cuda and B.is_cuda and (s is None or s.is_cuda) and (global_scale is None or global_scale.is_cuda) and (not moe or expert_offsets.is_cuda),
           "all tensors must be on GPU")
    _check(B.device == dev and (s is None or s.device == dev) and (global_scale is None or global_scale.device == dev) and
           (not moe or expert_offsets.device == dev), "all tensors must be on A's device")
    return a, dtype, int(quantized), act, E, a_rows, c_rows


def _mul_invariant(A, B, s, global_scale, size_m, size_n, size_k, bias, activation, kind="mx", fmt=None, experts=None) -> torch.Tensor:
    """One call of any entry (the arguments of _check_invariant): output, hints, epilogue, workspace, the C call, the raise."""
    a, dtype, quantized, act, E, a_rows, c_rows = _check_invariant(A, B, s, global_scale, size_m, size_n, size_k, bias, activation, kind, fmt,
                                                                   experts)
    native, moe, shape = fmt is not None, experts is not None, (int(size_m), int(size_n), int(size_k))
    lib = _lib.lib  # (plain attribute reads: this is the per-call path of a decode step)
    if native:  # (the form constants are shared by the two weight formats: one pair of queries)
        ws_fn = lib.petit_gemm_native_moe_invariant_workspace_bytes if moe else lib.petit_gemm_native_invariant_workspace_bytes
        if kind == "nv":
            fn = lib.petit_gemm_nvfp4_native_moe_invariant if moe else lib.petit_gemm_nvfp4_native_invariant
        else:
            fn = lib.petit_gemm_mxfp4_native_moe_invariant if moe else lib.petit_gemm_mxfp4_native_invariant
    elif moe:
        fn = lib.petit_gemm_fp4_fp16_moe_invariant if kind == "nv" else lib.petit_gemm_mxfp4_fp16_moe_invariant
        ws_fn = lib.petit_gemm_moe_invariant_workspace_bytes
    else:
        fn = lib.petit_gemm_fp4_fp16_invariant if kind == "nv" else lib.petit_gemm_mxfp4_fp16_invariant
        ws_fn = lib.petit_gemm_invariant_workspace_bytes
    out = experts[5] if moe else None
    if out is None:
        out = torch.empty((c_rows if moe else shape[0], shape[1] // 2 if act else shape[1]), dtype=dtype, device=a.device)
    hints = _hints(kind, dtype)
    epi = _epilogue(bias, act, a.device, dtype, (E if moe else 1) * shape[1], _INVARIANT_BIAS_TEXT[moe])
    form = (_QFORMATS[fmt], quantized) if native else ()
    ws = _scratch(int(ws_fn(*((E,) if moe else ()), *shape, hints.a_type, *(form or (hints.b_type,)))), a.device)
    routing = ((_ptr(experts[0]), E), (_opt_ptr(experts[2]), a_rows, _opt_ptr(experts[3]), c_rows)) if moe else ((), ())
    weights = (_ptr(B),) if s is None else (_ptr(B), _ptr(s))
    with torch.cuda.device(a.device):
        err = fn(_ptr(out), _ptr(a), *weights, _opt_ptr(global_scale), *routing[0], *shape, *routing[1], C.byref(hints), *form, epi,
                 _opt_ptr(ws), _stream(a))
    if err:
        where = "m=%d, n=%d, k=%d" % shape + (f", num_experts={E}, a_rows={a_rows}, c_rows={c_rows}" if moe else "")
        _raise_gemm(err, _invariant_name(kind, native, moe), "native-invariant" if native else "invariant", where)
    return out


def invariant_geometry(size_n: int, size_k: int, dtype: torch.dtype = torch.bfloat16, kind: str = "nvfp4"):
    """(S, L) of the batch-invariant GEMM for (n, k): S slices of L along K (petit_gemm_invariant_geometry) -- functions of the shape and the
    types alone, never of m."""
    S, L = C.c_uint(0), C.c_uint(0)
    _lib.lib.petit_gemm_invariant_geometry(int(size_n), int(size_k), _a_type(dtype), _B_TYPES[kind], C.byref(S), C.byref(L))
    return S.value, L.value


def invariant_slabs(size_m: int, size_n: int, size_k: int, dtype: torch.dtype = torch.bfloat16, kind: str = "nvfp4") -> int:
    """The slab count of the form m rows get (petit_gemm_invariant_slabs): S in the split form (small m), 1 in the whole form."""
    return int(_lib.lib.petit_gemm_invariant_slabs(int(size_m), int(size_n), int(size_k), _a_type(dtype), _B_TYPES[kind]))


def invariant_workspace_bytes(size_m: int, size_n: int, size_k: int, dtype: torch.dtype = torch.bfloat16, kind: str = "nvfp4") -> int:
    """Bytes of scratch the batch-invariant call uses (petit_gemm_invariant_workspace_bytes): the split form's slabs; 0 for the whole form
    and for a call that would be refused."""
    return int(_lib.lib.petit_gemm_invariant_workspace_bytes(int(size_m), int(size_n), int(size_k), _a_type(dtype), _B_TYPES[kind]))


def mul_nvfp4_a16_invariant(A, B, s, global_scale, size_m, size_n, size_k, bias=None, activation=None) -> torch.Tensor:
    """mul_nvfp4_a16 by the batch-invariant entry (petit_gemm_fp4_fp16_invariant, include/petit_amd.h "Batch-invariant GEMM"): a row's result
    does not depend on size_m, on the row's position or on the launch form.  Opt-in and slower than the default pick; no solution_id."""
    return _mul_invariant(A, B, s, global_scale, size_m, size_n, size_k, bias, activation, "nv")


def mul_mxfp4_a16_invariant(A, B, s, global_scale, size_m, size_n, size_k, bias=None, activation=None) -> torch.Tensor:
    """mul_mxfp4_a16 by the batch-invariant entry (petit_gemm_mxfp4_fp16_invariant); bfloat16 activations only."""
    return _mul_invariant(A, B, s, global_scale, size_m, size_n, size_k, bias, activation, "mx")


def get_fp4_solutions(*args) -> list:
    """fp4.cc:262-283 (GetNvFp4Solutions), bound twice (pybind.cc:14-17).

    Accepts both call shapes that exist in the reference: the bound C++ order
    `(hints, size_m, size_n, size_k)` and the Python wrapper's
    `(size_m, size_n, size_k, a_type, c_type)` (petit_kernel/__init__.py:63-66),
    which the reference itself cannot serve.
    """
    if len(args) == 4 and isinstance(args[0], PetitSolutionHints):
        hints, m, n, k = args
        ch = _c_hints(hints)
    elif len(args) == 5:
        m, n, k, a_type, c_type = args
        a = _cxx_dtype(a_type)
        ch = _CHints(a, _lib.CXX_DTYPE_FP4_E2M1, _cxx_dtype(c_type, a), 0)
    else:
        raise TypeError("get_fp4_solutions(hints, m, n, k) or get_fp4_solutions(m, n, k, a_type, c_type)")
    count = C.c_uint(0)
    err = _lib.lib.petit_gemm_get_solutions(C.byref(ch), m, n, k, None, C.byref(count))
    if err != 0:
        raise RuntimeError(f"Failed to get solutions: {err}")
    buf = (C.c_uint64 * max(count.value, 1))()
    err = _lib.lib.petit_gemm_get_solutions(C.byref(ch), m, n, k, buf, C.byref(count))
    if err != 0:
        raise RuntimeError(f"Failed to get solutions: {err}")
    return [int(buf[i]) for i in range(count.value)]


get_nvfp4_solutions = get_fp4_solutions


# --- native-FP4 path (no counterpart in the reference; opt-in, see include/petit_amd.h) -------------

def enable_native_fp4(enable: bool = True) -> None:
    """Let get_fp4_solutions enumerate the native block-scaled-MFMA kernels (MXFP4 weights only;
    activations are quantised to MXFP8 on the fly, a different accuracy class)."""
    _lib.lib.petit_enable_native_fp4(int(bool(enable)))


def set_mxfp4_default_activations(fmt=None) -> None:
    """Process-wide opt-in for call sites that cannot name a sentinel: fmt 'mxfp8' / 'mxfp6' / 'mxfp4' makes solution_id = -1 on MXFP4
    weights (mul_mxfp4_a16 of an unchanged serving stack) run the default pick of that native class for size_m >= $PETIT_AMD_NATIVE_MIN_M
    (64); None switches it off.  The same as $PETIT_AMD_MXFP4_ACTIVATIONS; quantised activations are another accuracy class."""
    _check(fmt is None or fmt in _QFORMATS, "fmt must be None, 'mxfp8', 'mxfp6' or 'mxfp4'")
    _raise_on(_lib.lib.petit_set_mxfp4_default_class(_QFORMATS[fmt] if fmt else 0), "set_mxfp4_default_activations")
    _ws_need_cache.clear()      # (what AUTO needs as scratch has just changed)


def mxfp4_default_activations():
    v = int(_lib.lib.petit_get_mxfp4_default_class())
    return {8: "mxfp8", 6: "mxfp6", 4: "mxfp4"}.get(v)


def native_workspace_bytes(size_m: int, size_k: int) -> int:
    return int(_lib.lib.petit_native_workspace_bytes(size_m, size_k))


def workspace_bytes(hints: PetitSolutionHints, size_m: int, size_n: int, size_k: int, solution_id: int = -1) -> int:
    """Scratch bytes the call would use (split-K slabs, native-FP4 activations); mul_*_a16 allocates them itself."""
    sid = _c_solution_id(solution_id, native_ok=True)
    ch = _c_hints(hints)
    return int(_lib.lib.petit_gemm_workspace_bytes(C.byref(ch), size_m, size_n, size_k, C.c_uint64(sid)))


def resolve_solution(hints: PetitSolutionHints, size_m: int, size_n: int, size_k: int, solution_id: int = -1, activation=None,
                     workspace_bytes: int = 1 << 62) -> int:
    """The concrete kernel id a call with these arguments runs (petit_gemm_resolve_solution): solution_id may be -1, -2 / -3 / -4
    (default pick inside the native class) or an explicit id; 0 when the call would be refused."""
    ch = _c_hints(hints)
    return int(_lib.lib.petit_gemm_resolve_solution(C.byref(ch), size_m, size_n, size_k, C.c_uint64(_c_solution_id(solution_id, native_ok=True)),
                                                    _query_epilogue(activation), C.c_uint64(workspace_bytes)))


def auto_row_split(hints: PetitSolutionHints, size_m: int, size_n: int, size_k: int, activation=None, solution_id: int = -1) -> int:
    """Rows of the first of the TWO launches a default-pick call at this (ragged prefill) M runs as, 0 = one launch (petit_gemm_row_split).  solution_id -2 / -4 / -3:
    the rows a native-class call runs in the class -- the short tail goes through the exact default pick."""
    ch = _c_hints(hints)
    return int(_lib.lib.petit_gemm_row_split(C.byref(ch), size_m, size_n, size_k, C.c_uint64(_c_solution_id(solution_id, native_ok=True)),
                                             _query_epilogue(activation)))


def dequant_packed(B: torch.Tensor, s: torch.Tensor, size_n: int, size_k: int, kind: str = "nvfp4", dtype=torch.float32,
                   global_scale: float = 1.0) -> torch.Tensor:
    """Dense [size_n, size_k] expansion of PACKED weights (from repack_nvfp4 / process_*_scales): a debug aid, the
    counterpart of the reference's test-only DequantPetitFp4 kernels (quantization_utils.cu:542-727)."""
    _check(kind in ("nvfp4", "mxfp4"), "kind must be 'nvfp4' or 'mxfp4'")
    _check(B.is_cuda and s.is_cuda and B.is_contiguous() and s.is_contiguous(), "packed tensors must be contiguous GPU tensors")
    _check_packed(B, None, size_n, size_k, None)
    out_type = {torch.float32: _lib.PETIT_DTYPE_FP32, torch.bfloat16: _lib.CXX_DTYPE_BF16, torch.float16: _lib.CXX_DTYPE_FP16}.get(dtype)
    _check(out_type is not None, "dtype must be float32, bfloat16 or float16")
    out = torch.empty((size_n, size_k), dtype=dtype, device=B.device)
    with torch.cuda.device(B.device):
        rc = _lib.lib.petit_dequant_packed_weights(_ptr(out), _ptr(B), _ptr(s), float(global_scale), size_n, size_k, _B_TYPES[kind], out_type,
                                                   _stream(B))
    _raise_on(rc, "dequant_packed")
    return out


_workspace_keepalive = {}


def set_workspace(buf) -> None:
    """Register (or with None, unregister) a device scratch tensor for kernels that need one
    (split-K slabs, quantised activations of the native path).  The tensor is kept alive here.
    Only raw C-ABI callers of the entry points WITHOUT a workspace argument use it (petit_gemm_*_grid, _ex):
    mul_*_a16 of both Python layers always allocates its scratch per call.  A registered workspace serves
    ONE stream (include/petit_amd.h "Scratch memory")."""
    if buf is None:
        with torch.cuda.device(torch.cuda.current_device()):
            _lib.lib.petit_set_workspace(None, 0)
        _workspace_keepalive.pop(torch.cuda.current_device(), None)
        return
    _check(buf.is_cuda and buf.is_contiguous(), "workspace must be a contiguous GPU tensor")
    with torch.cuda.device(buf.device):
        _lib.lib.petit_set_workspace(_ptr(buf), C.c_uint64(buf.numel() * buf.element_size()))
        _workspace_keepalive[buf.device.index] = buf


# --- the native class as a pipeline (include/petit_amd.h "The native class as a PIPELINE"; no counterpart in the reference) ---

_QFORMATS = {"mxfp8": 8, "mxfp6": 6, "mxfp4": 4}


class QuantizedActivations:
    """Activations [m, k] quantised to MXFP8 / MXFP4 in the layout the 32x32x64 native kernels read ("petit-qact/1": opaque
    bytes, k-tile major).  Produced by quantize_activations() or by mul_mxfp4_a16(..., activation="silu_mul",
    out_quantized=...); consumed by mul_mxfp4_a16(a=<this>, ...)."""

    def __init__(self, data: torch.Tensor, m: int, k: int, fmt: str, dtype: torch.dtype, hadamard: int = 0):
        self.data, self.m, self.k, self.fmt, self.dtype = data, m, k, fmt, dtype
        self.hadamard = hadamard   # the rotation block the rows were rotated with (bookkeeping: a GEMM cannot know how its weights were made)

    def __repr__(self) -> str:
        return (f"QuantizedActivations(m={self.m}, k={self.k}, fmt={self.fmt!r}, dtype={self.dtype}, hadamard={self.hadamard}, "
                f"{self.data.numel()} bytes)")


_HADAMARD_FP6 = "hadamard needs fmt 'mxfp8' or 'mxfp4': the MXFP6 quantiser has no rotating form"


def quantize_activations(A: torch.Tensor, fmt: str = "mxfp4", hadamard: int = 0) -> QuantizedActivations:
    """16-bit activations [m, k] -> QuantizedActivations (one launch; share the result among GEMMs with the same input).  hadamard = 32 / 128:
    the rows are rotated by that Hadamard block in f32 inside the launch ("petit-had/1"), for weights made with the same hadamard."""
    _check(fmt in _QFORMATS, "fmt must be 'mxfp8', 'mxfp6' or 'mxfp4'")
    _check(_hadamard_block(hadamard) == 0 or fmt != "mxfp6", _HADAMARD_FP6)
    _check(A.is_cuda and A.is_contiguous() and A.dim() == 2 and A.dtype in (torch.bfloat16, torch.float16),
           "A must be a contiguous 2-D bfloat16 / float16 GPU tensor")
    m, k = A.shape
    nbytes = int(_lib.lib.petit_quantized_activation_bytes(m, k, _QFORMATS[fmt]))
    qa = torch.empty(nbytes, dtype=torch.uint8, device=A.device)
    with torch.cuda.device(A.device):
        if hadamard:
            rc = _lib.lib.petit_quantize_activations_rot(_ptr(qa), _ptr(A), m, k, _a_type(A.dtype), _QFORMATS[fmt], hadamard, _stream(A))
        else:
            rc = _lib.lib.petit_quantize_activations(_ptr(qa), _ptr(A), m, k, _a_type(A.dtype), _QFORMATS[fmt], _stream(A))
    if rc == _lib.PETIT_ERROR_PROBLEM_SHAPE:
        raise RuntimeError(f"Incompatible problem shape (m={m}, k={k})")
    _raise_on(rc, "quantize_activations")
    return QuantizedActivations(qa, m, k, fmt, A.dtype, hadamard)


def _rmsnorm_operands(x, weight, eps, fmt, residual, weight_offset, on_gpu: bool, hadamard: int = 0):
    """The argument checks of rmsnorm_quantize and of its CPU twin, stated once -> (m, k)."""
    where = "GPU" if on_gpu else "CPU"
    _check(fmt in _QFORMATS, "fmt must be 'mxfp8', 'mxfp6' or 'mxfp4'")
    _check(_hadamard_block(hadamard) == 0 or fmt != "mxfp6", _HADAMARD_FP6)
    _check(x.is_cuda == on_gpu and x.is_contiguous() and x.dim() == 2 and x.dtype in (torch.bfloat16, torch.float16),
           f"x must be a contiguous 2-D bfloat16 / float16 {where} tensor")
    m, k = x.shape
    _check(weight.device == x.device and weight.is_contiguous() and weight.dtype == x.dtype and tuple(weight.shape) == (k,),
           f"weight must be a contiguous [k] tensor of x's dtype on x's device (k={k})")
    _check(residual is None or (residual.device == x.device and residual.is_contiguous() and residual.dtype == x.dtype and
                                residual.shape == x.shape), "residual must be a contiguous tensor of x's shape and dtype on x's device")
    _check(math.isfinite(eps) and eps > 0, "eps must be finite and positive")
    _check(math.isfinite(weight_offset), "weight_offset must be finite")
    return m, k


def _rmsnorm_outputs(x, fmt, residual, return_normed, inplace_residual):
    m, k = x.shape
    _check(not inplace_residual or residual is not None, "inplace_residual needs a residual")
    qa = torch.empty(int(_lib.lib.petit_quantized_activation_bytes(m, k, _QFORMATS[fmt])), dtype=torch.uint8, device=x.device)
    res_out = None if residual is None else residual if inplace_residual else torch.empty_like(residual)
    y16 = torch.empty_like(x) if return_normed else None
    return qa, res_out, y16


def _rmsnorm_result(rc, name, x, fmt, qa, res_out, y16, hadamard: int = 0):
    m, k = x.shape
    if rc == _lib.PETIT_ERROR_PROBLEM_SHAPE:
        raise RuntimeError(f"Incompatible problem shape (m={m}, k={k})")
    if rc == _lib.PETIT_ERROR_KERNEL_SHAPE:
        raise RuntimeError(f"No kernel implementation for k={k} (the fused norm holds a row of at most 16384 elements).")
    _raise_on(rc, name)
    q = QuantizedActivations(qa, m, k, fmt, x.dtype, hadamard)
    if res_out is None and y16 is None:
        return q
    return (q,) + ((res_out,) if res_out is not None else ()) + ((y16,) if y16 is not None else ())


def rmsnorm_quantize(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6, fmt: str = "mxfp8", *, residual: torch.Tensor = None,
                     weight_offset: float = 0.0, return_normed: bool = False, inplace_residual: bool = False, hadamard: int = 0):
    """(Residual add +) RMSNorm + quantize_activations in ONE launch (include/petit_amd.h "RMSNorm into quantised activations"):
    h = x (+ residual), y = RMSNorm(h) * (weight + weight_offset), result = quantize_activations(y, fmt, hadamard) bit for bit.  Returns the
    QuantizedActivations alone, or a tuple (q, residual_out[, y16]): the updated residual h when `residual` is given (a new tensor, or `residual`
    itself written in place with inplace_residual=True), then the 16-bit y with return_normed=True (never rotated)."""
    m, k = _rmsnorm_operands(x, weight, eps, fmt, residual, weight_offset, on_gpu=True, hadamard=hadamard)
    qa, res_out, y16 = _rmsnorm_outputs(x, fmt, residual, return_normed, inplace_residual)
    args = (_ptr(qa), _opt_ptr(y16), _opt_ptr(res_out), _ptr(x), _opt_ptr(residual), _ptr(weight), float(eps), float(weight_offset), m, k,
            _a_type(x.dtype), _QFORMATS[fmt])
    with torch.cuda.device(x.device):
        if hadamard:
            rc = _lib.lib.petit_rmsnorm_quantize_rot(*args, hadamard, _stream(x))
        else:
            rc = _lib.lib.petit_rmsnorm_quantize(*args, _stream(x))
    return _rmsnorm_result(rc, "rmsnorm_quantize", x, fmt, qa, res_out, y16, hadamard)


def _quantized_format(fmt, text: str) -> int:
    """'mxfp8' / 'mxfp6' / 'mxfp4' -> the format code of the C ABI, None -> 0; `text` for anything else."""
    _check(fmt is None or fmt in _QFORMATS, text)
    return _QFORMATS[fmt] if fmt else 0


def _activation_operand(A, size_m: int, size_k: int):
    """The activation argument of the native class, a 16-bit tensor or QuantizedActivations -> (tensor, 16-bit dtype, a_format).
    Quantised activations must be the call's [size_m, size_k]; what a 16-bit tensor must be is the caller's rule."""
    if isinstance(A, QuantizedActivations):
        _check(A.m == size_m and A.k == size_k, f"quantised activations are [{A.m}, {A.k}], the call says [{size_m}, {size_k}]")
        return A.data, A.dtype, _QFORMATS[A.fmt]
    return A, A.dtype, 0


# --- the batch-invariant GEMM on the native class (include/petit_amd.h "Batch-invariant GEMM on the native class") -------------------------

def native_invariant_slabs(size_m: int, size_n: int, size_k: int, dtype: torch.dtype = torch.bfloat16) -> int:
    """The slab count of the form m rows get (petit_gemm_native_invariant_slabs): S in the split form (m <= 64), 1 in the whole form."""
    return int(_lib.lib.petit_gemm_native_invariant_slabs(int(size_m), int(size_n), int(size_k), _a_type(dtype)))


def native_invariant_workspace_bytes(size_m: int, size_n: int, size_k: int, dtype: torch.dtype = torch.bfloat16, fmt: str = "mxfp8",
                                     quantized: bool = False) -> int:
    """Bytes of scratch mul_mxfp4_native_invariant uses (petit_gemm_native_invariant_workspace_bytes): the quantised bytes of a 16-bit A plus
    the split form's slabs, each rounded up to 256; 0 for a call that would be refused."""
    _check(fmt in _QFORMATS, "fmt must be 'mxfp8', 'mxfp6' or 'mxfp4'")
    return int(_lib.lib.petit_gemm_native_invariant_workspace_bytes(int(size_m), int(size_n), int(size_k), _a_type(dtype), _QFORMATS[fmt],
                                                                    int(bool(quantized))))


def mul_mxfp4_native_invariant(A, B, s, global_scale, size_m, size_n, size_k, fmt="mxfp8", bias=None, activation=None) -> torch.Tensor:
    """The native class's GEMM by the batch-invariant entry (petit_gemm_mxfp4_native_invariant, include/petit_amd.h "Batch-invariant GEMM on
    the native class"): MXFP4 weights against activations quantised to `fmt`, a row's result independent of size_m, of the row's position and
    of the launch form.  A: a 16-bit [size_m, size_k] tensor (quantised by the call) or QuantizedActivations of the same fmt -- the same bits
    either way.  Opt-in; no solution_id."""
    return _mul_invariant(A, B, s, global_scale, size_m, size_n, size_k, bias, activation, "mx", fmt)


def _native_output(rows: int, size_m: int, n_out: int, out_quantized, dtype, dev):
    """(the tensor the call writes, what the caller returns): 16-bit [rows, n_out], or with out_quantized the bytes of the quantised
    [size_m, n_out] rows and the QuantizedActivations around them."""
    if out_quantized:
        c = torch.empty(int(_lib.lib.petit_quantized_activation_bytes(size_m, n_out, _QFORMATS[out_quantized])), dtype=torch.uint8, device=dev)
        return c, QuantizedActivations(c, size_m, n_out, out_quantized, dtype)
    c = torch.empty((rows, n_out), dtype=dtype, device=dev)
    return c, c


def _check_packed(B, s, size_n: int, size_k: int, group, num_experts=None) -> None:
    """B holds the packed [size_n, size_k] FP4 weights and s one scale per `group` of k (None: s is not looked at) -- with num_experts,
    of that many matrices back to back."""
    count, what = (1, "") if num_experts is None else (num_experts, "num_experts * ")
    _check(B.is_contiguous() and B.numel() * B.element_size() == count * size_n * size_k // 2,
           f"B does not hold {what}size_n * size_k packed 4-bit weights")
    if group:
        _check(s is not None and s.is_cuda and s.is_contiguous() and s.numel() * s.element_size() == count * size_n * size_k // group,
               f"s does not hold {what}size_n * size_k / {group} scales")


def _mul_native(fn, workspace_bytes, name: str, kind: str, A, weights, global_scale, size_m, size_n, size_k, solution_id, bias, activation,
                out_quantized):
    """The dense call on the native class behind mul_mxfp4_native / mul_nvfp4_native / mul_nvfp4_native_transient.  weights: (B, s), the
    packed tensors of `kind` ('mx' / 'nv'), or (image,); fn / workspace_bytes: the C entry point and its scratch query."""
    a_t, dtype, a_fmt = _activation_operand(A, size_m, size_k)
    _check(a_fmt or (A.is_cuda and A.is_contiguous() and A.numel() == size_m * size_k and A.dtype in (torch.bfloat16, torch.float16)),
           "A must be a contiguous [size_m, size_k] bfloat16 / float16 GPU tensor")
    dev = a_t.device
    _check(all(t.is_cuda for t in weights) and global_scale.is_cuda, "all tensors must be on GPU")
    if len(weights) == 2:
        _check_packed(*weights, size_n, size_k, 32 if kind == "mx" else 16)
    else:
        image, = weights
        _check(image.is_contiguous() and image.dtype == torch.uint8 and
               image.numel() == int(_lib.lib.petit_nvfp4_native_image_bytes(size_k, size_n)) and image.numel() > 0,
               "image does not hold the native image of size_n x size_k NVFP4 weights")
    act = _activation(activation)
    out_fmt = _quantized_format(out_quantized, "out_quantized must be None, 'mxfp8', 'mxfp6' or 'mxfp4'")
    _check(not out_fmt or act, "out_quantized needs activation='silu_mul' or 'swiglu_oai'")
    hints = _hints(kind, dtype)
    sid = C.c_uint64(_c_solution_id(solution_id, native_ok=True))
    epi = _epilogue(bias, act, dev, dtype, size_n, "bias must be a contiguous [size_n] tensor of the activation dtype on the same device")
    na = _lib.NativeArgs(C.sizeof(_lib.NativeArgs), a_fmt, out_fmt, 0)
    c, result = _native_output(size_m, size_m, size_n // 2 if act else size_n, out_quantized, dtype, dev)
    ws_bytes = int(workspace_bytes(C.byref(hints), size_m, size_n, size_k, sid, epi, C.byref(na)))
    ws = _scratch(ws_bytes, dev)
    with torch.cuda.device(dev):
        err = fn(_ptr(c), _ptr(a_t), *map(_ptr, weights), _ptr(global_scale), size_m, size_n, size_k, C.byref(hints), sid, epi, C.byref(na),
                 _opt_ptr(ws), C.c_uint64(ws_bytes), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if err:
        _raise_gemm(err, name, solution_id, f"m={size_m}, n={size_n}, k={size_k}")
    return result


def mul_mxfp4_native(A, B, s, global_scale, size_m, size_n, size_k, solution_id=SOLUTION_AUTO_NATIVE_MXFP4, bias=None, activation=None,
                     out_quantized=None):
    """The native-FP4 class with its hand-over points (petit_gemm_mxfp4_native).  A: a 16-bit [size_m, size_k] tensor (quantised
    by the call: two launches) or QuantizedActivations (one launch).  out_quantized 'mxfp8' / 'mxfp6' / 'mxfp4' (with activation='silu_mul'):
    returns QuantizedActivations [size_m, size_n / 2] for the next GEMM instead of a 16-bit tensor.
    solution_id: SOLUTION_AUTO_NATIVE_MXFP8 / _MXFP4 / _MXFP6 (-2 / -3 / -4) or an explicit native kernel id."""
    return _mul_native(_lib.lib.petit_gemm_mxfp4_native, _lib.lib.petit_gemm_native_workspace_bytes, "mul_mxfp4_native", "mx", A, (B, s),
                       global_scale, size_m, size_n, size_k, solution_id, bias, activation, out_quantized)


# --- NVFP4 weights on the native class (include/petit_amd.h "NVFP4 weights on the native class"; no counterpart in the reference) ----------

_attached_images = {}   # data_ptr of the packed weights -> the image tensor (kept alive for as long as it is attached)


def nvfp4_native_image(B: torch.Tensor, s: torch.Tensor, size_n: int, size_k: int) -> torch.Tensor:
    """The MFMA-native image ("petit-cdna4-nv6/1": FP6 e2m3 elements + one E8M0 scale per 32 k, 6.25 bits per weight) of NVFP4 weights,
    from the PACKED tensors of repack_nvfp4 / process_nvfp4_scales; one launch, once at load time.  An opaque uint8 tensor."""
    _check(B.is_cuda and s.is_cuda and B.device == s.device, "B and s must be GPU tensors on one device")
    _check_packed(B, s, size_n, size_k, 16)
    nbytes = int(_lib.lib.petit_nvfp4_native_image_bytes(size_k, size_n))
    if nbytes == 0:
        raise RuntimeError(f"Incompatible problem shape (n={size_n}, k={size_k})")
    image = torch.empty(nbytes, dtype=torch.uint8, device=B.device)
    with torch.cuda.device(B.device):
        rc = _lib.lib.petit_nvfp4_native_image(_ptr(image), _ptr(B), _ptr(s), size_k, size_n, _stream(B))
    if rc == _lib.PETIT_ERROR_PROBLEM_SHAPE:
        raise RuntimeError(f"Incompatible problem shape (n={size_n}, k={size_k})")
    _raise_on(rc, "nvfp4_native_image")
    return image


def attach_nvfp4_native(B: torch.Tensor, image) -> None:
    """Attach `image` (nvfp4_native_image) to the packed weights B: mul_nvfp4_a16(..., B, ..., solution_id = -2 / -3 / -4) then runs the native
    class on it (MXFP8 / MXFP4 / MXFP6 activations).  image = None detaches.  The image is kept alive while attached; detach before B is freed."""
    key = B.data_ptr()
    if image is None:
        _attached_images.pop(key, None)
        _raise_on(_lib.lib.petit_nvfp4_native_attach(C.c_void_p(key), None), "attach_nvfp4_native")
        return
    _check(image.is_cuda and image.device == B.device and image.dtype == torch.uint8 and image.is_contiguous(), "image must come from nvfp4_native_image")
    _raise_on(_lib.lib.petit_nvfp4_native_attach(C.c_void_p(key), _ptr(image)), "attach_nvfp4_native")
    _attached_images[key] = image


def mul_nvfp4_native(A, image: torch.Tensor, global_scale, size_m, size_n, size_k, solution_id=SOLUTION_AUTO_NATIVE_MXFP8, bias=None,
                     activation=None, out_quantized=None):
    """NVFP4 weights on the block-scaled MFMA (petit_gemm_nvfp4_native): `image` from nvfp4_native_image; everything else as mul_mxfp4_native
    (A a 16-bit tensor or QuantizedActivations; solution_id -2 / -3 / -4 = MXFP8 / MXFP4 / MXFP6 activations or an explicit native id of the
    NVFP4 family; out_quantized with activation='silu_mul')."""
    return _mul_native(_lib.lib.petit_gemm_nvfp4_native, _lib.lib.petit_gemm_native_workspace_bytes, "mul_nvfp4_native", "nv", A, (image,),
                       global_scale, size_m, size_n, size_k, solution_id, bias, activation, out_quantized)


def nvfp4_native_transient_workspace_bytes(size_m, size_n, size_k, solution_id=SOLUTION_AUTO_NATIVE_MXFP8, dtype=torch.bfloat16, activation=None,
                                           a_format=None, out_quantized=None) -> int:
    """Workspace bytes of mul_nvfp4_native_transient (petit_gemm_nvfp4_native_transient_workspace_bytes): the image rounded up to 256 bytes, then the
    native call's own scratch; 0 when the call would be refused.  a_format: the format of pre-quantised activations (None: 16-bit)."""
    _activation(activation)
    a_fmt = _quantized_format(a_format, "a_format must be None, 'mxfp8', 'mxfp6' or 'mxfp4'")
    out_fmt = _quantized_format(out_quantized, "out_quantized must be None, 'mxfp8', 'mxfp6' or 'mxfp4'")
    hints = _hints("nv", dtype)
    na = _lib.NativeArgs(C.sizeof(_lib.NativeArgs), a_fmt, out_fmt, 0)
    return int(_lib.lib.petit_gemm_nvfp4_native_transient_workspace_bytes(C.byref(hints), size_m, size_n, size_k,
                                                                          C.c_uint64(_c_solution_id(solution_id, native_ok=True)),
                                                                          _query_epilogue(activation), C.byref(na)))


def mul_nvfp4_native_transient(A, B, s, global_scale, size_m, size_n, size_k, solution_id=SOLUTION_AUTO_NATIVE_MXFP8, bias=None, activation=None,
                               out_quantized=None):
    """NVFP4 weights on the block-scaled MFMA WITHOUT a resident image (petit_gemm_nvfp4_native_transient): B / s are the packed tensors
    mul_nvfp4_a16 takes; the call builds the image into a workspace it takes from torch's caching allocator, then runs the native call on it.
    Bit for bit mul_nvfp4_a16(..., solution_id) with the image attached (16-bit A and result) / mul_nvfp4_native on the image (QuantizedActivations
    A, out_quantized).  Everything else as mul_nvfp4_native."""
    return _mul_native(_lib.lib.petit_gemm_nvfp4_native_transient, _lib.lib.petit_gemm_nvfp4_native_transient_workspace_bytes,
                       "mul_nvfp4_native_transient", "nv", A, (B, s), global_scale, size_m, size_n, size_k, solution_id, bias, activation,
                       out_quantized)


# --- the batch-invariant native class on NVFP4 images (include/petit_amd.h "Batch-invariant native-class GEMM and MoE launch on NVFP4 images") ---

def mul_nvfp4_native_invariant(A, image, global_scale, size_m, size_n, size_k, fmt="mxfp8", bias=None, activation=None) -> torch.Tensor:
    """mul_mxfp4_native_invariant for NVFP4 weights (petit_gemm_nvfp4_native_invariant): `image` from nvfp4_native_image, global_scale NVFP4's
    real one.  A row's result is a pure function of that row, the image, the scale and the bias -- never of size_m, of the row's position or
    of the launch form; the accuracy class of mul_nvfp4_native.  The queries native_invariant_slabs / native_invariant_workspace_bytes
    answer for this entry too.  Opt-in; no solution_id (profiles/nvfp4_native_invariant.md has the price)."""
    return _mul_invariant(A, image, None, global_scale, size_m, size_n, size_k, bias, activation, "nv", fmt)


def mul_nvfp4_native_moe_invariant(A, images, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index=None,
                                   c_row_index=None, c_rows=None, fmt="mxfp8", bias=None, activation=None) -> torch.Tensor:
    """mul_mxfp4_native_moe_invariant for NVFP4 experts (petit_gemm_nvfp4_native_moe_invariant): `images` from nvfp4_native_images (expert e's
    image at byte e * nvfp4_native_image_bytes).  Every written row equals, bit for bit, mul_nvfp4_native_invariant(size_m=1) on its row and
    its expert's image, global scale and bias."""
    return _mul_invariant(A, images, None, global_scales, size_m, size_n, size_k, bias, activation, "nv", fmt,
                          (expert_offsets, num_experts, a_row_index, c_row_index, c_rows, None))


# --- grouped launch (include/petit_amd.h "Grouped launch"; no counterpart in the reference) ---------------------------------

def mul_fp4_a16_grouped(kind: str, A: torch.Tensor, members, size_m: int, size_k: int, solution_id: int = -1) -> list:
    """Up to 8 GEMMs that share the activations A [size_m, size_k] in ONE launch (size_m <= 16): `members` is a list of
    (B, s, global_scale, size_n) or (B, s, global_scale, size_n, bias) with tensors from repack_* / process_*_scales of `kind`
    ('nvfp4' / 'mxfp4').  Returns the list of outputs [size_m, size_n_i]; bit-identical to separate calls with the same kernel."""
    _check(kind in ("nvfp4", "mxfp4"), "kind must be 'nvfp4' or 'mxfp4'")
    _check(A.dtype in (torch.bfloat16, torch.float16), "A must be bfloat16 or float16.")
    _check(A.is_cuda and A.is_contiguous() and A.numel() == size_m * size_k, "A must be a contiguous [size_m, size_k] tensor")
    _check(1 <= len(members) <= 8, "a group holds 1 to 8 members")
    group = 16 if kind == "nvfp4" else 32
    arr = (_lib.GroupMember * len(members))()
    outs = []
    for i, mem in enumerate(members):
        B, s, gs, n = mem[:4]
        bias = mem[4] if len(mem) > 4 else None
        _check(B.is_cuda and s.is_cuda and gs.is_cuda and B.device == A.device, "all tensors must be on A's GPU")
        _check_packed(B, s, n, size_k, group)
        _check(gs.dtype == torch.float32 and gs.numel() >= 1, "global_scale must be float32")
        if bias is not None:
            _check(bias.is_cuda and bias.dtype == A.dtype and bias.is_contiguous() and bias.numel() == n, "bias must be a contiguous [size_n] tensor of A's dtype")
        c = torch.empty((size_m, n), dtype=A.dtype, device=A.device)
        outs.append(c)
        arr[i] = _lib.GroupMember(c.data_ptr(), B.data_ptr(), s.data_ptr(), gs.data_ptr(), bias.data_ptr() if bias is not None else None, n, 0)
    hints = _hints(kind, A.dtype)
    with torch.cuda.device(A.device):
        err = _lib.lib.petit_gemm_fp4_fp16_grouped(arr, len(members), _ptr(A), size_m, size_k, C.byref(hints), C.c_uint64(_c_solution_id(solution_id)),
                                                   _stream(A))
    if err:
        _raise_gemm(err, "mul_fp4_a16_grouped", solution_id, f"m={size_m}, k={size_k}, n={[mem[3] for mem in members]}")
    return outs


# --- routed-expert (MoE) launch (include/petit_amd.h "Routed-expert (MoE) launch"; no counterpart in the reference) ------------------------

def _check_expert_operands(kind: str, a_t, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, row_indices=(),
                           native: bool = False, transient: bool = False) -> int:
    """The rules the routed-expert launches share, on everything but the activations' shape: the expert count (returned as an int), the
    stacked weights -- packed B / s of `kind` ('nv' / 'mx'), or on the native class with kind 'nv' the experts' images (unless the call is
    transient and brings the packed tensors) --, one global scale
    per expert, the E + 1 offsets, and int32 [size_m] row indices on the activations' device.  a_t: the activation tensor."""
    E = int(num_experts)
    _check(1 <= E <= _lib.PETIT_MOE_MAX_EXPERTS, f"num_experts must be in 1..{_lib.PETIT_MOE_MAX_EXPERTS}, got {E}")
    if native:   # (s is None with images, and otherwise answers for itself below)
        _check(a_t.is_cuda and B.is_cuda and global_scales.is_cuda and expert_offsets.is_cuda and B.is_contiguous(), "all tensors must be on GPU")
    else:
        _check(a_t.is_cuda and B.is_cuda and s.is_cuda and global_scales.is_cuda and expert_offsets.is_cuda, "all tensors must be on GPU")
    if native and kind == "nv" and not transient:
        per = int(_lib.lib.petit_nvfp4_native_image_bytes(size_k, size_n))
        _check(B.dtype == torch.uint8 and per > 0 and B.numel() == E * per, "images do not hold num_experts native images (nvfp4_native_images)")
    else:
        _check_packed(B, s, size_n, size_k, 32 if kind == "mx" else 16, E)
    _check(global_scales.dtype == torch.float32 and global_scales.is_contiguous() and global_scales.numel() == E,
           "global_scales must be a contiguous float32 [num_experts] tensor")
    _check(expert_offsets.dtype == torch.int32 and expert_offsets.is_contiguous() and expert_offsets.numel() == E + 1,
           "expert_offsets must be a contiguous int32 [num_experts + 1] tensor")
    for idx in row_indices:
        if idx is not None:
            _check(idx.is_cuda and idx.device == a_t.device and idx.dtype == torch.int32 and idx.is_contiguous() and idx.numel() == size_m,
                   "row indices must be contiguous int32 [size_m] tensors on A's device")
    return E


def _mul_moe(kind: str, A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, solution_id=-1, bias=None,
             activation=None) -> torch.Tensor:
    """All experts of a MoE layer in one launch: rows expert_offsets[e] .. expert_offsets[e+1]-1 of A (grouped by expert) times expert e's
    weights.  B / s: the experts' packed tensors back to back (repack / process the stacked [E * size_n, size_k] tensors in one call);
    global_scales: float32 [E]; expert_offsets: int32 [E + 1] on A's device, never read by the host (no sync: capturable)."""
    if A.dtype != torch.bfloat16 and A.dtype != torch.float16:
        raise RuntimeError("A must be bfloat16 or float16.")
    E = _check_expert_operands(kind, A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts)
    _check(A.is_contiguous() and A.numel() == size_m * size_k, "A must be a contiguous [size_m, size_k] tensor")
    act = _activation(activation, size_n)
    epi = _epilogue(bias, act, A.device, A.dtype, E * size_n, "bias must be a contiguous [num_experts, size_n] tensor of A's dtype on A's device")
    c = torch.empty((size_m, size_n // 2 if act else size_n), dtype=A.dtype, device=A.device)
    hints = _hints(kind, A.dtype)
    with torch.cuda.device(A.device):
        err = _lib.lib.petit_gemm_fp4_fp16_moe(_ptr(c), _ptr(A), _ptr(B), _ptr(s), _ptr(global_scales), _ptr(expert_offsets), E, size_m, size_n,
                                               size_k, C.byref(hints), C.c_uint64(_c_solution_id(solution_id)),
                                               epi, _stream(A))
    if err:
        _raise_gemm(err, "mul_%sfp4_a16_moe" % kind, solution_id, f"m={size_m}, n={size_n}, k={size_k}, num_experts={E}")
    return c


def mul_nvfp4_a16_moe(A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, solution_id=-1, bias=None,
                      activation=None) -> torch.Tensor:
    return _mul_moe("nv", A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, solution_id, bias, activation)


def mul_mxfp4_a16_moe(A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, solution_id=-1, bias=None,
                      activation=None) -> torch.Tensor:
    return _mul_moe("mx", A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, solution_id, bias, activation)


def _mul_moe_indexed(kind: str, A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index=None,
                     c_row_index=None, c_rows=None, solution_id=-1, bias=None, activation=None, out=None) -> torch.Tensor:
    """The MoE launch with a row gather on A and a row scatter on C (petit_gemm_fp4_fp16_moe_ex): grouped row r reads row a_row_index[r]
    of A [a_rows, size_k] and writes row c_row_index[r] of the output [c_rows, n_out] (None: the identity).  An index outside the
    matrix reads zeros / stores nothing.  out: write into this tensor (rows no index names stay untouched) instead of a new one."""
    if A.dtype != torch.bfloat16 and A.dtype != torch.float16:
        raise RuntimeError("A must be bfloat16 or float16.")
    E = _check_expert_operands(kind, A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, (a_row_index, c_row_index))
    _check(A.is_contiguous() and size_k > 0 and A.numel() % size_k == 0, "A must be a contiguous [a_rows, size_k] tensor")
    act = _activation(activation, size_n)
    epi = _epilogue(bias, act, A.device, A.dtype, E * size_n, "bias must be a contiguous [num_experts, size_n] tensor of A's dtype on A's device")
    a_rows = A.numel() // size_k
    n_out = size_n // 2 if act else size_n
    if out is not None:
        _check(out.is_cuda and out.device == A.device and out.dtype == A.dtype and out.is_contiguous() and out.dim() == 2 and out.size(1) == n_out,
               "out must be a contiguous [c_rows, n_out] tensor of A's dtype on A's device")
        _check(c_rows is None or c_rows < 0 or c_rows == out.size(0), "c_rows does not match out.size(0)")
        c_rows = out.size(0)
    else:
        c_rows = size_m if c_rows is None or c_rows < 0 else int(c_rows)
        out = torch.empty((c_rows, n_out), dtype=A.dtype, device=A.device)
    hints = _hints(kind, A.dtype)
    with torch.cuda.device(A.device):
        err = _lib.lib.petit_gemm_fp4_fp16_moe_ex(_ptr(out), _ptr(A), _ptr(B), _ptr(s), _ptr(global_scales), _ptr(expert_offsets), E, size_m,
                                                  size_n, size_k, _opt_ptr(a_row_index), a_rows, _opt_ptr(c_row_index), c_rows, C.byref(hints),
                                                  C.c_uint64(_c_solution_id(solution_id)), epi, _stream(A))
    if err:
        _raise_gemm(err, "mul_%sfp4_a16_moe_indexed" % kind, solution_id,
                    f"m={size_m}, n={size_n}, k={size_k}, num_experts={E}, a_rows={a_rows}, c_rows={c_rows}")
    return out


def mul_nvfp4_a16_moe_indexed(A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index=None, c_row_index=None,
                              c_rows=None, solution_id=-1, bias=None, activation=None, out=None) -> torch.Tensor:
    return _mul_moe_indexed("nv", A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index, c_rows,
                            solution_id, bias, activation, out)


def mul_mxfp4_a16_moe_indexed(A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index=None, c_row_index=None,
                              c_rows=None, solution_id=-1, bias=None, activation=None, out=None) -> torch.Tensor:
    return _mul_moe_indexed("mx", A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index, c_rows,
                            solution_id, bias, activation, out)


# --- the batch-invariant MoE launch (include/petit_amd.h "Batch-invariant MoE launch"; no counterpart in the reference) ---------------------

def moe_invariant_form(size_m: int, num_experts: int) -> int:
    """The form a batch-invariant MoE call of size_m grouped rows over num_experts gets (petit_gemm_moe_invariant_form): 1 split, 0 whole.
    Both forms give the same bits; the switch is a speed choice."""
    return int(_lib.lib.petit_gemm_moe_invariant_form(int(size_m), int(num_experts)))


def moe_invariant_workspace_bytes(num_experts: int, size_m: int, size_n: int, size_k: int, dtype: torch.dtype = torch.bfloat16,
                                  kind: str = "nvfp4") -> int:
    """Bytes of scratch the batch-invariant MoE call uses (petit_gemm_moe_invariant_workspace_bytes): the split form's slabs; 0 for the
    whole form and for a call that would be refused."""
    return int(_lib.lib.petit_gemm_moe_invariant_workspace_bytes(int(num_experts), int(size_m), int(size_n), int(size_k), _a_type(dtype),
                                                                 _B_TYPES[kind]))


def mul_nvfp4_a16_moe_invariant(A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index=None,
                                c_row_index=None, c_rows=None, bias=None, activation=None, out=None) -> torch.Tensor:
    """mul_nvfp4_a16_moe_indexed by the batch-invariant entry (petit_gemm_fp4_fp16_moe_invariant): every written row equals, bit for bit,
    mul_nvfp4_a16_invariant(size_m=1) on its A row and its expert's tensors -- whatever else is in the batch and wherever the row sits.
    Opt-in and slower than the default pick (profiles/moe_invariant.md); no solution_id."""
    return _mul_invariant(A, B, s, global_scales, size_m, size_n, size_k, bias, activation, "nv",
                          experts=(expert_offsets, num_experts, a_row_index, c_row_index, c_rows, out))


def mul_mxfp4_a16_moe_invariant(A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index=None,
                                c_row_index=None, c_rows=None, bias=None, activation=None, out=None) -> torch.Tensor:
    """The same for MXFP4 experts (petit_gemm_mxfp4_fp16_moe_invariant); bfloat16 activations only."""
    return _mul_invariant(A, B, s, global_scales, size_m, size_n, size_k, bias, activation, "mx",
                          experts=(expert_offsets, num_experts, a_row_index, c_row_index, c_rows, out))


# --- the batch-invariant MoE launch on the native class (include/petit_amd.h "Batch-invariant MoE launch on the native class") --------------

def native_moe_invariant_form(size_m: int, num_experts: int) -> int:
    """The form a native-class batch-invariant MoE call of size_m grouped rows over num_experts gets
    (petit_gemm_native_moe_invariant_form): 1 split, 0 whole.  Both forms give the same bits; the switch is a speed choice."""
    return int(_lib.lib.petit_gemm_native_moe_invariant_form(int(size_m), int(num_experts)))


def native_moe_invariant_workspace_bytes(num_experts: int, size_m: int, size_n: int, size_k: int, dtype: torch.dtype = torch.bfloat16,
                                         fmt: str = "mxfp8", quantized: bool = False) -> int:
    """Bytes of scratch mul_mxfp4_native_moe_invariant uses (petit_gemm_native_moe_invariant_workspace_bytes): the quantised bytes of a 16-bit
    A plus the split form's slabs, each rounded up to 256; 0 for a call that would be refused."""
    _check(fmt in _QFORMATS, "fmt must be 'mxfp8', 'mxfp6' or 'mxfp4'")
    return int(_lib.lib.petit_gemm_native_moe_invariant_workspace_bytes(int(num_experts), int(size_m), int(size_n), int(size_k), _a_type(dtype),
                                                                        _QFORMATS[fmt], int(bool(quantized))))


def mul_mxfp4_native_moe_invariant(A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index=None,
                                   c_row_index=None, c_rows=None, fmt="mxfp8", bias=None, activation=None) -> torch.Tensor:
    """The native class's MoE GEMM by the batch-invariant entry (petit_gemm_mxfp4_native_moe_invariant, include/petit_amd.h "Batch-invariant
    MoE launch on the native class"): every written row equals, bit for bit, mul_mxfp4_native_invariant(size_m=1) on its row and its expert's
    tensors -- whatever else is in the batch and wherever the row sits.  A: a 16-bit [a_rows, size_k] tensor (gathered through a_row_index and
    quantised by the call) or QuantizedActivations of the size_m grouped rows (quantize_activation_rows) -- the same bits either way.
    Opt-in; no solution_id (profiles/native_moe_invariant.md has the price)."""
    return _mul_invariant(A, B, s, global_scales, size_m, size_n, size_k, bias, activation, "mx", fmt,
                          (expert_offsets, num_experts, a_row_index, c_row_index, c_rows, None))


def _check_topk_ids(topk_ids: torch.Tensor, num_experts: int) -> None:
    _check(1 <= int(num_experts) <= _lib.PETIT_MOE_MAX_EXPERTS, f"num_experts must be in 1..{_lib.PETIT_MOE_MAX_EXPERTS}, got {num_experts}")
    _check(topk_ids.is_cuda and topk_ids.dim() == 2 and topk_ids.is_contiguous() and topk_ids.dtype in (torch.int32, torch.int64),
           "topk_ids must be a contiguous int32 / int64 [num_tokens, topk] GPU tensor")
    _check(topk_ids.size(1) >= 1, "topk must be >= 1")


def moe_align_device(topk_ids: torch.Tensor, num_experts: int):
    """moe_align on the device (petit_moe_align): topk_ids [T, topk] int32 / int64 -> (sorted_pos, expert_offsets, token_index), all int32.
    sorted_pos [T * topk]: the flat (token, slot) positions grouped by expert, stable; token_index = sorted_pos // topk; expert_offsets
    [E + 1].  Ids outside [0, E) (-1 under expert parallelism) get no row: expert_offsets[E] counts the routed entries, and the rows past
    it are -1.  No host sync; deterministic."""
    _check_topk_ids(topk_ids, num_experts)
    T, topk = topk_ids.shape
    dev = topk_ids.device
    sorted_pos = torch.empty(T * topk, dtype=torch.int32, device=dev)
    token_index = torch.empty(T * topk, dtype=torch.int32, device=dev)
    offsets = torch.empty(int(num_experts) + 1, dtype=torch.int32, device=dev)
    ws_bytes = int(_lib.lib.petit_moe_align_workspace_bytes(T, topk, int(num_experts)))
    ws = _scratch(ws_bytes, dev)
    with torch.cuda.device(dev):
        rc = _lib.lib.petit_moe_align(_ptr(topk_ids), int(topk_ids.dtype == torch.int64), T, topk, int(num_experts), _ptr(offsets),
                                      _ptr(sorted_pos), _ptr(token_index), _opt_ptr(ws), _stream(topk_ids))
    if rc == _lib.PETIT_ERROR_PROBLEM_SHAPE:
        raise RuntimeError(f"Incompatible routing shape (num_tokens={T}, topk={topk}, num_experts={num_experts})")
    _raise_on(rc, "moe_align_device")
    return sorted_pos, offsets, token_index


def moe_combine(slot_out: torch.Tensor, topk_weights: torch.Tensor, topk_ids: torch.Tensor, num_experts: int) -> torch.Tensor:
    """The top-k reduce (petit_moe_combine): out[t] = to16(sum over j in order, ids in [0, E) only, of float(slot_out[t * topk + j]) *
    topk_weights[t, j]) in fp32 without FMA contraction, one RNE rounding.  slot_out [T * topk, n] bf16 / fp16, topk_weights float32
    [T, topk].  Returns [T, n] in slot_out's dtype."""
    _check_topk_ids(topk_ids, num_experts)
    T, topk = topk_ids.shape
    _check(slot_out.is_cuda and slot_out.device == topk_ids.device and slot_out.dtype in (torch.bfloat16, torch.float16) and
           slot_out.is_contiguous() and slot_out.dim() == 2 and slot_out.size(0) == T * topk,
           "slot_out must be a contiguous bfloat16 / float16 [num_tokens * topk, n] tensor on topk_ids' device")
    _check(topk_weights.is_cuda and topk_weights.device == topk_ids.device and topk_weights.dtype == torch.float32 and
           topk_weights.is_contiguous() and topk_weights.shape == topk_ids.shape, "topk_weights must be a contiguous float32 [num_tokens, topk] tensor")
    n = slot_out.size(1)
    _check(n % 8 == 0, f"n must be a multiple of 8, got {n}")
    out = torch.empty((T, n), dtype=slot_out.dtype, device=slot_out.device)
    with torch.cuda.device(slot_out.device):
        rc = _lib.lib.petit_moe_combine(_ptr(out), _ptr(slot_out), _ptr(topk_weights), _ptr(topk_ids), int(topk_ids.dtype == torch.int64), T, topk,
                                        n, int(num_experts), _a_type(slot_out.dtype), _stream(slot_out))
    if rc == _lib.PETIT_ERROR_PROBLEM_SHAPE:
        raise RuntimeError(f"Incompatible routing shape (num_tokens={T}, topk={topk}, n={n}, num_experts={num_experts})")
    _raise_on(rc, "moe_combine")
    return out


def _combine_norm_operands(slot_out, topk_weights, topk_ids, num_experts, weight, eps, fmt, residual, weight_offset, on_gpu: bool):
    """The argument checks of moe_combine_rmsnorm and of its CPU twin, stated once -> (T, topk, k)."""
    where = "GPU" if on_gpu else "CPU"
    _check(fmt is None or fmt in _QFORMATS, "fmt must be None, 'mxfp8', 'mxfp6' or 'mxfp4'")
    _check(1 <= int(num_experts) <= _lib.PETIT_MOE_MAX_EXPERTS, f"num_experts must be in 1..{_lib.PETIT_MOE_MAX_EXPERTS}, got {num_experts}")
    _check(topk_ids.is_cuda == on_gpu and topk_ids.dim() == 2 and topk_ids.is_contiguous() and topk_ids.dtype in (torch.int32, torch.int64),
           f"topk_ids must be a contiguous int32 / int64 [num_tokens, topk] {where} tensor")
    T, topk = topk_ids.shape
    _check(topk >= 1, "topk must be >= 1")
    _check(slot_out.device == topk_ids.device and slot_out.dtype in (torch.bfloat16, torch.float16) and slot_out.is_contiguous() and
           slot_out.dim() == 2 and slot_out.size(0) == T * topk,
           "slot_out must be a contiguous bfloat16 / float16 [num_tokens * topk, k] tensor on topk_ids' device")
    _check(topk_weights.device == topk_ids.device and topk_weights.dtype == torch.float32 and topk_weights.is_contiguous() and
           topk_weights.shape == topk_ids.shape, "topk_weights must be a contiguous float32 [num_tokens, topk] tensor on topk_ids' device")
    k = slot_out.size(1)
    _check(k % 8 == 0, f"k must be a multiple of 8, got {k}")
    _check(fmt is None or k % 256 == 0, f"k must be a multiple of 256 with a fmt, got {k}")
    _check(weight.device == slot_out.device and weight.is_contiguous() and weight.dtype == slot_out.dtype and tuple(weight.shape) == (k,),
           f"weight must be a contiguous [k] tensor of slot_out's dtype on its device (k={k})")
    _check(residual is None or (residual.device == slot_out.device and residual.is_contiguous() and residual.dtype == slot_out.dtype and
                                tuple(residual.shape) == (T, k)),
           "residual must be a contiguous [num_tokens, k] tensor of slot_out's dtype on its device")
    _check(math.isfinite(eps) and eps > 0, "eps must be finite and positive")
    _check(math.isfinite(weight_offset), "weight_offset must be finite")
    return T, topk, k


def _combine_norm_returns(fmt, residual, return_normed, return_hidden, inplace_residual):
    """What the call returns besides the quantised bytes -> (h wanted, y16 wanted), the defaults resolved."""
    want_y = fmt is None if return_normed is None else bool(return_normed)
    want_h = residual is not None if return_hidden is None else bool(return_hidden)
    _check(fmt is not None or want_y, "fmt=None returns the 16-bit y: return_normed cannot be False")
    _check(not inplace_residual or residual is not None, "inplace_residual needs a residual")
    _check(not inplace_residual or want_h, "inplace_residual writes h: return_hidden cannot be False")
    return want_h, want_y


def _combine_norm_outputs(slot_out, T, k, fmt, residual, want_h, want_y, inplace_residual):
    qa = None
    if fmt is not None:
        qa = torch.empty(int(_lib.lib.petit_quantized_activation_bytes(T, k, _QFORMATS[fmt])), dtype=torch.uint8, device=slot_out.device)
    res_out = None if not want_h else residual if inplace_residual else torch.empty((T, k), dtype=slot_out.dtype, device=slot_out.device)
    y16 = torch.empty((T, k), dtype=slot_out.dtype, device=slot_out.device) if want_y else None
    return qa, res_out, y16


def _combine_norm_result(rc, name, dtype, T, topk, k, num_experts, fmt, qa, res_out, y16):
    if rc == _lib.PETIT_ERROR_PROBLEM_SHAPE:
        raise RuntimeError(f"Incompatible problem shape (num_tokens={T}, topk={topk}, k={k}, num_experts={num_experts})")
    if rc == _lib.PETIT_ERROR_KERNEL_SHAPE:
        raise RuntimeError(f"No kernel implementation for k={k} (the fused norm holds a row of at most 16384 elements).")
    _raise_on(rc, name)
    out = () if qa is None else (QuantizedActivations(qa, T, k, fmt, dtype),)
    out += tuple(t for t in (res_out, y16) if t is not None)
    return out[0] if len(out) == 1 else out


def moe_combine_rmsnorm(slot_out: torch.Tensor, topk_weights: torch.Tensor, topk_ids: torch.Tensor, num_experts: int, weight: torch.Tensor,
                        eps: float = 1e-6, fmt: str = None, *, residual: torch.Tensor = None, weight_offset: float = 0.0,
                        return_normed: bool = None, return_hidden: bool = None, inplace_residual: bool = False):
    """moe_combine, the residual add, the RMSNorm and (with fmt) quantize_activations in ONE launch (include/petit_amd.h "Top-k combine into the
    norm"): c = moe_combine(slot_out, topk_weights, topk_ids, num_experts), h = c (+ residual), y = RMSNorm(h) * (weight + weight_offset) -- bit
    for bit moe_combine -> rmsnorm_quantize(residual=...) where that chain takes the call.  fmt None: no quantised output, any k % 8 == 0.
    Returns, in this order and alone when it is one: the QuantizedActivations when fmt is given; h when return_hidden (default: when a residual
    is given; without a residual h is the combined layer output; `residual` itself, written in place, with inplace_residual=True); the 16-bit y
    when return_normed (default, and always: when fmt is None)."""
    T, topk, k = _combine_norm_operands(slot_out, topk_weights, topk_ids, num_experts, weight, eps, fmt, residual, weight_offset, on_gpu=True)
    want_h, want_y = _combine_norm_returns(fmt, residual, return_normed, return_hidden, inplace_residual)
    qa, res_out, y16 = _combine_norm_outputs(slot_out, T, k, fmt, residual, want_h, want_y, inplace_residual)
    with torch.cuda.device(slot_out.device):
        rc = _lib.lib.petit_moe_combine_rmsnorm(_opt_ptr(qa), _opt_ptr(y16), _opt_ptr(res_out), _ptr(slot_out), _ptr(topk_weights), _ptr(topk_ids),
                                                int(topk_ids.dtype == torch.int64), _opt_ptr(residual), _ptr(weight), float(eps),
                                                float(weight_offset), T, topk, k, int(num_experts), _a_type(slot_out.dtype),
                                                _QFORMATS[fmt] if fmt else 0, _stream(slot_out))
    return _combine_norm_result(rc, "moe_combine_rmsnorm", slot_out.dtype, T, topk, k, num_experts, fmt, qa, res_out, y16)


_SCORINGS = {"softmax": _lib.PETIT_ROUTE_SOFTMAX, "sigmoid": _lib.PETIT_ROUTE_SIGMOID}
_LOGIT_DTYPES = {torch.float32: _lib.PETIT_DTYPE_FP32, torch.bfloat16: _lib.CXX_DTYPE_BF16, torch.float16: _lib.CXX_DTYPE_FP16}


def _check_route(router_logits, topk, scoring, bias, n_group, topk_group):
    """The argument checks of moe_route / moe_route_align (the same texts as csrc/torch_binding.cpp); returns (T, E)."""
    _check_scoring(scoring)
    _check(router_logits.is_cuda and router_logits.dim() == 2 and router_logits.is_contiguous() and router_logits.dtype in _LOGIT_DTYPES,
           "router_logits must be a contiguous float32 / bfloat16 / float16 [num_tokens, num_experts] GPU tensor")
    T, E = router_logits.shape
    _check_route_args(E, router_logits.device, topk, scoring, bias, n_group, topk_group)
    return T, E


def _check_scoring(scoring):
    _check(scoring in _SCORINGS, "scoring must be 'softmax' or 'sigmoid'")


def _check_route_args(E, dev, topk, scoring, bias, n_group, topk_group):
    """What a routing asks of everything but its logits (E experts, on device dev); moe_route_hidden has no logits tensor to show."""
    _check(1 <= E <= _lib.PETIT_MOE_MAX_EXPERTS, f"num_experts must be in 1..{_lib.PETIT_MOE_MAX_EXPERTS}, got {E}")
    _check(1 <= int(topk) <= min(E, _lib.PETIT_MOE_MAX_TOPK), f"topk must be in 1..min(num_experts, {_lib.PETIT_MOE_MAX_TOPK}), got {topk}")
    _check(int(n_group) >= 1 and int(topk_group) >= 1, "n_group and topk_group must be >= 1")
    if bias is not None:
        _check(scoring == "sigmoid", "bias needs scoring='sigmoid'")
        _check(bias.is_cuda and bias.device == dev and bias.dtype == torch.float32 and bias.is_contiguous() and
               tuple(bias.shape) == (E,), "bias must be a contiguous float32 [num_experts] tensor on router_logits' device")


def _route_desc(scoring, renormalize, bias, n_group, topk_group, routed_scaling_factor):
    return _lib.RouteDesc(_SCORINGS[scoring], int(bool(renormalize)), int(n_group), int(topk_group), float(routed_scaling_factor),
                          bias.data_ptr() if bias is not None else None)


def _route_shape_error(rc, T, E, topk, n_group, topk_group):
    if rc == _lib.PETIT_ERROR_PROBLEM_SHAPE:
        raise RuntimeError(f"Incompatible routing shape (num_tokens={T}, num_experts={E}, topk={topk}, n_group={n_group}, topk_group={topk_group})")


def moe_route(router_logits: torch.Tensor, topk: int, scoring: str = "softmax", renormalize: bool = True, bias: torch.Tensor = None,
              n_group: int = 1, topk_group: int = 1, routed_scaling_factor: float = 1.0, return_keys: bool = False):
    """Router logits [T, E] (float32 / bfloat16 / float16) -> (topk_weights float32 [T, topk], topk_ids int32 [T, topk][, keys float32 [T, E]])
    by petit_moe_route (include/petit_amd.h "Routing on the device, from the router's logits": the scorings, the tie rule -- larger key first,
    the lower index among equal keys --, the accuracy of the weights).  One launch, no host sync, deterministic."""
    T, E = _check_route(router_logits, topk, scoring, bias, n_group, topk_group)
    dev = router_logits.device
    ids = torch.empty((T, int(topk)), dtype=torch.int32, device=dev)
    w = torch.empty((T, int(topk)), dtype=torch.float32, device=dev)
    keys = torch.empty((T, E), dtype=torch.float32, device=dev) if return_keys else None
    desc = _route_desc(scoring, renormalize, bias, n_group, topk_group, routed_scaling_factor)
    with torch.cuda.device(dev):
        rc = _lib.lib.petit_moe_route(_ptr(router_logits), _LOGIT_DTYPES[router_logits.dtype], T, E, int(topk), C.byref(desc), _ptr(ids), _ptr(w),
                                      _opt_ptr(keys), _stream(router_logits))
    _route_shape_error(rc, T, E, topk, n_group, topk_group)
    _raise_on(rc, "moe_route")
    return (w, ids, keys) if return_keys else (w, ids)


def moe_route_align(router_logits: torch.Tensor, topk: int, scoring: str = "softmax", renormalize: bool = True, bias: torch.Tensor = None,
                    n_group: int = 1, topk_group: int = 1, routed_scaling_factor: float = 1.0, return_keys: bool = False):
    """moe_route followed by moe_align_device on its ids, bit for bit: (topk_weights, topk_ids, sorted_pos, expert_offsets, token_index[, keys]).
    ONE launch when T * topk <= 1024 (petit_moe_route_align: the align's workgroup routes first), four above."""
    T, E = _check_route(router_logits, topk, scoring, bias, n_group, topk_group)
    dev = router_logits.device
    topk = int(topk)
    ids = torch.empty((T, topk), dtype=torch.int32, device=dev)
    w = torch.empty((T, topk), dtype=torch.float32, device=dev)
    keys = torch.empty((T, E), dtype=torch.float32, device=dev) if return_keys else None
    sorted_pos = torch.empty(T * topk, dtype=torch.int32, device=dev)
    token_index = torch.empty(T * topk, dtype=torch.int32, device=dev)
    offsets = torch.empty(E + 1, dtype=torch.int32, device=dev)
    ws_bytes = int(_lib.lib.petit_moe_route_align_workspace_bytes(T, topk, E))
    ws = _scratch(ws_bytes, dev)
    desc = _route_desc(scoring, renormalize, bias, n_group, topk_group, routed_scaling_factor)
    with torch.cuda.device(dev):
        rc = _lib.lib.petit_moe_route_align(_ptr(router_logits), _LOGIT_DTYPES[router_logits.dtype], T, E, topk, C.byref(desc), _ptr(ids), _ptr(w),
                                            _opt_ptr(keys), _ptr(offsets), _ptr(sorted_pos), _ptr(token_index), _opt_ptr(ws),
                                            _stream(router_logits))
    _route_shape_error(rc, T, E, topk, n_group, topk_group)
    _raise_on(rc, "moe_route_align")
    out = (w, ids, sorted_pos, offsets, token_index)
    return out + (keys,) if return_keys else out


def _check_route_slots(router_logits, topk, E, expert_map, num_local_experts, num_shared, shared_gate_logits):
    """The argument checks of the slot list of moe_route_ex / moe_route_align_ex (the same texts as csrc/torch_binding.cpp); returns (L, S)."""
    return _check_route_slot_args(router_logits.size(0), E, router_logits.device, router_logits.dtype, topk, expert_map, num_local_experts,
                                  num_shared, shared_gate_logits)


def _check_route_slot_args(T, E, dev, logits_dtype, topk, expert_map, num_local_experts, num_shared, shared_gate_logits):
    """The slot list's checks for T tokens and E experts on device dev, the logits (and a shared gate's) being logits_dtype."""
    S = int(num_shared)
    L = E if num_local_experts is None or int(num_local_experts) <= 0 else int(num_local_experts)   # (None, -1 or 0: num_experts, as the C ABI's 0)
    _check(S >= 0 and int(topk) + S <= _lib.PETIT_MOE_MAX_TOPK, f"topk + num_shared must be in 1..{_lib.PETIT_MOE_MAX_TOPK}, got {int(topk) + S}")
    _check(1 <= L <= E and L + S <= _lib.PETIT_MOE_MAX_EXPERTS,
           f"num_local_experts must be in 1..num_experts with num_local_experts + num_shared <= {_lib.PETIT_MOE_MAX_EXPERTS}, got {L}")
    if expert_map is None:
        _check(L == E, "num_local_experts needs an expert_map")
    else:
        _check(expert_map.is_cuda and expert_map.device == dev and expert_map.dtype == torch.int32 and
               expert_map.is_contiguous() and tuple(expert_map.shape) == (E,),
               "expert_map must be a contiguous int32 [num_experts] tensor on router_logits' device")
    if shared_gate_logits is not None:
        _check(S >= 1, "shared_gate_logits needs num_shared >= 1")
        _check(shared_gate_logits.is_cuda and shared_gate_logits.device == dev and
               shared_gate_logits.dtype == logits_dtype and shared_gate_logits.is_contiguous() and
               tuple(shared_gate_logits.shape) == (T, S),
               "shared_gate_logits must be a contiguous [num_tokens, num_shared] tensor of router_logits' dtype on its device")
    return L, S


def _route_slots(expert_map, L, S, shared_weight, shared_gate_logits):
    return _lib.RouteSlots(expert_map.data_ptr() if expert_map is not None else None, L, S, float(shared_weight),
                           shared_gate_logits.data_ptr() if shared_gate_logits is not None else None)


def moe_route_ex(router_logits: torch.Tensor, topk: int, scoring: str = "softmax", renormalize: bool = True, bias: torch.Tensor = None,
                 n_group: int = 1, topk_group: int = 1, routed_scaling_factor: float = 1.0, return_keys: bool = False,
                 expert_map: torch.Tensor = None, num_local_experts: int = None, num_shared: int = 0, shared_weight: float = 1.0,
                 shared_gate_logits: torch.Tensor = None):
    """moe_route writing the complete slot list (petit_moe_route_ex, include/petit_amd.h "The complete slot list in the route launch"):
    topk_weights / topk_ids [T, topk + num_shared]; the routed ids through expert_map (int32 [E], global -> local, -1 when outside
    [0, num_local_experts)), then the shared slots num_local_experts + s with weight shared_weight (* sigmoid(shared_gate_logits[t, s]))."""
    T, E = _check_route(router_logits, topk, scoring, bias, n_group, topk_group)
    L, S = _check_route_slots(router_logits, topk, E, expert_map, num_local_experts, num_shared, shared_gate_logits)
    dev = router_logits.device
    ids = torch.empty((T, int(topk) + S), dtype=torch.int32, device=dev)
    w = torch.empty((T, int(topk) + S), dtype=torch.float32, device=dev)
    keys = torch.empty((T, E), dtype=torch.float32, device=dev) if return_keys else None
    desc = _route_desc(scoring, renormalize, bias, n_group, topk_group, routed_scaling_factor)
    slots = _route_slots(expert_map, L, S, shared_weight, shared_gate_logits)
    with torch.cuda.device(dev):
        rc = _lib.lib.petit_moe_route_ex(_ptr(router_logits), _LOGIT_DTYPES[router_logits.dtype], T, E, int(topk), C.byref(desc), C.byref(slots),
                                         _ptr(ids), _ptr(w), _opt_ptr(keys), _stream(router_logits))
    _route_shape_error(rc, T, E, topk, n_group, topk_group)
    _raise_on(rc, "moe_route_ex")
    return (w, ids, keys) if return_keys else (w, ids)


def moe_route_align_ex(router_logits: torch.Tensor, topk: int, scoring: str = "softmax", renormalize: bool = True, bias: torch.Tensor = None,
                       n_group: int = 1, topk_group: int = 1, routed_scaling_factor: float = 1.0, return_keys: bool = False,
                       expert_map: torch.Tensor = None, num_local_experts: int = None, num_shared: int = 0, shared_weight: float = 1.0,
                       shared_gate_logits: torch.Tensor = None):
    """moe_route_ex followed by moe_align_device(ids, num_local_experts + num_shared), bit for bit (petit_moe_route_align_ex): ONE launch when
    T * (topk + num_shared) <= 1024, four above.  expert_offsets has num_local_experts + num_shared + 1 entries."""
    T, E = _check_route(router_logits, topk, scoring, bias, n_group, topk_group)
    L, S = _check_route_slots(router_logits, topk, E, expert_map, num_local_experts, num_shared, shared_gate_logits)
    dev = router_logits.device
    topk = int(topk)
    n_slots = topk + S
    ids = torch.empty((T, n_slots), dtype=torch.int32, device=dev)
    w = torch.empty((T, n_slots), dtype=torch.float32, device=dev)
    keys = torch.empty((T, E), dtype=torch.float32, device=dev) if return_keys else None
    sorted_pos = torch.empty(T * n_slots, dtype=torch.int32, device=dev)
    token_index = torch.empty(T * n_slots, dtype=torch.int32, device=dev)
    offsets = torch.empty(L + S + 1, dtype=torch.int32, device=dev)
    desc = _route_desc(scoring, renormalize, bias, n_group, topk_group, routed_scaling_factor)
    slots = _route_slots(expert_map, L, S, shared_weight, shared_gate_logits)
    ws_bytes = int(_lib.lib.petit_moe_route_align_ex_workspace_bytes(T, topk, E, C.byref(slots)))
    ws = _scratch(ws_bytes, dev)
    with torch.cuda.device(dev):
        rc = _lib.lib.petit_moe_route_align_ex(_ptr(router_logits), _LOGIT_DTYPES[router_logits.dtype], T, E, topk, C.byref(desc), C.byref(slots),
                                               _ptr(ids), _ptr(w), _opt_ptr(keys), _ptr(offsets), _ptr(sorted_pos), _ptr(token_index),
                                               _opt_ptr(ws), _stream(router_logits))
    _route_shape_error(rc, T, E, topk, n_group, topk_group)
    _raise_on(rc, "moe_route_align_ex")
    out = (w, ids, sorted_pos, offsets, token_index)
    return out + (keys,) if return_keys else out


# --- the router's GEMM (include/petit_amd.h "The router's GEMM"; no counterpart in the reference) -----------------------------------------

def _check_router(hidden, router_weight, router_bias):
    """The argument checks of moe_router_logits / moe_route_hidden, stated here for both operator layers; returns (T, E, K)."""
    _check(hidden.is_cuda and hidden.dim() == 2 and hidden.dtype in (torch.bfloat16, torch.float16),
           "hidden must be a bfloat16 / float16 [num_tokens, k] GPU tensor")
    _check(hidden.is_contiguous(), "hidden must be contiguous")
    _check(router_weight.is_cuda and router_weight.device == hidden.device and router_weight.dim() == 2,
           "router_weight must be a [num_experts, k] tensor on hidden's device")
    _check(router_weight.dtype == hidden.dtype, f"router_weight must have hidden's dtype ({hidden.dtype}), got {router_weight.dtype}")
    _check(router_weight.is_contiguous(), "router_weight must be contiguous")
    (T, K), E = hidden.shape, router_weight.size(0)
    _check(router_weight.size(1) == K, f"router_weight must be [num_experts, {K}] (hidden's k), got {tuple(router_weight.shape)}")
    _check(K % 32 == 0 and 32 <= K <= 16384, f"k must be a multiple of 32 in 32..16384, got {K}")
    _check(1 <= E <= _lib.PETIT_MOE_MAX_EXPERTS, f"num_experts must be in 1..{_lib.PETIT_MOE_MAX_EXPERTS}, got {E}")
    _check(T < 1 << 20, f"num_tokens must be below 2^20, got {T}")
    _check(hidden.data_ptr() % 16 == 0 and router_weight.data_ptr() % 16 == 0, "hidden and router_weight must be 16-byte aligned")
    if router_bias is not None:
        _check(router_bias.is_cuda and router_bias.device == hidden.device and tuple(router_bias.shape) == (E,),
               "router_bias must be a [num_experts] tensor on hidden's device")
        _check(router_bias.dtype == torch.float32, f"router_bias must be float32, got {router_bias.dtype}")
        _check(router_bias.is_contiguous(), "router_bias must be contiguous")
    return T, E, K


def _check_route_hidden(hidden, router_weight, topk, router_bias, scoring, bias, n_group, topk_group, expert_map, num_local_experts, num_shared,
                        shared_gate_logits):
    """moe_route_hidden's checks: the router's, then the routing's on float32 logits that are never stored; returns (T, E, K, L, S)."""
    _check_scoring(scoring)
    T, E, K = _check_router(hidden, router_weight, router_bias)
    _check_route_args(E, hidden.device, topk, scoring, bias, n_group, topk_group)
    L, S = _check_route_slot_args(T, E, hidden.device, torch.float32, topk, expert_map, num_local_experts, num_shared, shared_gate_logits)
    return T, E, K, L, S


def router_geometry(num_experts: int, k: int, dtype: torch.dtype = torch.bfloat16):
    """(S, L) of the router GEMM for (E, K): S slices of L along K (petit_moe_router_geometry) -- functions of the shape alone, never of T."""
    S, L = C.c_uint(0), C.c_uint(0)
    _lib.lib.petit_moe_router_geometry(int(num_experts), int(k), _a_type(dtype), C.byref(S), C.byref(L))
    return S.value, L.value


def router_slabs(num_tokens: int, num_experts: int, k: int, dtype: torch.dtype = torch.bfloat16) -> int:
    """The slab count of the form T tokens get (petit_moe_router_slabs): S in the split form (small T), 1 in the whole form."""
    return int(_lib.lib.petit_moe_router_slabs(int(num_tokens), int(num_experts), int(k), _a_type(dtype)))


def moe_router_logits(hidden: torch.Tensor, router_weight: torch.Tensor, router_bias: torch.Tensor = None) -> torch.Tensor:
    """hidden [T, K] . router_weight [E, K]^T (+ router_bias float32 [E]) -> float32 [T, E] by petit_moe_router_logits (include/petit_amd.h
    "The router's GEMM": fp32 accumulation in an order fixed by (E, K) alone, so a row's logits do not depend on its batch).  bfloat16 or
    float16, both tensors alike and contiguous.  One launch without a bias in the whole form, else two."""
    T, E, K = _check_router(hidden, router_weight, router_bias)
    dev = hidden.device
    logits = torch.empty((T, E), dtype=torch.float32, device=dev)
    a_type = _a_type(hidden.dtype)
    ws = _scratch(int(_lib.lib.petit_moe_router_workspace_bytes(T, E, K, a_type)), dev)
    with torch.cuda.device(dev):
        rc = _lib.lib.petit_moe_router_logits(_ptr(logits), _ptr(hidden), _ptr(router_weight), _opt_ptr(router_bias), a_type, T, E, K,
                                              _opt_ptr(ws), _stream(hidden))
    _raise_on(rc, "moe_router_logits")
    return logits


def moe_route_hidden(hidden: torch.Tensor, router_weight: torch.Tensor, topk: int, router_bias: torch.Tensor = None, align: bool = True,
                     scoring: str = "softmax", renormalize: bool = True, bias: torch.Tensor = None, n_group: int = 1, topk_group: int = 1,
                     routed_scaling_factor: float = 1.0, return_keys: bool = False, expert_map: torch.Tensor = None,
                     num_local_experts: int = None, num_shared: int = 0, shared_weight: float = 1.0, shared_gate_logits: torch.Tensor = None):
    """The routing from the hidden state (petit_moe_route_hidden): what moe_route_align_ex (align=True) or moe_route_ex (align=False) return
    on moe_router_logits(hidden, router_weight, router_bias), bit for bit, in two launches for a decode batch -- the router GEMM, then
    route (+ align) on its partial sums; the logits are never stored.  shared_gate_logits is float32 here."""
    T, E, K, L, S = _check_route_hidden(hidden, router_weight, topk, router_bias, scoring, bias, n_group, topk_group, expert_map,
                                        num_local_experts, num_shared, shared_gate_logits)
    dev = hidden.device
    topk = int(topk)
    n_slots = topk + S
    ids = torch.empty((T, n_slots), dtype=torch.int32, device=dev)
    w = torch.empty((T, n_slots), dtype=torch.float32, device=dev)
    keys = torch.empty((T, E), dtype=torch.float32, device=dev) if return_keys else None
    sorted_pos = torch.empty(T * n_slots, dtype=torch.int32, device=dev) if align else None
    token_index = torch.empty(T * n_slots, dtype=torch.int32, device=dev) if align else None
    offsets = torch.empty(L + S + 1, dtype=torch.int32, device=dev) if align else None
    desc = _route_desc(scoring, renormalize, bias, n_group, topk_group, routed_scaling_factor)
    slots = _route_slots(expert_map, L, S, shared_weight, shared_gate_logits)
    a_type = _a_type(hidden.dtype)
    ws = _scratch(int(_lib.lib.petit_moe_route_hidden_workspace_bytes(T, E, K, a_type, topk, C.byref(slots))), dev)
    with torch.cuda.device(dev):
        rc = _lib.lib.petit_moe_route_hidden(_ptr(hidden), _ptr(router_weight), _opt_ptr(router_bias), a_type, T, E, K, topk, C.byref(desc),
                                             C.byref(slots), _ptr(ids), _ptr(w), _opt_ptr(keys), _opt_ptr(offsets), _opt_ptr(sorted_pos),
                                             _opt_ptr(token_index), _opt_ptr(ws), _stream(hidden))
    _route_shape_error(rc, T, E, topk, n_group, topk_group)
    _raise_on(rc, "moe_route_hidden")
    out = (w, ids, sorted_pos, offsets, token_index) if align else (w, ids)
    return out + (keys,) if return_keys else out


def moe_resolve_solution(hints: PetitSolutionHints, num_experts: int, size_m: int, size_n: int, size_k: int, solution_id: int = -1,
                         activation=None) -> int:
    """The kernel id a MoE call with these arguments runs (petit_gemm_moe_resolve_solution, the launcher's own pick); 0 when it would be refused."""
    ch = _c_hints(hints)
    return int(_lib.lib.petit_gemm_moe_resolve_solution(C.byref(ch), int(num_experts), size_m, size_n, size_k,
                                                        C.c_uint64(_c_solution_id(solution_id)), _query_epilogue(activation)))


# --- native-class MoE (include/petit_amd.h "Native-class MoE launch"; no counterpart in the reference) ------------------------------------

def quantize_activation_rows(A: torch.Tensor, fmt: str = "mxfp8", row_index: torch.Tensor = None, rows: int = None,
                             hadamard: int = 0) -> QuantizedActivations:
    """quantize_activations of gathered rows (petit_quantize_activations_rows): row r of the result is row row_index[r] of A [a_rows, k]
    (None: row r; rows = row_index.numel(), or A's row count).  An index outside [0, a_rows) gives a zero row.  One launch, any row count.
    hadamard: as quantize_activations."""
    _check(fmt in _QFORMATS, "fmt must be 'mxfp8', 'mxfp6' or 'mxfp4'")
    _check(_hadamard_block(hadamard) == 0 or fmt != "mxfp6", _HADAMARD_FP6)
    _check(A.is_cuda and A.is_contiguous() and A.dim() == 2 and A.dtype in (torch.bfloat16, torch.float16),
           "A must be a contiguous 2-D bfloat16 / float16 GPU tensor")
    a_rows, k = A.shape
    if row_index is not None:
        _check(row_index.is_cuda and row_index.device == A.device and row_index.dtype == torch.int32 and row_index.is_contiguous() and
               row_index.dim() == 1, "row_index must be a contiguous int32 1-D tensor on A's device")
        _check(rows is None or rows == row_index.numel(), "rows does not match row_index.numel()")
        m = row_index.numel()
    else:
        m = a_rows if rows is None else int(rows)
    nbytes = int(_lib.lib.petit_quantized_activation_bytes(m, k, _QFORMATS[fmt]))
    qa = torch.empty(nbytes, dtype=torch.uint8, device=A.device)
    with torch.cuda.device(A.device):
        if hadamard:
            rc = _lib.lib.petit_quantize_activations_rows_rot(_ptr(qa), _ptr(A), _opt_ptr(row_index), a_rows, m, k, _a_type(A.dtype),
                                                              _QFORMATS[fmt], hadamard, _stream(A))
        else:
            rc = _lib.lib.petit_quantize_activations_rows(_ptr(qa), _ptr(A), _opt_ptr(row_index), a_rows, m, k, _a_type(A.dtype), _QFORMATS[fmt],
                                                          _stream(A))
    if rc == _lib.PETIT_ERROR_PROBLEM_SHAPE:
        raise RuntimeError(f"Incompatible problem shape (m={m}, k={k}, a_rows={a_rows})")
    _raise_on(rc, "quantize_activation_rows")
    return QuantizedActivations(qa, m, k, fmt, A.dtype, hadamard)


def nvfp4_native_images(B: torch.Tensor, s: torch.Tensor, num_experts: int, size_n: int, size_k: int) -> torch.Tensor:
    """The MFMA-native images of E stacked NVFP4 experts, back to back (what mul_nvfp4_native_moe reads): expert e's image is
    nvfp4_native_image of its slice of the stacked packed tensors B / s (repack_nvfp4 / process_nvfp4_scales of [E * size_n, size_k])."""
    E = int(num_experts)
    _check(1 <= E <= _lib.PETIT_MOE_MAX_EXPERTS, f"num_experts must be in 1..{_lib.PETIT_MOE_MAX_EXPERTS}, got {E}")
    _check(B.is_cuda and s.is_cuda and B.is_contiguous() and s.is_contiguous(), "B and s must be contiguous GPU tensors")
    _check_packed(B, s, size_n, size_k, 16, E)
    per = int(_lib.lib.petit_nvfp4_native_image_bytes(size_k, size_n))
    _check(per > 0, f"no native image for size_n={size_n}, size_k={size_k}")
    out = torch.empty(E * per, dtype=torch.uint8, device=B.device)
    with torch.cuda.device(B.device):
        rc = _lib.lib.petit_nvfp4_native_images(_ptr(out), _ptr(B), _ptr(s), E, size_k, size_n, None, 0, _stream(B))
    _raise_on(rc, "nvfp4_native_images")
    return out


def _mul_native_moe(kind: str, A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index=None, c_row_index=None,
                    c_rows=None, solution_id=SOLUTION_AUTO_NATIVE_MXFP8, bias=None, activation=None, out_quantized=None, transient=False,
                    workspace=None):
    """The routed-expert launch on the native class (petit_gemm_native_moe).  A: 16-bit [a_rows, size_k] (gathered through a_row_index and
    quantised by the call: two launches) or QuantizedActivations of the size_m grouped rows (one launch).  Output: 16-bit [c_rows, n_out], row
    c_row_index[r] for grouped row r (None: the identity), or with out_quantized (activation='silu_mul') QuantizedActivations of the grouped
    [size_m, size_n / 2] rows for the next launch.  transient (kind 'nv'): petit_gemm_native_moe_transient on the packed B / s; workspace: the caller's
    scratch for it (a 256-byte aligned uint8 tensor of at least the queried bytes) instead of one from the allocator."""
    a_t, dtype, a_fmt = _activation_operand(A, size_m, size_k)
    fn, workspace_bytes, name = ((_lib.lib.petit_gemm_native_moe_transient, _lib.lib.petit_gemm_native_moe_transient_workspace_bytes,
                                  "mul_nvfp4_native_moe_transient") if transient else
                                 (_lib.lib.petit_gemm_native_moe, _lib.lib.petit_gemm_native_moe_workspace_bytes, "mul_%sfp4_native_moe" % kind))
    if a_fmt:
        _check(a_row_index is None, "quantised activations are grouped rows already: a_row_index must be None")
        a_rows = size_m
    else:
        _check(A.is_cuda and A.is_contiguous() and A.dtype in (torch.bfloat16, torch.float16) and size_k > 0 and A.numel() % size_k == 0,
               "A must be a contiguous [a_rows, size_k] bfloat16 / float16 GPU tensor")
        a_rows = A.numel() // size_k
    dev = a_t.device
    E = _check_expert_operands(kind, a_t, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, (a_row_index, c_row_index),
                               native=True, transient=transient)
    act = _activation(activation)
    out_fmt = _quantized_format(out_quantized, "out_quantized must be None, 'mxfp8', 'mxfp6' or 'mxfp4'")
    _check(not out_fmt or (act and c_row_index is None), "out_quantized needs activation='silu_mul' or 'swiglu_oai' and no c_row_index")
    epi = _epilogue(bias, act, dev, dtype, E * size_n,
                    "bias must be a contiguous [num_experts, size_n] tensor of the activation dtype on the same device")
    hints = _hints(kind, dtype)
    sid = C.c_uint64(_c_solution_id(solution_id, native_ok=True))
    na = _lib.NativeArgs(C.sizeof(_lib.NativeArgs), a_fmt, out_fmt, 0)
    c_rows = size_m if out_fmt or c_rows is None or c_rows < 0 else int(c_rows)
    c, result = _native_output(c_rows, size_m, size_n // 2 if act else size_n, out_quantized, dtype, dev)
    ws_bytes = int(workspace_bytes(C.byref(hints), E, size_m, size_n, size_k, sid, epi, C.byref(na)))
    if workspace is not None:
        _check(transient and workspace.is_cuda and workspace.device == dev and workspace.dtype == torch.uint8 and workspace.is_contiguous() and
               workspace.numel() >= ws_bytes, "workspace must be a contiguous uint8 tensor on A's device of at least the queried bytes")
    ws = workspace if workspace is not None and ws_bytes else _scratch(ws_bytes, dev)
    with torch.cuda.device(dev):
        err = fn(_ptr(c), _ptr(a_t), _ptr(B), _opt_ptr(s), _ptr(global_scales), _ptr(expert_offsets), E, size_m, size_n, size_k,
                 _opt_ptr(a_row_index), a_rows, _opt_ptr(c_row_index), c_rows, C.byref(hints), sid, epi, C.byref(na), _opt_ptr(ws),
                 C.c_uint64(ws_bytes), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if err:
        _raise_gemm(err, name, solution_id,
                    f"m={size_m}, n={size_n}, k={size_k}, num_experts={E}, a_rows={a_rows}, c_rows={c_rows}")
    return result


def mul_mxfp4_native_moe(A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index=None, c_row_index=None,
                         c_rows=None, solution_id=SOLUTION_AUTO_NATIVE_MXFP8, bias=None, activation=None, out_quantized=None):
    return _mul_native_moe("mx", A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index, c_rows,
                           solution_id, bias, activation, out_quantized)


def mul_nvfp4_native_moe(A, images, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index=None, c_row_index=None,
                         c_rows=None, solution_id=SOLUTION_AUTO_NATIVE_MXFP8, bias=None, activation=None, out_quantized=None):
    return _mul_native_moe("nv", A, images, None, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index,
                           c_rows, solution_id, bias, activation, out_quantized)


def mul_nvfp4_native_moe_transient(A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index=None,
                                   c_row_index=None, c_rows=None, solution_id=SOLUTION_AUTO_NATIVE_MXFP8, bias=None, activation=None,
                                   out_quantized=None, workspace=None):
    """mul_nvfp4_native_moe WITHOUT resident images (petit_gemm_native_moe_transient): B / s are the experts' stacked packed tensors, what
    mul_nvfp4_a16_moe takes; the call builds the images of the experts that have rows into a workspace it takes from torch's caching allocator
    (one launch), then runs the native launch on them -- or into `workspace`, a uint8 tensor of at least
    nvfp4_native_moe_transient_workspace_bytes(...) that several calls may share one after the other.  Bit for bit mul_nvfp4_native_moe on
    nvfp4_native_images(B, s, ...)."""
    return _mul_native_moe("nv", A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index, c_rows,
                           solution_id, bias, activation, out_quantized, transient=True, workspace=workspace)


def nvfp4_native_moe_transient_workspace_bytes(num_experts, size_m, size_n, size_k, solution_id=SOLUTION_AUTO_NATIVE_MXFP8, dtype=torch.bfloat16,
                                               activation=None, a_format=None, out_quantized=None) -> int:
    """Workspace bytes of mul_nvfp4_native_moe_transient (petit_gemm_native_moe_transient_workspace_bytes): num_experts images, then the native
    launch's own scratch; 0 when the call would be refused.  a_format: the format of pre-quantised activations (None: 16-bit)."""
    _activation(activation)
    a_fmt = _quantized_format(a_format, "a_format must be None, 'mxfp8', 'mxfp6' or 'mxfp4'")
    out_fmt = _quantized_format(out_quantized, "out_quantized must be None, 'mxfp8', 'mxfp6' or 'mxfp4'")
    hints = _hints("nv", dtype)
    na = _lib.NativeArgs(C.sizeof(_lib.NativeArgs), a_fmt, out_fmt, 0)
    return int(_lib.lib.petit_gemm_native_moe_transient_workspace_bytes(C.byref(hints), int(num_experts), size_m, size_n, size_k,
                                                                        C.c_uint64(_c_solution_id(solution_id, native_ok=True)),
                                                                        _query_epilogue(activation), C.byref(na)))


def native_moe_resolve_solution(hints: PetitSolutionHints, num_experts: int, size_m: int, size_n: int, size_k: int,
                                solution_id: int = SOLUTION_AUTO_NATIVE_MXFP8, activation=None, a_format: str = None, out_quantized: str = None) -> int:
    """The kernel id petit_gemm_native_moe runs for these arguments (the launcher's own pick); 0 when the call would be refused."""
    ch = _c_hints(hints)
    na = _lib.NativeArgs(C.sizeof(_lib.NativeArgs), _QFORMATS[a_format] if a_format else 0, _QFORMATS[out_quantized] if out_quantized else 0, 0)
    return int(_lib.lib.petit_gemm_native_moe_resolve_solution(C.byref(ch), int(num_experts), size_m, size_n, size_k,
                                                               C.c_uint64(_c_solution_id(solution_id, native_ok=True)), _query_epilogue(activation),
                                                               C.byref(na)))

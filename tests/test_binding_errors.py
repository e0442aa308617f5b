"""The error texts of the two operator layers, pinned: petit_kernel.ops (ctypes) and petit_kernel.compiled (torch.ops.petit_kernel.*).

Every row is one call on a small valid problem (zeros: M = 2, N = 64, K = 256, two experts) with exactly ONE rule broken, and the whole
message the caller gets.  Nothing here launches a kernel: a row is refused by an argument check of the layer or by the library's own
validation (a K that is no multiple of 256: PETIT_ERROR_PROBLEM_SHAPE; an id or sentinel the entry point does not serve:
PETIT_ERROR_KERNEL_SHAPE), both of which return before any device work -- and should a row ever pass a check, its pointers and sizes are
those of a valid problem.  The texts are recorded behaviour: they were taken from a run of this table before the layers were refactored.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
M, N, K, E = 2, 64, 256, 2
BF16, F32, I32, U8 = torch.bfloat16, torch.float32, torch.int32, torch.uint8

DENSE = "A B s global_scale size_m size_n size_k solution_id bias activation"
MOE = "A B s global_scales expert_offsets size_m size_n size_k num_experts solution_id bias activation"
INDEXED = "A B s global_scales expert_offsets size_m size_n size_k num_experts a_row_index c_row_index c_rows solution_id bias activation out"
NATIVE_MOE = ("A B s global_scales expert_offsets size_m size_n size_k num_experts a_row_index c_row_index c_rows solution_id bias activation "
              "out_quantized")
NATIVE = "A B s global_scale size_m size_n size_k solution_id bias activation out_quantized"
SIGNATURES = {
    "mul_nvfp4_a16": DENSE, "mul_mxfp4_a16": DENSE, "mul_nvfp4_a16_moe": MOE, "mul_mxfp4_a16_moe": MOE,
    "mul_nvfp4_a16_moe_indexed": INDEXED, "mul_mxfp4_a16_moe_indexed": INDEXED, "mul_mxfp4_native_moe": NATIVE_MOE,
    "mul_nvfp4_native_moe": NATIVE_MOE.replace(" s ", " "), "mul_nvfp4_native_transient": NATIVE, "mul_mxfp4_native": NATIVE,
    "mul_nvfp4_native": NATIVE.replace(" s ", " "),
}


def z(shape, dtype=BF16, dev=DEV):
    if dtype == torch.float8_e4m3fn:
        return torch.zeros(shape, dtype=U8, device=dev).view(dtype)
    return torch.zeros(shape, dtype=dtype, device=dev)


def scales(nv, e, n, k):
    return z((e * n, k // 16), torch.float8_e4m3fn) if nv else z((e * n * k // 32,), U8)


def image_bytes(n, k):
    from petit_kernel import _lib
    return int(_lib.lib.petit_nvfp4_native_image_bytes(k, n))


def qact(m, k, says_m=None, fmt="mxfp8"):
    from petit_kernel import _lib, ops
    nbytes = int(_lib.lib.petit_quantized_activation_bytes(m, k, ops._QFORMATS[fmt]))
    return ops.QuantizedActivations(z((nbytes,), U8), m if says_m is None else says_m, k, fmt, BF16)


def base(entry, n=N, k=K):
    """The arguments of a valid call of `entry`, by name."""
    nv = "nvfp4" in entry
    moe = "moe" in entry
    e = E if moe else 1
    native_sentinel = "native" in entry
    d = dict(A=z((M, k)), B=z((e * n // 16, 2 * k), I32), s=scales(nv, e, n, k), global_scale=z((1,), F32), global_scales=z((e,), F32),
             expert_offsets=z((e + 1,), I32), size_m=M, size_n=n, size_k=k, num_experts=e, a_row_index=None, c_row_index=None, c_rows=None,
             solution_id=-2 if native_sentinel else -1, bias=None, activation=None, out=None, out_quantized=None)
    if entry == "mul_mxfp4_a16":
        d["s"] = z((n // 32, k), U8)
    if entry in ("mul_nvfp4_native", "mul_nvfp4_native_moe"):
        d["B"] = z((e * image_bytes(n, k),), U8)
    return d


def mul(entry, n=N, k=K, **broken):
    """The call of `entry` with the arguments in `broken` replaced (a callable builds its tensor when the row runs)."""
    def run(layer):
        args = base(entry, n, k)
        args.update({name: v() if callable(v) else v for name, v in broken.items()})
        return getattr(layer, entry)(*[args[name] for name in SIGNATURES[entry].split()])
    return run


def call(name, *args, **kwargs):
    """layer.name(*args) for the entry points that are not GEMMs; callables build their tensors when the row runs."""
    def run(layer):
        return getattr(layer, name)(*[a() if callable(a) else a for a in args], **{key: v() if callable(v) else v for key, v in kwargs.items()})
    return run


def hints_with_b_type(b_type):
    def make():
        from petit_kernel import ops
        h = ops.PetitSolutionHints()
        h.a_type, h.b_type = BF16, b_type
        return h
    return make


ACT = "activation must be one of ['none', 'silu_mul', 'swiglu_oai'] or None"
ACT_N = ("silu_mul needs size_n % 32 == 0 (gate / up halves of whole tiles), got 48",
         "silu_mul / swiglu_oai need size_n % 32 == 0 (gate / up halves of whole tiles), got 48")
A16 = "A must be bfloat16 or float16."
ON_GPU = "all tensors must be on GPU"
A_MK = "A must be a contiguous [size_m, size_k] tensor"
A_MK16 = "A must be a contiguous [size_m, size_k] bfloat16 / float16 GPU tensor"
A_ROWS16 = "A must be a contiguous [a_rows, size_k] bfloat16 / float16 GPU tensor"
B_NK = "B does not hold size_n * size_k packed 4-bit weights"
B_ENK = "B does not hold num_experts * size_n * size_k packed 4-bit weights"
GS_E = "global_scales must be a contiguous float32 [num_experts] tensor"
OFF_E = "expert_offsets must be a contiguous int32 [num_experts + 1] tensor"
ROWS = "row indices must be contiguous int32 [size_m] tensors on A's device"
BIAS_E = "bias must be a contiguous [num_experts, size_n] tensor of A's dtype on A's device"
BIAS_E16 = "bias must be a contiguous [num_experts, size_n] tensor of the activation dtype on the same device"
BIAS_16 = "bias must be a contiguous [size_n] tensor of the activation dtype on the same device"
E_RANGE = "num_experts must be in 1..1024, got 0"
OUT_Q = "out_quantized must be None, 'mxfp8', 'mxfp6' or 'mxfp4'"
OUT_Q_ACT = "out_quantized needs activation='silu_mul' or 'swiglu_oai'"
QA_SAYS = "quantised activations are [3, 256], the call says [2, 256]"
FMT = "fmt must be 'mxfp8', 'mxfp6' or 'mxfp4'"
A_2D = "A must be a contiguous 2-D bfloat16 / float16 GPU tensor"
KIND = "kind must be 'nvfp4' or 'mxfp4'"
SHAPE_MNK = "Incompatible problem shape (m=2, n=64, k=128)"
SHAPE_MOE = "Incompatible problem shape (m=2, n=64, k=128, num_experts=2)"
SHAPE_IDX = "Incompatible problem shape (m=2, n=64, k=128, num_experts=2, a_rows=2, c_rows=2)"
NO_KERNEL_1 = "No kernel implementation for solution_id=1."
NO_KERNEL_AUTO = "No kernel implementation for solution_id=-1."
CTYPES_ONLY = None

# (id, the call, the text of the ctypes layer, the text of the compiled layer -- True: the same, CTYPES_ONLY: the entry point is not there)
ROWS_TABLE = [
    # the reference's functions
    ("repack-n", call("repack_nvfp4", lambda: z((8, K // 8), I32), 8, K), "size_n = 8 is not divisible by tile_n_size = 16", True),
    ("repack-k", call("repack_nvfp4", lambda: z((N, 8), I32), N, 64), "size_k = 64 is not divisible by tile_k_size = 128", True),
    ("nv-scales-n", call("process_nvfp4_scales", lambda: z((8, K // 16), torch.float8_e4m3fn), 8, K),
     "size_n = 8 is not divisible by tile_n_size = 16", True),
    ("nv-scales-k", call("process_nvfp4_scales", lambda: z((N, 8), torch.float8_e4m3fn), N, 128),
     "size_k = 128 is not divisible by tile_k_size = 256", True),
    ("nv-scales-rows", call("process_nvfp4_scales", lambda: z((N + 16, K // 16), torch.float8_e4m3fn), N, K),
     "scales.size(0) = 80 is not size_n = 64", True),
    ("nv-scales-cpu", call("process_nvfp4_scales", lambda: z((N, K // 16), torch.float8_e4m3fn, "cpu"), N, K), "scales is not on GPU", True),
    ("nv-scales-strided", call("process_nvfp4_scales", lambda: z((K // 16, N), torch.float8_e4m3fn).t(), N, K), "scales is not contiguous", True),
    ("mx-scales-n", call("process_mxfp4_scales", lambda: z((8, K // 32), U8), 8, K), "size_n = 8 is not divisible by tile_n_size = 16", True),
    ("mx-scales-k", call("process_mxfp4_scales", lambda: z((N, 4), U8), N, 128), "size_k = 128 is not divisible by tile_k_size = 256", True),
    ("mx-scales-rows", call("process_mxfp4_scales", lambda: z((N + 16, K // 32), U8), N, K), "scales.size(0) = 80 is not size_n = 64", True),
    ("mx-scales-cpu", call("process_mxfp4_scales", lambda: z((N, K // 32), U8, "cpu"), N, K), "scales is not on GPU", True),
    ("mx-scales-strided", call("process_mxfp4_scales", lambda: z((K // 32, N), U8).t(), N, K), "scales is not contiguous", True),
    # dense
    ("dense-a-dtype", mul("mul_nvfp4_a16", A=lambda: z((M, K), F32)), A16, True),
    ("dense-mx-a-dtype", mul("mul_mxfp4_a16", A=lambda: z((M, K), F32)), A16, True),
    ("dense-cpu", mul("mul_nvfp4_a16", A=lambda: z((M, K), BF16, "cpu")), ON_GPU, True),
    ("dense-mx-cpu", mul("mul_mxfp4_a16", global_scale=lambda: z((1,), F32, "cpu")), ON_GPU, True),
    ("dense-a-size", mul("mul_nvfp4_a16", A=lambda: z((M + 1, K))), A_MK, True),
    ("dense-b-size", mul("mul_nvfp4_a16", B=lambda: z((N // 16 + 1, 2 * K), I32)), B_NK, True),
    ("dense-s-size", mul("mul_nvfp4_a16", s=lambda: z((N + 1, K // 16), torch.float8_e4m3fn)), "s does not hold size_n * size_k / 16 scales", True),
    ("dense-gs-dtype", mul("mul_nvfp4_a16", global_scale=lambda: z((1,), torch.float16)), "global_scale must be float32", True),
    ("dense-activation", mul("mul_nvfp4_a16", activation="gelu"), ACT, True),
    ("dense-activation-n", mul("mul_nvfp4_a16", n=48, activation="silu_mul"), *ACT_N),
    ("dense-bias", mul("mul_nvfp4_a16", bias=lambda: z((N,), F32)), "bias must be a contiguous [size_n] tensor of A's dtype on A's device", True),
    ("dense-problem-shape", mul("mul_nvfp4_a16", k=128), SHAPE_MNK, True),
    ("dense-kernel-shape", mul("mul_nvfp4_a16", solution_id=1), NO_KERNEL_1, True),
    # MoE
    ("moe-a-dtype", mul("mul_nvfp4_a16_moe", A=lambda: z((M, K), F32)), A16, True),
    ("moe-experts", mul("mul_nvfp4_a16_moe", num_experts=0), E_RANGE, True),
    ("moe-cpu", mul("mul_nvfp4_a16_moe", expert_offsets=lambda: z((E + 1,), I32, "cpu")), ON_GPU, True),
    ("moe-a-size", mul("mul_nvfp4_a16_moe", A=lambda: z((M + 1, K))), A_MK, True),
    ("moe-b-size", mul("mul_nvfp4_a16_moe", B=lambda: z((E * N // 16 + 1, 2 * K), I32)), B_ENK, True),
    ("moe-s-size", mul("mul_nvfp4_a16_moe", s=lambda: z((E * N + 1, K // 16), torch.float8_e4m3fn)),
     "s does not hold num_experts * size_n * size_k / 16 scales", True),
    ("moe-gs", mul("mul_nvfp4_a16_moe", global_scales=lambda: z((E + 1,), F32)), GS_E, True),
    ("moe-offsets", mul("mul_nvfp4_a16_moe", expert_offsets=lambda: z((E,), I32)), OFF_E, True),
    ("moe-activation", mul("mul_nvfp4_a16_moe", activation="gelu"), ACT, True),
    ("moe-activation-n", mul("mul_nvfp4_a16_moe", n=48, activation="silu_mul"), *ACT_N),
    ("moe-bias", mul("mul_nvfp4_a16_moe", bias=lambda: z((E, N), F32)), BIAS_E, True),
    ("moe-problem-shape", mul("mul_nvfp4_a16_moe", k=128), SHAPE_MOE, True),
    ("moe-kernel-shape", mul("mul_nvfp4_a16_moe", solution_id=1), NO_KERNEL_1, True),
    # indexed MoE
    ("indexed-a-dtype", mul("mul_mxfp4_a16_moe_indexed", A=lambda: z((M, K), F32)), A16, True),
    ("indexed-experts", mul("mul_mxfp4_a16_moe_indexed", num_experts=0), E_RANGE, True),
    ("indexed-cpu", mul("mul_mxfp4_a16_moe_indexed", global_scales=lambda: z((E,), F32, "cpu")), ON_GPU, True),
    ("indexed-a-size", mul("mul_mxfp4_a16_moe_indexed", A=lambda: z((M * K + 1,))), "A must be a contiguous [a_rows, size_k] tensor", True),
    ("indexed-b-size", mul("mul_mxfp4_a16_moe_indexed", B=lambda: z((E * N // 16 + 1, 2 * K), I32)), B_ENK, True),
    ("indexed-s-size", mul("mul_mxfp4_a16_moe_indexed", s=lambda: z((E * N * K // 32 + 1,), U8)),
     "s does not hold num_experts * size_n * size_k / 32 scales", True),
    ("indexed-gs", mul("mul_mxfp4_a16_moe_indexed", global_scales=lambda: z((E,), torch.float16)), GS_E, True),
    ("indexed-offsets", mul("mul_mxfp4_a16_moe_indexed", expert_offsets=lambda: z((E + 1,), torch.int64)), OFF_E, True),
    ("indexed-a-rows", mul("mul_mxfp4_a16_moe_indexed", a_row_index=lambda: z((M,), torch.int64)), ROWS, True),
    ("indexed-c-rows", mul("mul_mxfp4_a16_moe_indexed", c_row_index=lambda: z((M + 1,), I32)), ROWS, True),
    ("indexed-activation", mul("mul_mxfp4_a16_moe_indexed", activation="gelu"), ACT, True),
    ("indexed-activation-n", mul("mul_mxfp4_a16_moe_indexed", n=48, activation="silu_mul"), *ACT_N),
    ("indexed-bias", mul("mul_mxfp4_a16_moe_indexed", bias=lambda: z((E, N + 1))), BIAS_E, True),
    ("indexed-out", mul("mul_mxfp4_a16_moe_indexed", out=lambda: z((M, N + 8))),
     "out must be a contiguous [c_rows, n_out] tensor of A's dtype on A's device", True),
    ("indexed-out-rows", mul("mul_mxfp4_a16_moe_indexed", out=lambda: z((M, N)), c_rows=M + 1), "c_rows does not match out.size(0)", True),
    ("indexed-problem-shape", mul("mul_mxfp4_a16_moe_indexed", k=128), SHAPE_IDX, True),
    ("indexed-kernel-shape", mul("mul_mxfp4_a16_moe_indexed", solution_id=1), NO_KERNEL_1, True),
    ("indexed-nv-kernel-shape", mul("mul_nvfp4_a16_moe_indexed", solution_id=1), NO_KERNEL_1, True),
    # native MoE
    ("native-moe-experts", mul("mul_mxfp4_native_moe", num_experts=0), E_RANGE, True),
    ("native-moe-a-dtype", mul("mul_mxfp4_native_moe", A=lambda: z((M, K), F32)), A_ROWS16, A16),
    ("native-moe-a-size", mul("mul_mxfp4_native_moe", A=lambda: z((M * K + 1,))), A_ROWS16, True),
    ("native-moe-cpu", mul("mul_mxfp4_native_moe", expert_offsets=lambda: z((E + 1,), I32, "cpu")), ON_GPU, True),
    ("native-moe-b-size", mul("mul_mxfp4_native_moe", B=lambda: z((E * N // 16 + 1, 2 * K), I32)), B_ENK, True),
    ("native-moe-s-size", mul("mul_mxfp4_native_moe", s=lambda: z((E * N * K // 32 + 1,), U8)),
     "s does not hold num_experts * size_n * size_k / 32 scales", True),
    ("native-moe-images", mul("mul_nvfp4_native_moe", B=lambda: z((256,), U8)),
     "images do not hold num_experts native images (nvfp4_native_images)", True),
    ("native-moe-gs", mul("mul_mxfp4_native_moe", global_scales=lambda: z((E + 1,), F32)), GS_E, True),
    ("native-moe-offsets", mul("mul_mxfp4_native_moe", expert_offsets=lambda: z((E,), I32)), OFF_E, True),
    ("native-moe-rows", mul("mul_mxfp4_native_moe", c_row_index=lambda: z((M,), torch.int64)), ROWS, True),
    ("native-moe-activation", mul("mul_mxfp4_native_moe", activation="gelu"), ACT, True),
    ("native-moe-out-format", mul("mul_mxfp4_native_moe", activation="silu_mul", out_quantized="fp8"), OUT_Q, True),
    ("native-moe-out-needs", mul("mul_mxfp4_native_moe", out_quantized="mxfp8"), OUT_Q_ACT + " and no c_row_index", True),
    ("native-moe-bias", mul("mul_mxfp4_native_moe", bias=lambda: z((E, N), F32)), BIAS_E16, True),
    ("native-moe-qa-says", mul("mul_mxfp4_native_moe", A=lambda: qact(M, K, says_m=M + 1)), QA_SAYS, True),
    ("native-moe-qa-gather", mul("mul_mxfp4_native_moe", A=lambda: qact(M, K), a_row_index=lambda: z((M,), I32)),
     "quantised activations are grouped rows already: a_row_index must be None", True),
    ("native-moe-problem-shape", mul("mul_mxfp4_native_moe", k=128), SHAPE_IDX, True),
    ("native-moe-kernel-shape", mul("mul_mxfp4_native_moe", solution_id=-1), NO_KERNEL_AUTO, True),
    ("native-moe-nv-kernel-shape", mul("mul_nvfp4_native_moe", solution_id=-1), NO_KERNEL_AUTO, True),
    # NVFP4 on the native class without a resident image
    ("transient-a-dtype", mul("mul_nvfp4_native_transient", A=lambda: z((M, K), F32)), A_MK16, A16),
    ("transient-a-size", mul("mul_nvfp4_native_transient", A=lambda: z((M + 1, K))), A_MK16, True),
    ("transient-a-cpu", mul("mul_nvfp4_native_transient", A=lambda: z((M, K), BF16, "cpu")), A_MK16, True),
    ("transient-cpu", mul("mul_nvfp4_native_transient", global_scale=lambda: z((1,), F32, "cpu")), ON_GPU, True),
    ("transient-b-size", mul("mul_nvfp4_native_transient", B=lambda: z((N // 16 + 1, 2 * K), I32)), B_NK, True),
    ("transient-s-size", mul("mul_nvfp4_native_transient", s=lambda: z((N + 1, K // 16), torch.float8_e4m3fn)),
     "s does not hold size_n * size_k / 16 scales", True),
    ("transient-activation", mul("mul_nvfp4_native_transient", activation="gelu"), ACT, True),
    ("transient-out-format", mul("mul_nvfp4_native_transient", activation="silu_mul", out_quantized="fp8"), OUT_Q, True),
    ("transient-out-needs", mul("mul_nvfp4_native_transient", out_quantized="mxfp8"), OUT_Q_ACT, True),
    ("transient-bias", mul("mul_nvfp4_native_transient", bias=lambda: z((N,), F32)), BIAS_16, True),
    ("transient-qa-says", mul("mul_nvfp4_native_transient", A=lambda: qact(M, K, says_m=M + 1)), QA_SAYS, True),
    ("transient-problem-shape", mul("mul_nvfp4_native_transient", k=128), SHAPE_MNK, True),
    ("transient-kernel-shape", mul("mul_nvfp4_native_transient", solution_id=-1), NO_KERNEL_AUTO, True),
    # routing
    ("align-experts", call("moe_align_device", lambda: z((M, 2), I32), 0), E_RANGE, True),
    ("combine-experts", call("moe_combine", lambda: z((2 * M, 8)), lambda: z((M, 2), F32), lambda: z((M, 2), I32), 0), E_RANGE, True),
    ("route-experts", call("moe_route", lambda: z((M, 1025), F32), 2), "num_experts must be in 1..1024, got 1025", True),
    ("route-align-experts", call("moe_route_align", lambda: z((M, 1025), F32), 2), "num_experts must be in 1..1024, got 1025", True),
    # the entry points of the ctypes layer alone
    ("mx-native-a-dtype", mul("mul_mxfp4_native", A=lambda: z((M, K), F32)), A_MK16, CTYPES_ONLY),
    ("mx-native-cpu", mul("mul_mxfp4_native", global_scale=lambda: z((1,), F32, "cpu")), ON_GPU, CTYPES_ONLY),
    ("mx-native-b-size", mul("mul_mxfp4_native", B=lambda: z((N // 16 + 1, 2 * K), I32)), B_NK, CTYPES_ONLY),
    ("mx-native-s-size", mul("mul_mxfp4_native", s=lambda: z((N * K // 32 + 1,), U8)), "s does not hold size_n * size_k / 32 scales", CTYPES_ONLY),
    ("mx-native-activation", mul("mul_mxfp4_native", activation="gelu"), ACT, CTYPES_ONLY),
    ("mx-native-out-format", mul("mul_mxfp4_native", activation="silu_mul", out_quantized="fp8"), OUT_Q, CTYPES_ONLY),
    ("mx-native-out-needs", mul("mul_mxfp4_native", out_quantized="mxfp4"), OUT_Q_ACT, CTYPES_ONLY),
    ("mx-native-bias", mul("mul_mxfp4_native", bias=lambda: z((N + 1,))), BIAS_16, CTYPES_ONLY),
    ("mx-native-qa-says", mul("mul_mxfp4_native", A=lambda: qact(M, K, says_m=M + 1)), QA_SAYS, CTYPES_ONLY),
    ("mx-native-problem-shape", mul("mul_mxfp4_native", k=128), SHAPE_MNK, CTYPES_ONLY),
    ("mx-native-kernel-shape", mul("mul_mxfp4_native", solution_id=-1), NO_KERNEL_AUTO, CTYPES_ONLY),
    ("nv-native-a-dtype", mul("mul_nvfp4_native", A=lambda: z((M, K), F32)), A_MK16, CTYPES_ONLY),
    ("nv-native-cpu", mul("mul_nvfp4_native", global_scale=lambda: z((1,), F32, "cpu")), ON_GPU, CTYPES_ONLY),
    ("nv-native-image", mul("mul_nvfp4_native", B=lambda: z((256,), U8)),
     "image does not hold the native image of size_n x size_k NVFP4 weights", CTYPES_ONLY),
    ("nv-native-out-format", mul("mul_nvfp4_native", activation="silu_mul", out_quantized="fp8"), OUT_Q, CTYPES_ONLY),
    ("nv-native-out-needs", mul("mul_nvfp4_native", out_quantized="mxfp4"), OUT_Q_ACT, CTYPES_ONLY),
    ("nv-native-bias", mul("mul_nvfp4_native", bias=lambda: z((N,), F32)), BIAS_16, CTYPES_ONLY),
    ("nv-native-qa-says", mul("mul_nvfp4_native", A=lambda: qact(M, K, says_m=M + 1)), QA_SAYS, CTYPES_ONLY),
    ("nv-native-kernel-shape", mul("mul_nvfp4_native", solution_id=-1), NO_KERNEL_AUTO, CTYPES_ONLY),
    ("transient-bytes-activation", call("nvfp4_native_transient_workspace_bytes", M, N, K, activation="gelu"), ACT, CTYPES_ONLY),
    ("transient-bytes-out-format", call("nvfp4_native_transient_workspace_bytes", M, N, K, out_quantized="fp8"), OUT_Q, CTYPES_ONLY),
    ("quantize-fmt", call("quantize_activations", lambda: z((M, K)), "fp8"), FMT, CTYPES_ONLY),
    ("quantize-a", call("quantize_activations", lambda: z((M, K), F32)), A_2D, CTYPES_ONLY),
    ("quantize-problem-shape", call("quantize_activations", lambda: z((M, 128))), "Incompatible problem shape (m=2, k=128)", CTYPES_ONLY),
    ("quantize-rows-fmt", call("quantize_activation_rows", lambda: z((M, K)), "fp8"), FMT, CTYPES_ONLY),
    ("quantize-rows-a", call("quantize_activation_rows", lambda: z((M * K,))), A_2D, CTYPES_ONLY),
    ("grouped-kind", call("mul_fp4_a16_grouped", "fp4", lambda: z((M, K)), [], M, K), KIND, CTYPES_ONLY),
    ("grouped-a-dtype", call("mul_fp4_a16_grouped", "nvfp4", lambda: z((M, K), F32), [], M, K), A16, CTYPES_ONLY),
    ("grouped-a-size", call("mul_fp4_a16_grouped", "nvfp4", lambda: z((M + 1, K)), [], M, K), A_MK, CTYPES_ONLY),
    ("grouped-b-size", call("mul_fp4_a16_grouped", "nvfp4", lambda: z((M, K)),
                            lambda: [(z((N // 16 + 1, 2 * K), I32), scales(True, 1, N, K), z((1,), F32), N)], M, K), B_NK, CTYPES_ONLY),
    ("grouped-gs-dtype", call("mul_fp4_a16_grouped", "nvfp4", lambda: z((M, K)),
                              lambda: [(z((N // 16, 2 * K), I32), scales(True, 1, N, K), z((1,), torch.float16), N)], M, K),
     "global_scale must be float32", CTYPES_ONLY),
    ("grouped-kernel-shape", call("mul_fp4_a16_grouped", "nvfp4", lambda: z((17, K)),
                                  lambda: [(z((N // 16, 2 * K), I32), scales(True, 1, N, K), z((1,), F32), N)], 17, K), NO_KERNEL_AUTO, CTYPES_ONLY),
    ("dequant-kind", call("dequant_packed", lambda: z((N // 16, 2 * K), I32), lambda: scales(True, 1, N, K), N, K, "fp4"), KIND, CTYPES_ONLY),
    ("dequant-b-size", call("dequant_packed", lambda: z((N // 16 + 1, 2 * K), I32), lambda: scales(True, 1, N, K), N, K), B_NK, CTYPES_ONLY),
    ("image-b-size", call("nvfp4_native_image", lambda: z((N // 16 + 1, 2 * K), I32), lambda: scales(True, 1, N, K), N, K), B_NK, CTYPES_ONLY),
    ("image-s-size", call("nvfp4_native_image", lambda: z((N // 16, 2 * K), I32), lambda: scales(True, 1, N + 1, K), N, K),
     "s does not hold size_n * size_k / 16 scales", CTYPES_ONLY),
    ("image-problem-shape", call("nvfp4_native_image", lambda: z((N // 16, 256), I32), lambda: scales(True, 1, N, 128), N, 128),
     "Incompatible problem shape (n=64, k=128)", CTYPES_ONLY),
    ("images-experts", call("nvfp4_native_images", lambda: z((E * N // 16, 2 * K), I32), lambda: scales(True, E, N, K), 0, N, K), E_RANGE, CTYPES_ONLY),
    ("images-b-size", call("nvfp4_native_images", lambda: z((E * N // 16 + 1, 2 * K), I32), lambda: scales(True, E, N, K), E, N, K), B_ENK,
     CTYPES_ONLY),
    ("solutions-a-dtype", call("get_fp4_solutions", M, N, K, F32, None), A16, CTYPES_ONLY),
    ("solutions-b-type", call("get_fp4_solutions", hints_with_b_type(torch.float16), M, N, K), "Failed to get solutions: -1", CTYPES_ONLY),
]


def _cases():
    for row_id, run, ctypes_text, compiled_text in ROWS_TABLE:
        yield pytest.param("ops", run, ctypes_text, id=f"ops-{row_id}")
        if compiled_text is not CTYPES_ONLY:
            yield pytest.param("compiled", run, ctypes_text if compiled_text is True else compiled_text, id=f"compiled-{row_id}")


def test_row_ids_are_unique():
    ids = [row[0] for row in ROWS_TABLE]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("layer,run,text", list(_cases()))
def test_one_broken_rule_gives_its_whole_text(layer, run, text):
    import petit_kernel
    from petit_kernel import compiled
    assert compiled.available(), compiled.why_unavailable()
    with pytest.raises(RuntimeError) as caught:
        run(getattr(petit_kernel, layer))
    torch.cuda.synchronize()
    got = str(caught.value)
    print(f"{layer}: {got!r}")
    assert got == text

"""The batch-invariant MoE launch on the native class (include/petit_amd.h "Batch-invariant MoE launch on the native class") without a GPU: the
symbols and their declarations, the form query and the workspace arithmetic, every refusal with its code (all of them precede any launch: none
of these calls has a device), the CPU twin against the dense twin on each row alone -- empty experts, malformed offsets under the clamp rule, a
C index with out-of-range entries --, the two operator layers' signatures and texts, and the layer switch's refusals.
tests/test_native_moe_invariant.py imports the builders below."""
import ctypes as C
import inspect
from pathlib import Path

import numpy as np
import pytest
import torch

from petit_kernel import _lib
from test_native_invariant_abi import (BAD, BF16, FMTS, FP16, MX, NV, OK, PTR, SHAPE, exact_weights, geometry, host_quantize, random_weights, to16,
                                       twin)

L = _lib.lib
ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("petit_gemm_native_moe_invariant_form", "petit_gemm_native_moe_invariant_workspace_bytes", "petit_gemm_mxfp4_native_moe_invariant",
           "petit_gemm_native_moe_invariant_host")
SHAPES = [(64, 1024), (64, 4352), (128, 256), (96, 512)]          # S = 4; S = 9 with a short last slice; S = 1; three pairs of n-tiles
GATED_SHAPES = [(128, 1024), (192, 512)]
EXPERTS = (3, 65, 130)
CASES = [(fmt, is_bf16) for fmt in FMTS for is_bf16 in (True, False)]
IDS = [f"{fmt}-{'bf16' if b else 'fp16'}" for fmt, b in CASES]
POISON16 = 0x7FC1


# --- builders (shared with the GPU module) ---------------------------------------------------------------------------------------------------

class HostExperts:
    """E experts' packed MXFP4 tensors stacked back to back (CPU), their dequantised float64 weights, one global scale and one bias row each."""

    def __init__(self, E, n, k, is_bf16, seed, exact=False, gs=None):
        make = exact_weights if exact else random_weights
        parts = [make(n, k, seed + 7 * e) for e in range(E)]
        self.b_e, self.s_e, self.w = [p[0] for p in parts], [p[1] for p in parts], [p[2] for p in parts]
        self.b = torch.cat([p.contiguous().view(torch.uint8).reshape(-1) for p in self.b_e])
        self.s = torch.cat([p.contiguous().view(torch.uint8).reshape(-1) for p in self.s_e])
        rng = np.random.default_rng([seed, E, n, k, 5])
        self.gs = np.asarray(gs if gs is not None else rng.uniform(0.5, 1.0, E), dtype=np.float32)
        self.bias64 = rng.integers(-8, 9, (E, n)) * 0.5
        self.bias_bits = to16(self.bias64, is_bf16)
        self.E, self.n, self.k, self.is_bf16 = E, n, k, is_bf16


def row_owner(offsets, m):
    """owner[r] = the expert whose clamped range holds grouped row r, or -1: each offset clamped into [its predecessor, m] (a running maximum)."""
    hi = np.minimum(np.maximum.accumulate(np.clip(np.asarray(offsets, dtype=np.int64), 0, None)), m)
    owner = np.searchsorted(hi[1:], np.arange(m), side="right")
    return np.where((np.arange(m) >= hi[0]) & (owner < len(hi) - 1), owner, -1)


def moe_twin(qa, X, offsets, m, c_idx, c_rows, fmt, use_bias=True, out=None):
    """petit_gemm_native_moe_invariant_host on host bytes -> the uint16 patterns of c [c_rows, n] (unwritten rows keep POISON16)"""
    out = np.full((c_rows, X.n), POISON16, dtype=np.uint16) if out is None else out
    off = np.ascontiguousarray(offsets, dtype=np.int32)
    idx = None if c_idx is None else np.ascontiguousarray(c_idx, dtype=np.int32)
    rc = L.petit_gemm_native_moe_invariant_host(out.ctypes.data, qa.ctypes.data, X.b.data_ptr(), X.s.data_ptr(), X.gs.ctypes.data,
                                                X.bias_bits.ctypes.data if use_bias else None, off.ctypes.data, X.E, m, X.n, X.k,
                                                None if idx is None else idx.ctypes.data, c_rows, BF16 if X.is_bf16 else FP16, FMTS[fmt])
    assert rc == OK
    return out


def r256(x):
    return (x + 255) // 256 * 256


# --- the ABI ---------------------------------------------------------------------------------------------------------------------------------

def test_symbols_exist_and_are_declared():
    raw = C.CDLL(str(_lib.LIB_PATH))
    header = (ROOT / "include" / "petit_amd.h").read_text()
    assert "Batch-invariant MoE launch on the native class" in header
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert f" {name}(" in header, name


@pytest.mark.parametrize("a_type", [BF16, FP16])
@pytest.mark.parametrize("n,k", SHAPES + GATED_SHAPES)
def test_workspace_is_the_stated_arithmetic(n, k, a_type):
    S, Lk = geometry(n, k, a_type)
    assert 1 <= S <= 16 and S * Lk >= k > (S - 1) * Lk
    forms = set()
    for E in EXPERTS + (1, 8, 1024):
        for m in list(range(1, 40)) + [63, 64, 65, 200, 4096, 70000]:
            split = L.petit_gemm_native_moe_invariant_form(m, E)
            forms.add(split)
            slab = r256(S * m * n * 4) if split else 0
            for fmt in (8, 6, 4):
                qbytes = m * (k // 8 * fmt) + m * (k // 32)
                assert qbytes == L.petit_quantized_activation_bytes(m, k, fmt)
                assert L.petit_gemm_native_moe_invariant_workspace_bytes(E, m, n, k, a_type, fmt, 0) == r256(qbytes) + slab, (E, m, fmt)
                assert L.petit_gemm_native_moe_invariant_workspace_bytes(E, m, n, k, a_type, fmt, 1) == slab, (E, m, fmt)
    assert forms == {0, 1}
    # refused calls and m == 0 need no workspace
    for args in ((3, 1, n, k + 128, a_type, 8, 0), (3, 1, n + 16, k, a_type, 8, 0), (3, 1, n, k, 3, 8, 0), (3, 0, n, k, a_type, 8, 0),
                 (3, 1, n, k, a_type, 5, 0), (3, 1 << 20, n, k, a_type, 8, 1), (0, 1, n, k, a_type, 8, 0), (1025, 1, n, k, a_type, 8, 0)):
        assert L.petit_gemm_native_moe_invariant_workspace_bytes(*args) == 0, args


def test_shapes_of_the_gpu_module():
    assert geometry(64, 1024) == (4, 256) and geometry(64, 4352) == (9, 512) and geometry(128, 256) == (1, 256)
    want, per = min(16, -(-2048 // (64 // 16))), -(-4352 // 16)
    assert (want, per) == (16, 272) and 4352 % 512 == 256                                   # (64, 4352): last slice 256


def test_the_form_is_a_function_of_m_and_num_experts_alone():
    form = L.petit_gemm_native_moe_invariant_form
    seen = set()
    for E in (1, 2, 3, 8, 65, 128, 130, 1024):
        for m in list(range(0, 80)) + [512, 4096, (1 << 20) - 1]:
            f = form(m, E)
            assert f in (0, 1) and form(m, E) == f
            seen.add(f)
            if m == 0:
                continue
            # whatever else the call says -- shape, types, format, input kind --, the slab part is there exactly in the split form
            for (n, k) in ((64, 1024), (192, 512)):
                for a_type in (BF16, FP16):
                    for fmt in (8, 4):
                        assert (L.petit_gemm_native_moe_invariant_workspace_bytes(E, m, n, k, a_type, fmt, 1) > 0) == bool(f), (E, m, n, k)
    assert seen == {0, 1}


def _call(a_type=BF16, E=3, m=4, n=64, k=256, fmt=8, quantized=0, c=PTR, a=PTR, b=PTR, s=PTR, gs=PTR, off=PTR, a_idx=None, a_rows=16, c_idx=None,
          c_rows=16, hints="auto", epi=None, ws=PTR, c_type=None, b_type=MX):
    if hints == "auto":
        hints = C.byref(_lib.SolutionHints(a_type, b_type, a_type if c_type is None else c_type, 0))
    return L.petit_gemm_mxfp4_native_moe_invariant(c, a, b, s, gs, off, E, m, n, k, a_idx, a_rows, c_idx, c_rows, hints, fmt, quantized, epi, ws,
                                                   None)


@pytest.mark.parametrize("quantized", [0, 1])
@pytest.mark.parametrize("a_type", [BF16, FP16])
def test_refusals_and_their_codes(a_type, quantized):
    """Non-null dummy pointers throughout: a call that got as far as a launch would fault here, so every code comes from before any launch."""
    call = lambda **kw: _call(a_type=a_type, quantized=quantized, **kw)  # noqa: E731
    # the dense native-invariant entry's codes
    assert call(n=48) == SHAPE and call(n=16) == SHAPE and call(n=0) == SHAPE          # n % 32
    assert call(k=128) == SHAPE and call(k=384) == SHAPE and call(k=0) == SHAPE        # k % 256
    assert call(m=1 << 20, a_rows=1 << 20, c_rows=1 << 20) == SHAPE
    for name in ("c", "a", "b", "s"):
        assert call(**{name: None}) == SHAPE, name                                    # null required pointers
        assert call(**{name: C.c_void_p(0x1008)}) == SHAPE, name                      # not 16-byte aligned
    # the byte query is not zero at m = 4 with a 16-bit input (the quantised bytes) and in the split form (the slabs)
    assert L.petit_gemm_native_moe_invariant_workspace_bytes(3, 4, 64, 256, a_type, 8, quantized) > 0
    assert call(ws=None) == SHAPE and call(ws=C.c_void_p(0x1010)) == SHAPE
    assert call(gs=None, m=0, c=None, a=None, b=None, s=None, ws=None) == OK          # m == 0: nothing to do
    assert call(hints=None) == BAD
    assert call(c_type=FP16 if a_type == BF16 else BF16) == BAD
    assert call(b_type=NV) == BAD                                                     # NVFP4 images are not served here
    for fmt in (0, 5, 7, 16, -4):
        assert call(fmt=fmt) == BAD, fmt
    for act in (3, -1, 77):
        assert call(epi=C.byref(_lib.Epilogue(None, act, 0))) == BAD
    assert call(epi=C.byref(_lib.Epilogue(None, 0, 1))) == BAD                        # reserved
    assert call(n=96, epi=C.byref(_lib.Epilogue(None, 1, 0))) == SHAPE                # gated: n % 64
    assert call(n=96, epi=C.byref(_lib.Epilogue(None, 2, 0))) == SHAPE
    assert call(epi=C.byref(_lib.Epilogue(0x1004, 0, 0))) == SHAPE                    # a bias that is not 8-byte aligned
    # the MoE invariant entry's codes
    assert call(E=0) == SHAPE and call(E=1025) == SHAPE
    assert call(gs=None) == SHAPE and call(off=None) == SHAPE
    for name in ("gs", "off", "c_idx") + (() if quantized else ("a_idx",)):
        assert call(**{name: C.c_void_p(0x1002)}) == SHAPE, name                      # not 4-byte aligned
    assert call(c_rows=3) == SHAPE                                                    # a NULL C index with fewer than m rows behind it
    if quantized:
        assert call(a_idx=PTR) == BAD                                                 # quantised bytes are the grouped rows already
    else:
        assert call(a_rows=3) == SHAPE                                                # a NULL A index with fewer than m rows behind it
    # 2^31 workgroups or more: the whole form's (2^14 + 1024) slots x 2^25 / 32 / 2 / 4 n-blocks
    big_m, big_n = (1 << 20) - 1, 1 << 25
    assert call(E=1024, m=big_m, n=big_n, a_rows=big_m, c_rows=big_m) == SHAPE
    # the quantised rows reach 2^32 bytes: m x (k + k / 32) at MXFP8
    assert call(m=1 << 19, k=8192, a_rows=1 << 19, c_rows=1 << 19) == SHAPE
    if not quantized:   # no 65535-row limit on 16-bit input (the dense entry answers KERNEL_SHAPE here): this call gets as far as the pointer checks
        assert call(m=65536, a_rows=65536, c_rows=65536, ws=None) == SHAPE


def test_bad_types_and_the_host_entry():
    for a_type in (NV, _lib.PETIT_DTYPE_FP32, 0, 77):
        assert _call(a_type=a_type) == BAD
    host = L.petit_gemm_native_moe_invariant_host
    assert host(PTR, PTR, PTR, PTR, PTR, None, PTR, 3, 4, 64, 128, None, 4, BF16, 8) == SHAPE
    assert host(PTR, PTR, PTR, PTR, PTR, None, PTR, 3, 4, 48, 256, None, 4, BF16, 8) == SHAPE
    assert host(PTR, PTR, PTR, PTR, PTR, None, PTR, 0, 4, 64, 256, None, 4, BF16, 8) == SHAPE
    assert host(PTR, PTR, PTR, PTR, PTR, None, PTR, 3, 4, 64, 256, None, 3, BF16, 8) == SHAPE      # a NULL C index with fewer than m rows
    assert host(None, PTR, PTR, PTR, PTR, None, PTR, 3, 4, 64, 256, None, 4, BF16, 8) == SHAPE
    assert host(PTR, PTR, PTR, PTR, None, None, PTR, 3, 4, 64, 256, None, 4, BF16, 8) == SHAPE
    assert host(PTR, PTR, PTR, PTR, PTR, None, PTR, 3, 4, 64, 256, None, 4, 0, 8) == BAD
    assert host(PTR, PTR, PTR, PTR, PTR, None, PTR, 3, 4, 64, 256, None, 4, FP16, 5) == BAD
    assert host(None, None, None, None, None, None, None, 3, 0, 64, 256, None, 0, FP16, 6) == OK


# --- the CPU twin ----------------------------------------------------------------------------------------------------------------------------

ROUTINGS = {   # E = 5 unless the offsets say otherwise; m = 12
    "well formed": (0, 3, 3, 7, 12, 12),
    "empty first and last": (0, 0, 5, 5, 12, 12),
    "rows of no expert": (1, 4, 6, 6, 10, 11),
    "descending": (0, 7, 2, 9, 9, 12),
    "negative and beyond m": (-3, 5, -1, 40, 8, 30),
}


@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
@pytest.mark.parametrize("n,k", SHAPES)
def test_twin_equals_the_dense_twin_on_each_row_alone(n, k, fmt, is_bf16):
    m, E = 12, 5
    X = HostExperts(E, n, k, is_bf16, 40)
    bits = to16(np.random.default_rng([n, k, 3]).standard_normal((m, k)), is_bf16, exact=False)
    qa = host_quantize(bits, is_bf16, fmt)                                            # the image of the m grouped rows
    alone = {}

    def dense_row(e, r, use_bias):
        if (e, r, use_bias) not in alone:
            alone[(e, r, use_bias)] = twin(host_quantize(bits[r:r + 1], is_bf16, fmt), X.b_e[e], X.s_e[e], float(X.gs[e]),
                                           X.bias_bits[e] if use_bias else None, 1, n, k, is_bf16, fmt)[0]
        return alone[(e, r, use_bias)]

    c_rows = m + 3
    c_idx = np.random.default_rng(9).permutation(c_rows)[:m].astype(np.int32)
    c_idx[2], c_idx[7] = c_rows, -1                                                   # outside [0, c_rows): stores nothing
    for name, offsets in ROUTINGS.items():
        owner = row_owner(offsets, m)
        assert (owner >= 0).sum() >= 6
        for idx, use_bias in ((None, True), (c_idx, True), (c_idx, False)):
            rows_out = m if idx is None else c_rows
            got = moe_twin(qa, X, offsets, m, idx, rows_out, fmt, use_bias)
            want = np.full((rows_out, n), POISON16, dtype=np.uint16)
            for r in range(m):
                dst = r if idx is None else int(idx[r])
                if owner[r] >= 0 and 0 <= dst < rows_out:
                    want[dst] = dense_row(int(owner[r]), r, use_bias)
            assert np.array_equal(got, want), (name, idx is None, use_bias)


@pytest.mark.parametrize("E", EXPERTS)
def test_twin_crosses_the_expert_chunks(E):
    """One row on experts at the 64-expert chunk boundaries of the slot map, every other expert empty."""
    n, k, fmt, is_bf16 = 64, 256, "mxfp8", True
    X = HostExperts(E, n, k, is_bf16, 50)
    busy = sorted({e for e in (0, 1, 62, 63, 64, 65, 127, 128, 129, E - 1) if e < E})
    counts = np.zeros(E, dtype=np.int64)
    counts[busy] = 1
    m = int(counts.sum())
    offsets = np.concatenate([[0], np.cumsum(counts)])
    bits = to16(np.random.default_rng(E).standard_normal((m, k)), is_bf16, exact=False)
    got = moe_twin(host_quantize(bits, is_bf16, fmt), X, offsets, m, None, m, fmt)
    for r, e in enumerate(busy):
        want = twin(host_quantize(bits[r:r + 1], is_bf16, fmt), X.b_e[e], X.s_e[e], float(X.gs[e]), X.bias_bits[e], 1, n, k, is_bf16, fmt)[0]
        assert np.array_equal(got[r], want), (r, e)


# --- the operator layers ---------------------------------------------------------------------------------------------------------------------

NAMES = ("mul_mxfp4_native_moe_invariant", "native_moe_invariant_form", "native_moe_invariant_workspace_bytes")


def test_both_operator_layers_export_identical_signatures():
    import petit_kernel
    from petit_kernel import compiled, ops
    for name in NAMES:
        assert name in petit_kernel.__all__ and callable(getattr(petit_kernel, name))
        sigs = [inspect.signature(getattr(mod, name)) for mod in (ops, compiled, petit_kernel)]
        rows = [[(p.name, p.default, p.kind) for p in sig.parameters.values()] for sig in sigs]
        assert rows[0] == rows[1], name
        assert [r[0].lower() for r in rows[0]] == [r[0].lower() for r in rows[2]], name
    assert list(inspect.signature(ops.mul_mxfp4_native_moe_invariant).parameters) == [
        "A", "B", "s", "global_scales", "expert_offsets", "size_m", "size_n", "size_k", "num_experts", "a_row_index", "c_row_index", "c_rows", "fmt",
        "bias", "activation"]
    assert inspect.signature(ops.mul_mxfp4_native_moe_invariant).parameters["fmt"].default == "mxfp8"


def test_python_queries_agree_with_the_c_abi():
    from petit_kernel import ops
    for E in EXPERTS:
        for m in (1, 8, 9, 64, 65, 4096):
            assert ops.native_moe_invariant_form(m, E) == L.petit_gemm_native_moe_invariant_form(m, E)
            for (n, k) in SHAPES:
                for fmt, code in FMTS.items():
                    for quantized in (False, True):
                        assert ops.native_moe_invariant_workspace_bytes(E, m, n, k, torch.float16, fmt, quantized) == \
                            L.petit_gemm_native_moe_invariant_workspace_bytes(E, m, n, k, FP16, code, int(quantized))


def _cpu_operands(dtype, E=3, m=4, n=64, k=256, quantized=None):
    from petit_kernel import ops
    A = torch.zeros(m, k, dtype=dtype)
    if quantized:
        A = ops.QuantizedActivations(torch.zeros(m * (k // 8 * FMTS[quantized]) + m * (k // 32), dtype=torch.uint8), m, k, quantized, dtype)
    return dict(A=A, B=torch.zeros(E * n // 16, 2 * k, dtype=torch.int32), s=torch.zeros(E * n * k // 32, dtype=torch.uint8),
                global_scales=torch.ones(E), expert_offsets=torch.zeros(E + 1, dtype=torch.int32), size_m=m, size_n=n, size_k=k, num_experts=E)


BROKEN = [
    ("fmt", lambda o: o.update(fmt="mxfp5"), "fmt must be 'mxfp8', 'mxfp6' or 'mxfp4'"),
    ("dtype", lambda o: o.update(A=o["A"].float()), "A must be bfloat16 or float16"),
    ("experts", lambda o: o.update(num_experts=0), "num_experts must be in 1..1024, got 0"),
    ("k", lambda o: o.update(size_k=128), "Incompatible problem shape (m=4, n=64, k=128)"),
    ("n", lambda o: o.update(size_n=48), "Incompatible problem shape (m=4, n=48, k=256)"),
    ("activation", lambda o: o.update(activation="relu"), "activation must be one of"),
    ("gated n", lambda o: o.update(size_n=96, activation="silu_mul"), "silu_mul needs size_n % 64 == 0"),
    ("A shape", lambda o: o.update(A=o["A"].reshape(-1)[:1000]), "A must be a contiguous [a_rows, size_k] tensor"),
    ("B size", lambda o: o.update(B=o["B"][:1]), "B does not hold num_experts * size_n * size_k packed 4-bit weights"),
    ("s size", lambda o: o.update(s=o["s"][:7]), "s does not hold num_experts * size_n * size_k / 32 scales"),
    ("gs", lambda o: o.update(global_scales=torch.ones(2)), "global_scales must be a contiguous float32 [num_experts] tensor"),
    ("offsets", lambda o: o.update(expert_offsets=torch.zeros(4, dtype=torch.int64)), "expert_offsets must be a contiguous int32 [num_experts + 1] tensor"),
    ("index", lambda o: o.update(c_row_index=torch.zeros(3, dtype=torch.int32)), "row indices must be contiguous int32 [size_m] tensors on A's device"),
    ("rows", lambda o: o.update(c_rows=3), "without a row index the matrix must hold size_m rows (a_rows=4, c_rows=3, m=4)"),
    ("bias", lambda o: o.update(bias=torch.zeros(64, dtype=o["A"].dtype)), "bias must be a contiguous [num_experts, size_n] tensor of A's dtype on A's device"),
    ("device", lambda o: None, "all tensors must be on GPU"),
]
BROKEN_Q = [
    ("fmt mismatch", lambda o: o.update(fmt="mxfp4"), "quantised activations are mxfp8, the call says fmt='mxfp4'"),
    ("shape mismatch", lambda o: o.update(size_m=5), "quantised activations are [4, 256], the call says [5, 256]"),
    ("a index", lambda o: o.update(a_row_index=torch.zeros(4, dtype=torch.int32)), "a_row_index must be None"),
    ("device", lambda o: None, "all tensors must be on GPU"),
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", BROKEN + BROKEN_Q, ids=[b[0] for b in BROKEN] + ["q " + b[0] for b in BROKEN_Q])
def test_both_layers_raise_the_same_texts(case, dtype):
    """The argument checks are stated once (ops._check_invariant) and run by both layers in front of anything that needs a device."""
    from petit_kernel import compiled, ops
    _, breakage, text = case
    messages = []
    for layer in (ops, compiled):
        o = _cpu_operands(dtype, quantized="mxfp8" if case in BROKEN_Q else None)
        breakage(o)
        with pytest.raises(RuntimeError) as e:
            layer.mul_mxfp4_native_moe_invariant(**o)
        messages.append(str(e.value))
    assert messages[0] == messages[1] and text in messages[0], messages


# --- the layer switch ------------------------------------------------------------------------------------------------------------------------

def test_the_native_layer_refuses_images_and_transient():
    from petit_kernel import moe
    assert inspect.signature(moe.fp4_moe_native).parameters["invariant"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(moe.fp4_moe_native).parameters["invariant"].default is False
    x = torch.zeros(2, 256, dtype=torch.bfloat16)
    t = torch.zeros(1)
    ids = torch.zeros(2, 1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="kind 'mxfp4': NVFP4 images have no batch-invariant native kernel"):
        moe.fp4_moe_native(x, t, None, t, t, None, t, torch.ones(2, 1), ids, kind="nvfp4", invariant=True)
    with pytest.raises(RuntimeError, match="does not take transient=True"):
        moe.fp4_moe_native(x, t, t, t, t, t, t, torch.ones(2, 1), ids, kind="nvfp4", transient=True, invariant=True)
    # the routed entry keeps its refusal of the native path, and the gpt-oss block takes the switch
    with pytest.raises(RuntimeError, match="invariant=True is for path 'fused'"):
        moe.fp4_moe_routed(x, torch.zeros(2, 1), t, t, t, t, t, t, 1, "mxfp4", path="native", invariant=True)
    from petit_kernel.gptoss import GptOssExperts
    assert inspect.signature(GptOssExperts.forward).parameters["invariant"].default is False

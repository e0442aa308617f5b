"""The batch-invariant MoE launch (include/petit_amd.h "Batch-invariant MoE launch") without a GPU: the symbols, every refusal with its code
(all of them precede any launch: none of these calls has a device), the form switch and the workspace arithmetic, the two operator layers'
signatures and texts, and the CPU twin against the dense CPU twin run per owned row, under well-formed and malformed offsets."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from petit_kernel import _lib, offline

FP16, BF16 = _lib.CXX_DTYPE_FP16, _lib.CXX_DTYPE_BF16
NV, MX = _lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_MXFP4_E2M1
OK, SHAPE, KERNEL, BAD = _lib.PETIT_OK, _lib.PETIT_ERROR_PROBLEM_SHAPE, _lib.PETIT_ERROR_KERNEL_SHAPE, _lib.PETIT_ERROR_BAD_ARGUMENT
SYMBOLS = ("petit_gemm_fp4_fp16_moe_invariant", "petit_gemm_mxfp4_fp16_moe_invariant", "petit_gemm_moe_invariant_workspace_bytes",
           "petit_gemm_moe_invariant_form", "petit_gemm_fp4_moe_invariant_host")
PAIRS = [(BF16, NV), (BF16, MX), (FP16, NV)]
L = _lib.lib
PTR = C.c_void_p(0x1000)   # a non-null, 256-byte aligned pointer for calls that are refused before anything reads it


def test_symbols_exist():
    raw = C.CDLL(str(_lib.LIB_PATH))
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTED_SYMBOLS


def _geometry(n, k, a_type=BF16, b_type=NV):
    S, Lk = C.c_uint(0), C.c_uint(0)
    L.petit_gemm_invariant_geometry(n, k, a_type, b_type, C.byref(S), C.byref(Lk))
    return S.value, Lk.value


def _call(a_type=BF16, b_type=NV, E=4, m=4, n=32, k=256, c=PTR, a=PTR, b=PTR, s=PTR, gs=PTR, off=PTR, a_idx=None, a_rows=4, c_idx=None,
          c_rows=4, hints="auto", epi=None, ws=PTR, c_type=None, hints_b=None):
    fn = L.petit_gemm_mxfp4_fp16_moe_invariant if b_type == MX else L.petit_gemm_fp4_fp16_moe_invariant
    if hints == "auto":
        hints = C.byref(_lib.SolutionHints(a_type, b_type if hints_b is None else hints_b, a_type if c_type is None else c_type, 0))
    return fn(c, a, b, s, gs, off, E, m, n, k, a_idx, a_rows, c_idx, c_rows, hints, epi, ws, None)


@pytest.mark.parametrize("a_type,b_type", PAIRS)
def test_refusals_and_their_codes(a_type, b_type):
    call = lambda **kw: _call(a_type=a_type, b_type=b_type, **kw)  # noqa: E731
    assert call(E=0) == SHAPE and call(E=1025) == SHAPE                             # num_experts in 1..1024
    assert call(m=1 << 20, a_idx=PTR, c_idx=PTR) == SHAPE
    assert call(n=24) == SHAPE and call(n=0) == SHAPE                                # n % 16
    assert call(k=128) == SHAPE and call(k=384) == SHAPE and call(k=0) == SHAPE
    if b_type == MX:
        assert call(n=48) == SHAPE and call(n=16) == SHAPE                           # MXFP4: n % 32
    assert call(n=48, epi=C.byref(_lib.Epilogue(None, 1, 0))) == SHAPE               # gated: n % 32
    for name in ("c", "a", "b", "s", "gs", "off"):
        assert call(**{name: None}) == SHAPE, name                                   # null required pointers; expert_offsets is one
    for name in ("c", "a", "b", "s"):
        assert call(**{name: C.c_void_p(0x1008)}) == SHAPE, name                     # not 16-byte aligned
    for name in ("gs", "off"):
        assert call(**{name: C.c_void_p(0x1002)}) == SHAPE, name                     # not 4-byte aligned
    assert call(a_idx=C.c_void_p(0x1002)) == SHAPE and call(c_idx=C.c_void_p(0x1002)) == SHAPE
    assert _form(4, 4) == 1
    assert call(ws=None) == SHAPE and call(ws=C.c_void_p(0x1010)) == SHAPE           # the byte query is not zero at m = 4 (split form)
    assert call(a_rows=3) == SHAPE and call(c_rows=3) == SHAPE                       # a null index is the identity: the rows must exist
    assert call(a_rows=(1 << 22) + 1, a_idx=PTR) == SHAPE                            # a_rows * k * 2 > 2^31
    assert call(off=None, m=0) == SHAPE                                              # expert_offsets is required, whatever m is
    assert call(m=0, c=None, a=None, b=None, s=None, gs=None, ws=None, a_rows=0, c_rows=0) == OK   # m == 0: nothing to do
    assert call(hints=None) == BAD
    assert call(c_type=FP16 if a_type == BF16 else BF16) == BAD
    assert call(hints_b=MX if b_type == NV else NV) == BAD                           # the hints name the other format
    for act in (3, -1, 77):
        assert call(epi=C.byref(_lib.Epilogue(None, act, 0))) == BAD
    assert call(epi=C.byref(_lib.Epilogue(None, 0, 1))) == BAD                       # reserved
    assert call(epi=C.byref(_lib.Epilogue(0x1004, 0, 0))) == SHAPE                   # a bias that is not 8-byte aligned


def test_bad_types_and_fp16_mxfp4():
    for a_type in (NV, _lib.PETIT_DTYPE_FP32, 0, 77):
        assert _call(a_type=a_type) == BAD
    assert _call(a_type=FP16, b_type=MX) == KERNEL
    assert L.petit_gemm_moe_invariant_workspace_bytes(4, 4, 32, 256, FP16, MX) == 0
    host = lambda *tail: L.petit_gemm_fp4_moe_invariant_host(PTR, PTR, PTR, PTR, PTR, None, PTR, *tail)  # noqa: E731
    assert host(4, 4, 32, 256, None, 4, None, 4, FP16, MX) == KERNEL
    assert host(4, 4, 32, 128, None, 4, None, 4, BF16, NV) == SHAPE
    assert host(0, 4, 32, 256, None, 4, None, 4, BF16, NV) == SHAPE
    assert host(4, 4, 32, 256, None, 3, None, 4, BF16, NV) == SHAPE
    assert host(4, 4, 32, 256, None, 4, None, 4, 0, NV) == BAD


def _form(m, E):
    return L.petit_gemm_moe_invariant_form(m, E)


def test_form_is_monotone_on_both_constants():
    """split (1) iff ceil(m / min(E, m)) <= R and m <= M: for every E the split m form one interval from 1, whose end does not shrink as E
    grows (more experts: fewer rows each), and never passes M."""
    ends = []
    for E in (1, 2, 3, 8, 64, 65, 130, 256, 1024):
        forms = [_form(m, E) for m in range(1, 4200)]
        assert forms[0] == 1 and set(forms) <= {0, 1}
        end = forms.index(0)                                                          # forms[i] is m = i + 1: `end` is the last split-form m
        assert all(f == 1 for f in forms[:end]) and all(f == 0 for f in forms[end:]), E
        ends.append(end)
        for m in (1 << 12, 1 << 16, (1 << 20) - 1):
            assert _form(m, E) == 0
    assert ends == sorted(ends)
    R, M = ends[0], ends[-1]                                                          # E = 1: rows per expert = m; E = 1024: the cap on m
    assert (R, M) == (8, 8)                                                           # the library's constants (profiles/moe_invariant.md)
    for E, end in zip((1, 2, 3, 8, 64, 65, 130, 256, 1024), ends):
        assert end == min(R * E, M), (E, end)


@pytest.mark.parametrize("a_type,b_type", PAIRS)
@pytest.mark.parametrize("n,k", [(32, 256), (224, 768), (32, 4352), (4096, 2048)])
def test_workspace_is_the_split_forms_slabs(n, k, a_type, b_type):
    S, _ = _geometry(n, k, a_type, b_type)
    for E in (1, 3, 65, 130, 1024):
        for m in (1, 3, 8, 9, 15, 17, 32, 33, 96, 97, 2048, 2049, 4096, (1 << 20) - 1):
            ws = L.petit_gemm_moe_invariant_workspace_bytes(E, m, n, k, a_type, b_type)
            assert ws == ((S * m * n * 4 + 255) // 256 * 256 if _form(m, E) else 0), (E, m)
        assert L.petit_gemm_moe_invariant_workspace_bytes(E, 0, n, k, a_type, b_type) == 0
        assert L.petit_gemm_moe_invariant_workspace_bytes(E, 1, n, k + 128, a_type, b_type) == 0
        assert L.petit_gemm_moe_invariant_workspace_bytes(E, 1, n + 8, k, a_type, b_type) == 0
    assert L.petit_gemm_moe_invariant_workspace_bytes(0, 1, n, k, a_type, b_type) == 0
    assert L.petit_gemm_moe_invariant_workspace_bytes(1025, 1, n, k, a_type, b_type) == 0


# --- the CPU twin ------------------------------------------------------------------------------------------------------------------------

def row_ownership(offsets, m):
    """owner[r] = the expert whose clamped range holds grouped row r, or -1: each offset clamped into [its predecessor, m] (a running maximum)."""
    hi = np.minimum(np.maximum.accumulate(np.clip(np.asarray(offsets, dtype=np.int64), 0, None)), m)
    owner = np.searchsorted(hi[1:], np.arange(m), side="right")
    return np.where((np.arange(m) >= hi[0]) & (owner < len(hi) - 1), owner, -1)


def _experts(b_type, E, n, k, seed):
    rng = np.random.default_rng([seed, b_type, n, k])
    mx = b_type == MX
    group = 32 if mx else 16
    code = rng.integers(0, 16, (E * n, k), dtype=np.uint8)
    sbyte = rng.integers(125, 130, (E * n, k // group)).astype(np.uint8) if mx else rng.integers(0x28, 0x48, (E * n, k // group)).astype(np.uint8)
    q = torch.from_numpy((code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8)).view(torch.int32)
    b = offline.repack_nvfp4_cpu(q, E * n, k)
    s = offline.process_mxfp4_scales_cpu(torch.from_numpy(sbyte), E * n, k) if mx else \
        offline.process_nvfp4_scales_cpu(torch.from_numpy(sbyte).view(torch.float8_e4m3fn), E * n, k)
    return b.contiguous(), s.contiguous()


OFFSETS = {
    "well formed": [0, 3, 3, 7, 9],
    "rows before the first and after the last": [2, 4, 6, 6, 8],
    "descending": [0, 5, 2, 7, 9],
    "negative": [-4, 3, -1, 6, 9],
    "beyond m": [0, 4, 100, 3, 50],
}


@pytest.mark.parametrize("name", list(OFFSETS))
@pytest.mark.parametrize("a_type,b_type", PAIRS)
def test_host_twin_equals_the_dense_twin_per_owned_row(a_type, b_type, name):
    """Every owned row equals petit_gemm_fp4_invariant_host(m = 1) on its A row and its owner's tensors; poisoned rows of no expert, and
    rows no index names, stay untouched; an A index out of range reads zeros, a C index out of range stores nothing."""
    E, m, n, k = 4, 9, 32, 512
    offsets = np.array(OFFSETS[name], dtype=np.int32)
    bf16 = a_type == BF16
    dt = torch.bfloat16 if bf16 else torch.float16
    b, s = _experts(b_type, E, n, k, 5)
    g = torch.Generator().manual_seed(17)
    a_rows, c_rows = 6, m + 2
    a = torch.randn(a_rows, k, generator=g).to(dt)
    bias = torch.randn(E, n, generator=g).to(dt)
    gs = (torch.rand(E, generator=g) * 0.05 + 0.01).float()
    a_idx = np.array([3, 0, 5, -1, 2, 6, 1, 4, 0], dtype=np.int32)                    # -1 and 6: outside [0, a_rows)
    c_idx = np.array([8, 7, 6, 5, 11, 3, 2, -2, 0], dtype=np.int32)                   # 11 and -2: outside [0, c_rows)
    out = np.full((c_rows, n), 0x7FC1, dtype=np.int16)
    a_bits, bias_bits = a.view(torch.int16).numpy(), bias.view(torch.int16).numpy()
    rc = L.petit_gemm_fp4_moe_invariant_host(out.ctypes.data, a_bits.ctypes.data, b.data_ptr(), s.data_ptr(), gs.data_ptr(), bias_bits.ctypes.data,
                                             offsets.ctypes.data, E, m, n, k, a_idx.ctypes.data, a_rows, c_idx.ctypes.data, c_rows, a_type, b_type)
    assert rc == OK
    owner = row_ownership(offsets, m)
    assert (owner >= 0).any()
    want = np.full((c_rows, n), 0x7FC1, dtype=np.int16)
    w_bytes, s_bytes = n * k // 2, n * k // (32 if b_type == MX else 16)
    zero = np.zeros(k, dtype=np.int16)
    for r in range(m):
        e = int(owner[r])
        if e < 0 or not 0 <= c_idx[r] < c_rows:
            continue
        row = np.ascontiguousarray(a_bits[a_idx[r]]) if 0 <= a_idx[r] < a_rows else zero
        one = np.zeros(n, dtype=np.int16)
        rc = L.petit_gemm_fp4_invariant_host(one.ctypes.data, row.ctypes.data, b.data_ptr() + e * w_bytes, s.data_ptr() + e * s_bytes,
                                             C.c_void_p(gs.data_ptr() + 4 * e), bias_bits[e].ctypes.data, 1, n, k, a_type, b_type)
        assert rc == OK
        want[c_idx[r]] = one
    assert np.array_equal(out, want), name
    # the identity on both sides, no bias
    out2 = np.full((m, n), 0x7FC1, dtype=np.int16)
    a9 = torch.randn(m, k, generator=g).to(dt).view(torch.int16).numpy()
    rc = L.petit_gemm_fp4_moe_invariant_host(out2.ctypes.data, a9.ctypes.data, b.data_ptr(), s.data_ptr(), gs.data_ptr(), None, offsets.ctypes.data,
                                             E, m, n, k, None, m, None, m, a_type, b_type)
    assert rc == OK
    assert np.array_equal((out2 == 0x7FC1).all(axis=1), owner < 0) and not (out2[owner >= 0] == 0x7FC1).all(axis=1).any()


def test_host_twin_reads_e8m0_byte_0_as_the_kernels_do():
    """The MoE twin inherits the dense twin's decode: expert 1 of 2 has every weight +6 under e8m0 byte 0 (2^-127, not 0.0), expert 0 -6 under
    byte 127; the one A row holds 2^120 once.  Expert 0's row is -6 * 2^120, expert 1's rows 6 * 2^-127 * 2^120 * gs[1] = 1.5 * 2^-4, and the
    grouped row whose A index is out of range is 0."""
    E, m, n, k = 2, 3, 32, 256
    q = torch.full((E * n, k // 2), 0xFF, dtype=torch.uint8)
    q[n:] = 0x77
    sbyte = np.full((E * n, k // 32), 127, dtype=np.uint8)
    sbyte[n:] = 0
    b = offline.repack_nvfp4_cpu(q.view(torch.int32), E * n, k).contiguous()
    s = offline.process_mxfp4_scales_cpu(torch.from_numpy(sbyte), E * n, k).contiguous()
    a = torch.zeros(1, k, dtype=torch.bfloat16)
    a[0, 77] = 2.0 ** 120
    a_bits = a.view(torch.int16).numpy()
    gs = torch.tensor([1.0, 2.0])
    offsets, a_idx = np.array([0, 1, 3], dtype=np.int32), np.array([0, 0, 5], dtype=np.int32)
    out = np.full((m, n), 0x7FC1, dtype=np.int16)
    rc = L.petit_gemm_fp4_moe_invariant_host(out.ctypes.data, a_bits.ctypes.data, b.data_ptr(), s.data_ptr(), gs.data_ptr(), None, offsets.ctypes.data,
                                             E, m, n, k, a_idx.ctypes.data, 1, None, m, BF16, MX)
    assert rc == OK
    got = torch.from_numpy(out).view(torch.bfloat16).double().numpy()
    assert np.array_equal(got, np.repeat(np.array([[-6.0 * 2.0 ** 120], [1.5 * 2.0 ** -4], [0.0]]), n, axis=1))


# --- the operator layers -----------------------------------------------------------------------------------------------------------------

NAMES = ("mul_nvfp4_a16_moe_invariant", "mul_mxfp4_a16_moe_invariant", "moe_invariant_form", "moe_invariant_workspace_bytes")
ARGS = ["A", "B", "s", "global_scales", "expert_offsets", "size_m", "size_n", "size_k", "num_experts", "a_row_index", "c_row_index", "c_rows",
        "bias", "activation", "out"]


def test_both_operator_layers_export_identical_signatures():
    import petit_kernel
    from petit_kernel import compiled, ops
    for name in NAMES:
        assert name in petit_kernel.__all__ and callable(getattr(petit_kernel, name))
        sigs = [inspect.signature(getattr(mod, name)) for mod in (ops, compiled, petit_kernel)]
        rows = [[(p.name, p.default, p.kind) for p in sig.parameters.values()] for sig in sigs]
        assert rows[0] == rows[1], name
        assert [r[0].lower() for r in rows[0]] == [r[0].lower() for r in rows[2]], name
        assert [r[1:] for r in rows[0]] == [r[1:] for r in rows[2]], name
    for name in NAMES[:2]:
        assert list(inspect.signature(getattr(ops, name)).parameters) == ARGS                # no solution_id
    for fn in (petit_kernel.fp4_moe_fused, petit_kernel.fp4_moe_routed):
        assert inspect.signature(fn).parameters["invariant"].default is False


def test_python_queries_agree_with_the_c_abi():
    from petit_kernel import ops
    for E in (1, 8, 130):
        for m in (1, 17, 300, 4096):
            assert ops.moe_invariant_form(m, E) == _form(m, E)
            assert ops.moe_invariant_workspace_bytes(E, m, 224, 768, torch.bfloat16, "mxfp4") == \
                L.petit_gemm_moe_invariant_workspace_bytes(E, m, 224, 768, BF16, MX)
            assert ops.moe_invariant_workspace_bytes(E, m, 208, 768, torch.float16) == L.petit_gemm_moe_invariant_workspace_bytes(E, m, 208, 768, FP16, NV)


def _cpu_operands(kind, dtype, E=3, m=4, n=32, k=256):
    group = 16 if kind == "nv" else 32
    return dict(A=torch.zeros(m, k, dtype=dtype), B=torch.zeros(E * n // 16, 2 * k, dtype=torch.int32),
                s=torch.zeros(E * n * k // group, dtype=torch.uint8), global_scales=torch.ones(E), expert_offsets=torch.zeros(E + 1, dtype=torch.int32),
                size_m=m, size_n=n, size_k=k, num_experts=E)


BROKEN = [
    ("dtype", lambda o: o.update(A=o["A"].float()), "A must be bfloat16 or float16."),
    ("experts", lambda o: o.update(num_experts=0), "num_experts must be in 1..1024, got 0"),
    ("k", lambda o: o.update(size_k=128), "Incompatible problem shape (m=4, n=32, k=128)"),
    ("n", lambda o: o.update(size_n=24), "Incompatible problem shape (m=4, n=24, k=256)"),
    ("activation", lambda o: o.update(activation="relu"), "activation must be one of"),
    ("A shape", lambda o: o.update(A=o["A"].reshape(-1)[:1000]), "A must be a contiguous [a_rows, size_k] tensor"),
    ("B size", lambda o: o.update(B=o["B"][:1]), "B does not hold num_experts * size_n * size_k packed 4-bit weights"),
    ("s size", lambda o: o.update(s=o["s"][:7]), "s does not hold num_experts * size_n * size_k /"),
    ("gs", lambda o: o.update(global_scales=torch.ones(2)), "global_scales must be a contiguous float32 [num_experts] tensor"),
    ("offsets", lambda o: o.update(expert_offsets=torch.zeros(4, dtype=torch.int64)), "expert_offsets must be a contiguous int32 [num_experts + 1] tensor"),
    ("index", lambda o: o.update(a_row_index=torch.zeros(3, dtype=torch.int32)), "row indices must be contiguous int32 [size_m] tensors on A's device"),
    ("out", lambda o: o.update(out=torch.zeros(4, 16, dtype=o["A"].dtype)), "out must be a contiguous [c_rows, n_out] tensor of A's dtype on A's device"),
    ("c_rows", lambda o: o.update(out=torch.zeros(4, 32, dtype=o["A"].dtype), c_rows=5), "c_rows does not match out.size(0)"),
    ("identity rows", lambda o: o.update(c_rows=3), "without a row index the matrix must hold size_m rows"),
    ("bias", lambda o: o.update(bias=torch.zeros(32, dtype=o["A"].dtype)), "bias must be a contiguous [num_experts, size_n] tensor of A's dtype on A's device"),
    ("device", lambda o: None, "all tensors must be on GPU"),
]


@pytest.mark.parametrize("kind", ["nv", "mx"])
@pytest.mark.parametrize("case", BROKEN, ids=[b[0] for b in BROKEN])
def test_both_layers_raise_the_same_texts(kind, case):
    """The argument checks are stated once (ops._check_invariant) and run by both layers in front of anything that needs a device."""
    from petit_kernel import compiled, ops
    _, breakage, text = case
    messages = []
    for layer in (ops, compiled):
        o = _cpu_operands(kind, torch.bfloat16)
        breakage(o)
        with pytest.raises(RuntimeError) as e:
            getattr(layer, f"mul_{kind}fp4_a16_moe_invariant")(**o)
        messages.append(str(e.value))
    assert messages[0] == messages[1] and text in messages[0], messages
    for layer in (ops, compiled):                                                        # the gated forms' shape rule
        o = _cpu_operands("nv", torch.bfloat16, n=48)
        with pytest.raises(RuntimeError, match="silu_mul needs size_n % 32 == 0"):
            layer.mul_nvfp4_a16_moe_invariant(**o, activation="silu_mul")
    if kind == "mx":
        for layer in (ops, compiled):
            with pytest.raises(RuntimeError, match="float16 activations with MXFP4 weights have no batch-invariant kernel"):
                layer.mul_mxfp4_a16_moe_invariant(**_cpu_operands("mx", torch.float16))
            with pytest.raises(RuntimeError, match="Incompatible problem shape"):
                layer.mul_mxfp4_a16_moe_invariant(**_cpu_operands("mx", torch.bfloat16, n=48))   # MXFP4: n % 32


def test_layer_switch_refuses_what_has_no_invariant_kernel():
    import petit_kernel
    h = torch.zeros(2, 256, dtype=torch.float16)
    z = torch.zeros(1)
    with pytest.raises(RuntimeError, match="native class .* has no batch-invariant kernel"):
        petit_kernel.fp4_moe_routed(h.bfloat16(), z, z, z, z, z, z, z, 2, "mxfp4", path="native", invariant=True)
    with pytest.raises(RuntimeError, match="float16 activations with MXFP4 weights have no batch-invariant kernel"):
        petit_kernel.fp4_moe_routed(h, z, z, z, z, z, z, z, 2, "mxfp4", invariant=True)
    with pytest.raises(RuntimeError, match="float16 activations with MXFP4 weights have no batch-invariant kernel"):
        petit_kernel.fp4_moe_fused(h, z, z, z, z, z, z, z, z, "mxfp4", invariant=True)

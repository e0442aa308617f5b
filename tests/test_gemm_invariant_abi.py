"""The batch-invariant GEMM (include/petit_amd.h "Batch-invariant GEMM") without a GPU: the symbols, the geometry (S slices of L along K,
functions of (n, k, types) alone), the slab / workspace arithmetic, every refusal with its code (all of them precede any launch: none of
these calls has a device), the CPU twin on exact-integer inputs and on a row alone and in a batch, and the two operator layers' texts."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from petit_kernel import _lib, offline

FP16, BF16 = _lib.CXX_DTYPE_FP16, _lib.CXX_DTYPE_BF16
NV, MX = _lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_MXFP4_E2M1
OK, SHAPE, KERNEL, BAD = _lib.PETIT_OK, _lib.PETIT_ERROR_PROBLEM_SHAPE, _lib.PETIT_ERROR_KERNEL_SHAPE, _lib.PETIT_ERROR_BAD_ARGUMENT
SYMBOLS = ("petit_gemm_invariant_geometry", "petit_gemm_invariant_slabs", "petit_gemm_invariant_workspace_bytes",
           "petit_gemm_fp4_fp16_invariant", "petit_gemm_mxfp4_fp16_invariant", "petit_gemm_fp4_invariant_host")
PAIRS = [(BF16, NV), (BF16, MX), (FP16, NV)]
SHAPES = [(16, 256), (48, 512), (208, 768), (16, 4352), (8192, 8192), (10240, 8192), (57344, 8192), (8192, 28672)]
L = _lib.lib
PTR = C.c_void_p(0x1000)   # a non-null, 256-byte aligned pointer for calls that are refused before anything reads it
FP4 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0])


def test_symbols_exist():
    raw = C.CDLL(str(_lib.LIB_PATH))
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTED_SYMBOLS


def _geometry(n, k, a_type=BF16, b_type=NV):
    S, Lk = C.c_uint(0), C.c_uint(0)
    L.petit_gemm_invariant_geometry(n, k, a_type, b_type, C.byref(S), C.byref(Lk))
    return S.value, Lk.value


def _call(a_type=BF16, b_type=NV, m=4, n=32, k=256, c=PTR, a=PTR, b=PTR, s=PTR, gs=PTR, hints="auto", epi=None, ws=PTR, c_type=None,
          hints_b=None):
    fn = L.petit_gemm_mxfp4_fp16_invariant if b_type == MX else L.petit_gemm_fp4_fp16_invariant
    if hints == "auto":
        hints = C.byref(_lib.SolutionHints(a_type, b_type if hints_b is None else hints_b, a_type if c_type is None else c_type, 0))
    return fn(c, a, b, s, gs, m, n, k, hints, epi, ws, None)


@pytest.mark.parametrize("a_type,b_type", PAIRS)
def test_refusals_and_their_codes(a_type, b_type):
    call = lambda **kw: _call(a_type=a_type, b_type=b_type, **kw)  # noqa: E731
    assert call(n=24) == SHAPE and call(n=0) == SHAPE                        # n % 16
    assert call(k=128) == SHAPE and call(k=384) == SHAPE and call(k=0) == SHAPE   # k % 256: the packed scale layout has nothing else
    assert call(m=1 << 20) == SHAPE
    if b_type == MX:
        assert call(n=48) == SHAPE and call(n=16) == SHAPE                    # MXFP4: n % 32 (its scale tensor comes in rows of 32)
    for name in ("c", "a", "b", "s"):
        assert call(**{name: None}) == SHAPE, name                            # null required pointers
        assert call(**{name: C.c_void_p(0x1008)}) == SHAPE, name              # not 16-byte aligned
    assert call(ws=None) == SHAPE and call(ws=C.c_void_p(0x1010)) == SHAPE    # the byte query is not zero at m = 4
    assert call(gs=None, m=0, c=None, a=None, b=None, s=None, ws=None) == OK  # m == 0: nothing to do
    assert call(hints=None) == BAD
    assert call(c_type=FP16 if a_type == BF16 else BF16) == BAD
    assert call(hints_b=MX if b_type == NV else NV) == BAD                    # the hints name the other format
    for act in (3, -1, 77):
        assert call(epi=C.byref(_lib.Epilogue(None, act, 0))) == BAD
    assert call(epi=C.byref(_lib.Epilogue(None, 0, 1))) == BAD                # reserved
    assert call(n=48, epi=C.byref(_lib.Epilogue(None, 1, 0))) == SHAPE        # gated: n % 32
    assert call(epi=C.byref(_lib.Epilogue(0x1004, 0, 0))) == SHAPE            # a bias that is not 8-byte aligned


def test_bad_types_and_fp16_mxfp4():
    for a_type in (NV, _lib.PETIT_DTYPE_FP32, 0, 77):
        assert _call(a_type=a_type) == BAD
    assert _call(a_type=FP16, b_type=MX) == KERNEL
    assert _call(a_type=FP16, b_type=MX, hints_b=_lib.CXX_DTYPE_MXFP4_E2M1_F16RANGE) == KERNEL
    assert L.petit_gemm_invariant_workspace_bytes(4, 32, 256, FP16, MX) == 0
    assert L.petit_gemm_fp4_invariant_host(PTR, PTR, PTR, PTR, None, None, 4, 32, 256, FP16, MX) == KERNEL
    assert L.petit_gemm_fp4_invariant_host(PTR, PTR, PTR, PTR, None, None, 4, 32, 128, BF16, NV) == SHAPE
    assert L.petit_gemm_fp4_invariant_host(None, PTR, PTR, PTR, None, None, 4, 32, 256, BF16, NV) == SHAPE
    assert L.petit_gemm_fp4_invariant_host(PTR, PTR, PTR, PTR, None, None, 4, 32, 256, 0, NV) == BAD


@pytest.mark.parametrize("a_type,b_type", PAIRS)
@pytest.mark.parametrize("n,k", SHAPES)
def test_geometry_and_workspace(n, k, a_type, b_type):
    if b_type == MX and n % 32:                                               # MXFP4 needs n % 32 == 0: refused, no workspace
        assert L.petit_gemm_invariant_workspace_bytes(1, n, k, a_type, b_type) == 0
        return
    S, Lk = _geometry(n, k, a_type, b_type)
    assert Lk % 128 == 0 and Lk % 256 == 0 and Lk > 0
    assert S * Lk >= k > (S - 1) * Lk and 1 <= S <= 16
    split_max = _split_max(n, k, a_type, b_type)                              # the form switch: the last m with a workspace
    assert 1 <= split_max < 4096
    for m in list(range(1, 300)) + [512, 4096, (1 << 20) - 1]:
        slabs = L.petit_gemm_invariant_slabs(m, n, k, a_type, b_type)
        assert slabs == (S if m <= split_max else 1)                          # S does not move with m: two values at most
        ws = L.petit_gemm_invariant_workspace_bytes(m, n, k, a_type, b_type)
        assert ws == ((S * m * n * 4 + 255) // 256 * 256 if m <= split_max else 0), (m, slabs, ws)
    assert L.petit_gemm_invariant_slabs(1, n, k, a_type, b_type) == S
    # refused shapes need no workspace
    assert L.petit_gemm_invariant_workspace_bytes(1, n, k + 128, a_type, b_type) == 0
    assert L.petit_gemm_invariant_workspace_bytes(1, n + 8, k, a_type, b_type) == 0
    assert L.petit_gemm_invariant_workspace_bytes(1, n, k, 3, b_type) == 0
    assert L.petit_gemm_invariant_workspace_bytes(0, n, k, a_type, b_type) == 0


def _split_max(n, k, a_type, b_type):
    m = 1
    while L.petit_gemm_invariant_workspace_bytes(m + 1, n, k, a_type, b_type):
        m += 1
    return m


def test_decode_geometry_fills_the_chip():
    """At M = 1 a model shape's split form launches n-tiles x S waves: at least two per CU of a 256-CU chip."""
    for n, k in SHAPES[4:]:
        S, _ = _geometry(n, k)
        assert n // 16 * S >= 512, (n, k, S)


# --- the CPU twin ------------------------------------------------------------------------------------------------------------------------

def _bits16(v64, bf16):
    t = torch.from_numpy(v64).to(torch.bfloat16 if bf16 else torch.float16)
    assert np.array_equal(t.double().numpy(), v64)
    return t.view(torch.int16).numpy().copy()


def _host_problem(a_type, b_type, m, n, k, seed, exact=True):
    rng = np.random.default_rng([seed, a_type, b_type, n, k])
    mx, bf16 = b_type == MX, a_type == BF16
    group = 32 if mx else 16
    code = rng.integers(0, 16, (n, k), dtype=np.uint8)
    sidx = rng.integers(0, 3, (n, k // group))
    sval = np.array([1.0, 2.0, 4.0])[sidx]
    sbyte = np.array([127, 128, 129] if mx else [0x38, 0x40, 0x48], dtype=np.uint8)[sidx]
    q = torch.from_numpy((code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8)).view(torch.int32)
    b = offline.repack_nvfp4_cpu(q, n, k)
    s = offline.process_mxfp4_scales_cpu(torch.from_numpy(sbyte), n, k) if mx else \
        offline.process_nvfp4_scales_cpu(torch.from_numpy(sbyte).view(torch.float8_e4m3fn), n, k)
    w = FP4[code] * np.repeat(sval, group, axis=1)
    if exact:
        a = rng.integers(-3, 4, (m, k)) * (rng.random((m, k)) < 0.5) + 0.0
    else:
        a = torch.randn(m, k, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16 if bf16 else torch.float16).double().numpy()
    bias = rng.integers(-8, 9, n) + 0.0
    return b.contiguous(), s.contiguous(), w, a, bias


def _host(a_type, b_type, b, s, a, bias, gs, n, k):
    bf16 = a_type == BF16
    m = a.shape[0]
    a_bits = np.ascontiguousarray(_bits16(a, bf16))
    bias_bits = None if bias is None else np.ascontiguousarray(_bits16(bias, bf16))
    out = np.full((m, n), 0x7FC1, dtype=np.int16)
    gsf = None if gs is None else C.byref(C.c_float(gs))
    rc = L.petit_gemm_fp4_invariant_host(out.ctypes.data, a_bits.ctypes.data, b.data_ptr(), s.data_ptr(), gsf,
                                         None if bias_bits is None else bias_bits.ctypes.data, m, n, k, a_type, b_type)
    assert rc == OK
    return torch.from_numpy(out).view(torch.bfloat16 if bf16 else torch.float16)


@pytest.mark.parametrize("a_type,b_type", PAIRS)
@pytest.mark.parametrize("n,k", [(32, 256), (48, 512), (32, 768)])
def test_host_twin_is_exact_on_small_numbers(n, k, a_type, b_type):
    """On inputs whose partial sums are exact in any order the twin equals the float64 result rounded once (test 1 of the GPU module)."""
    if b_type == MX and n % 32:
        n = 64
    m = 5
    b, s, w, a, bias = _host_problem(a_type, b_type, m, n, k, 3)
    assert (np.abs(a) @ np.abs(w).T).max() < 2 ** 22
    for gs in (0.25, None):
        for use_bias in (True, False):
            y = a @ w.T * (1.0 if gs is None else gs) + (bias if use_bias else 0.0)
            got = _host(a_type, b_type, b, s, a, bias if use_bias else None, gs, n, k)
            want = torch.from_numpy(y).float().to(got.dtype)
            assert torch.equal(got, want), (gs, use_bias)


@pytest.mark.parametrize("a_type,b_type", PAIRS)
def test_host_twin_gives_a_row_the_same_bits_alone_and_in_a_batch(a_type, b_type):
    n, k, m = 32, 768, 6
    b, s, w, a, bias = _host_problem(a_type, b_type, m, n, k, 9, exact=False)
    full = _host(a_type, b_type, b, s, a, bias, 0.0123, n, k)
    for r in (0, 3, m - 1):
        alone = _host(a_type, b_type, b, s, a[r:r + 1], bias, 0.0123, n, k)
        assert torch.equal(alone[0].view(torch.int16), full[r].view(torch.int16)), r
    moved = np.roll(a, 2, axis=0)
    assert torch.equal(_host(a_type, b_type, b, s, moved, bias, 0.0123, n, k).view(torch.int16), torch.roll(full, 2, 0).view(torch.int16))


def test_host_twin_reads_e8m0_byte_0_as_the_kernels_do():
    """e8m0 scale byte 0 is 2^-127 (the hardware convert the kernels dequantise with; `byte << 23` would make it 0.0 and every output 0):
    every weight +6 under byte 0, one activation of +-2^120 per row -> +-6 * 2^-127 * 2^120 = +-1.5 * 2^-5 in every column; with gs = 2 and
    a bias of 1: 1 +- 3 * 2^-5.  Byte 255 in one block of one column: that column is NaN in every row, the others keep their bits."""
    n, k, m = 32, 512, 2
    q = torch.full((n, k // 2), 0x77, dtype=torch.uint8).view(torch.int32)
    b = offline.repack_nvfp4_cpu(q, n, k).contiguous()
    sbyte = np.zeros((n, k // 32), dtype=np.uint8)
    s = offline.process_mxfp4_scales_cpu(torch.from_numpy(sbyte), n, k).contiguous()
    a = np.zeros((m, k))
    a[0, 5], a[1, 300] = 2.0 ** 120, -2.0 ** 120
    sign = np.array([[1.0], [-1.0]])
    got = _host(BF16, MX, b, s, a, None, None, n, k)
    assert np.array_equal(got.double().numpy(), np.broadcast_to(sign * 1.5 * 2.0 ** -5, (m, n)))
    got = _host(BF16, MX, b, s, a, np.ones(n), 2.0, n, k)
    assert np.array_equal(got.double().numpy(), np.broadcast_to(1.0 + sign * 3.0 * 2.0 ** -5, (m, n)))
    sbyte[7, 3] = 255
    s = offline.process_mxfp4_scales_cpu(torch.from_numpy(sbyte), n, k).contiguous()
    v = _host(BF16, MX, b, s, a, np.ones(n), 2.0, n, k).double().numpy()
    assert np.isnan(v[:, 7]).all() and np.array_equal(np.delete(v, 7, axis=1), np.broadcast_to(1.0 + sign * 3.0 * 2.0 ** -5, (m, n - 1)))


# --- the operator layers -----------------------------------------------------------------------------------------------------------------

NAMES = ("mul_nvfp4_a16_invariant", "mul_mxfp4_a16_invariant", "invariant_geometry", "invariant_slabs", "invariant_workspace_bytes")


def test_both_operator_layers_export_identical_signatures():
    import petit_kernel
    from petit_kernel import compiled, ops
    for name in NAMES:
        assert name in petit_kernel.__all__ and callable(getattr(petit_kernel, name))
        sigs = [inspect.signature(getattr(mod, name)) for mod in (ops, compiled, petit_kernel)]
        rows = [[(p.name, p.default, p.kind) for p in sig.parameters.values()] for sig in sigs]
        assert rows[0] == rows[1], name
        assert [r[0].lower() for r in rows[0]] == [r[0].lower() for r in rows[2]], name   # (the front end spells a, b in lower case, as mul_nvfp4_a16)
    assert list(inspect.signature(ops.mul_nvfp4_a16_invariant).parameters) == ["A", "B", "s", "global_scale", "size_m", "size_n", "size_k",
                                                                                "bias", "activation"]


def test_python_queries_agree_with_the_c_abi():
    from petit_kernel import ops
    for (n, k) in SHAPES:
        assert ops.invariant_geometry(n, k, torch.bfloat16, "mxfp4") == _geometry(n, k, BF16, MX)
        for m in (1, 17, 4096):
            assert ops.invariant_slabs(m, n, k, torch.float16, "nv") == L.petit_gemm_invariant_slabs(m, n, k, FP16, NV)
            assert ops.invariant_workspace_bytes(m, n, k) == L.petit_gemm_invariant_workspace_bytes(m, n, k, BF16, NV)


def _cpu_operands(kind, dtype, m=4, n=32, k=256):
    group = 16 if kind == "nv" else 32
    return dict(A=torch.zeros(m, k, dtype=dtype), B=torch.zeros(n // 16, 2 * k, dtype=torch.int32),
                s=torch.zeros(n * k // group, dtype=torch.uint8), global_scale=torch.ones(1), size_m=m, size_n=n, size_k=k)


BROKEN = [
    ("dtype", lambda o: o.update(A=o["A"].float()), "A must be bfloat16 or float16."),
    ("k", lambda o: o.update(size_k=128), "Incompatible problem shape (m=4, n=32, k=128)"),
    ("n", lambda o: o.update(size_n=24), "Incompatible problem shape (m=4, n=24, k=256)"),
    ("activation", lambda o: o.update(activation="relu"), "activation must be one of"),
    ("gated n", lambda o: o.update(size_n=48, activation="silu_mul"), "silu_mul needs size_n % 32 == 0"),
    ("A shape", lambda o: o.update(A=o["A"][:3]), "A must be a contiguous [size_m, size_k] tensor"),
    ("B size", lambda o: o.update(B=o["B"][:1]), "B does not hold size_n * size_k packed 4-bit weights"),
    ("s size", lambda o: o.update(s=o["s"][:7]), "s does not hold size_n * size_k /"),
    ("gs dtype", lambda o: o.update(global_scale=torch.ones(1, dtype=torch.float64)), "global_scale must be float32"),
    ("bias", lambda o: o.update(bias=torch.zeros(31, dtype=o["A"].dtype)), "bias must be a contiguous [size_n] tensor of A's dtype on A's device"),
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
            getattr(layer, f"mul_{kind}fp4_a16_invariant")(**o)
        messages.append(str(e.value))
    assert messages[0] == messages[1] and text in messages[0], messages
    if kind == "mx":
        for layer in (ops, compiled):
            with pytest.raises(RuntimeError, match="float16 activations with MXFP4 weights have no batch-invariant kernel"):
                layer.mul_mxfp4_a16_invariant(**_cpu_operands("mx", torch.float16))

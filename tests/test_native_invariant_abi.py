"""The batch-invariant GEMM on the native class (include/petit_amd.h "Batch-invariant GEMM on the native class") without a GPU: the symbols and
their declarations, the slab / workspace arithmetic, every refusal with its code (all of them precede any launch: none of these calls has a
device), the host quantiser against the numpy statements of the three formats, the CPU twin on exact inputs (bit for bit against float64) and
on random ones (inside the header's bound), and the two operator layers' signatures and texts.  tests/test_native_invariant.py imports the
problem builders below."""
import ctypes as C
import inspect
from pathlib import Path

import numpy as np
import pytest
import torch

from petit_kernel import _lib, offline
from test_gpu_parity import decode_qact, native_exact_bound, quantize_act_mxfp4, quantize_act_mxfp6, quantize_act_mxfp8

FP16, BF16 = _lib.CXX_DTYPE_FP16, _lib.CXX_DTYPE_BF16
NV, MX = _lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_MXFP4_E2M1
OK, SHAPE, KERNEL, BAD = _lib.PETIT_OK, _lib.PETIT_ERROR_PROBLEM_SHAPE, _lib.PETIT_ERROR_KERNEL_SHAPE, _lib.PETIT_ERROR_BAD_ARGUMENT
SYMBOLS = ("petit_gemm_native_invariant_slabs", "petit_gemm_native_invariant_workspace_bytes", "petit_gemm_mxfp4_native_invariant",
           "petit_quantize_activations_host", "petit_gemm_native_invariant_host")
FMTS = {"mxfp8": 8, "mxfp6": 6, "mxfp4": 4}
QUANT = {"mxfp8": quantize_act_mxfp8, "mxfp6": quantize_act_mxfp6, "mxfp4": quantize_act_mxfp4}
SHAPES = [(64, 1024), (4096, 2304), (128, 256), (8192, 8192), (57344, 8192), (8192, 28672)]
SPLIT_MAX_M = 64
L = _lib.lib
PTR = C.c_void_p(0x1000)   # a non-null, 256-byte aligned pointer for calls that are refused before anything reads it
FP4 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0])
ROOT = Path(__file__).resolve().parent.parent


# --- problem builders (shared with the GPU module) -------------------------------------------------------------------------------------------

def dt(is_bf16):
    return torch.bfloat16 if is_bf16 else torch.float16


def to16(v64: np.ndarray, is_bf16: bool, exact=True) -> np.ndarray:
    """float64 values -> the uint16 patterns of the 16-bit type (exact: the values must be representable)."""
    t = torch.from_numpy(np.ascontiguousarray(v64)).to(dt(is_bf16))
    if exact:
        assert np.array_equal(t.double().numpy(), v64)
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def from16(b: np.ndarray, is_bf16: bool) -> np.ndarray:
    return torch.from_numpy(b.view(np.int16).copy()).view(dt(is_bf16)).double().numpy()


def pack_weights(code: np.ndarray, sbyte: np.ndarray):
    """e2m1 codes [n, k] and e8m0 bytes [n, k / 32] -> (packed b, packed s) CPU tensors, and the dequantised float64 weights."""
    n, k = code.shape
    q = torch.from_numpy((code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8)).view(torch.int32)
    b = offline.repack_nvfp4_cpu(q, n, k).contiguous()
    s = offline.process_mxfp4_scales_cpu(torch.from_numpy(sbyte.astype(np.uint8)), n, k).contiguous()
    w = FP4[code] * np.repeat(np.ldexp(1.0, sbyte.astype(np.int64) - 127), 32, axis=1)
    return b, s, w


def exact_weights(n, k, seed):
    rng = np.random.default_rng([seed, n, k])
    return pack_weights(rng.integers(0, 16, (n, k), dtype=np.uint8), rng.integers(126, 129, (n, k // 32)))


def random_weights(n, k, seed):
    """checkpoint-like: every code, block scales over a band of 17 binades"""
    rng = np.random.default_rng([seed, n, k, 1])
    return pack_weights(rng.integers(0, 16, (n, k), dtype=np.uint8), rng.integers(119, 136, (n, k // 32)))


def exact_activations(m, k, seed):
    """Activations every format's quantiser keeps exactly, with exact partial sums against exact_weights: per 32-k block small integers out of
    {0, 1, 2, 3, 4, 6} with a 4 or a 6 among them (the block maximum then lands on the formats' top binade: e2m1, e2m3 and e4m3 hold
    v, v, 32 v exactly) or an all-zero block, signs at random, times one power of two per block."""
    rng = np.random.default_rng([seed, m, k, 2])
    v = np.array([0.0, 1, 2, 3, 4, 6])[rng.integers(0, 6, (m, k // 32, 32))] * (rng.random((m, k // 32, 32)) < 0.6)
    v[:, :, 0] = np.array([4.0, 6.0])[rng.integers(0, 2, (m, k // 32))]
    v *= rng.choice([-1.0, 1.0], v.shape)
    v[rng.random((m, k // 32)) < 0.1] = 0.0                                  # zero blocks
    v *= np.ldexp(1.0, rng.integers(-1, 2, (m, k // 32)))[:, :, None]
    return v.reshape(m, k)


def host_quantize(a_bits: np.ndarray, is_bf16: bool, fmt: str) -> np.ndarray:
    m, k = a_bits.shape
    nbytes = int(L.petit_quantized_activation_bytes(m, k, FMTS[fmt]))
    qa = np.full(nbytes + 64, 0xA5, dtype=np.uint8)
    a = np.ascontiguousarray(a_bits)
    assert L.petit_quantize_activations_host(qa.ctypes.data, a.ctypes.data, m, k, BF16 if is_bf16 else FP16, FMTS[fmt]) == OK
    assert (qa[nbytes:] == 0xA5).all()
    return qa[:nbytes].copy()


def twin(qa: np.ndarray, b, s, gs, bias_bits, m, n, k, is_bf16, fmt) -> np.ndarray:
    """petit_gemm_native_invariant_host on host bytes -> the uint16 patterns of c [m, n]"""
    out = np.full((m, n), 0x7FC1, dtype=np.uint16)
    gsf = None if gs is None else C.byref(C.c_float(gs))
    bias_bits = None if bias_bits is None else np.ascontiguousarray(bias_bits)
    rc = L.petit_gemm_native_invariant_host(out.ctypes.data, qa.ctypes.data, b.data_ptr(), s.data_ptr(), gsf,
                                            None if bias_bits is None else bias_bits.ctypes.data, m, n, k, BF16 if is_bf16 else FP16, FMTS[fmt])
    assert rc == OK
    return out


def expect_plain(fold32: np.ndarray, gs, bias64, is_bf16) -> np.ndarray:
    """The plain epilogue of the definition on an fp32 fold: a multiply, then an add, each rounded, then one rounding to 16 bit."""
    y = fold32.astype(np.float32)
    if gs is not None:
        y = (y * np.float32(gs)).astype(np.float32)
    if bias64 is not None:
        y = (y + bias64.astype(np.float32)[None, :]).astype(np.float32)
    return to16(y.astype(np.float64), is_bf16, exact=False)


def geometry(n, k, a_type=BF16):
    S, Lk = C.c_uint(0), C.c_uint(0)
    L.petit_gemm_invariant_geometry(n, k, a_type, MX, C.byref(S), C.byref(Lk))
    return S.value, Lk.value


def header_bound(a_q, w, gs, bias64, fmt, is_bf16, y_abs):
    """The header's accuracy statement: the class's derived bound (its 16 T term covers the S - 1 <= 15 slab additions and the multiply), one
    more fp32 rounding for a bias, and one 16-bit rounding of the result."""
    g = 1.0 if gs is None else abs(gs)
    bound = native_exact_bound(a_q.astype(np.float32), w.astype(np.float32), g, fmt)
    if bias64 is not None:
        bound = bound + 2.0 ** -24 * (y_abs + np.abs(bias64)[None, :])
    return bound + (2.0 ** -8 if is_bf16 else 2.0 ** -11) * y_abs + (0.0 if is_bf16 else 2.0 ** -25)   # (fp16: half a subnormal step)


# --- the ABI ---------------------------------------------------------------------------------------------------------------------------------

def test_symbols_exist_and_are_declared():
    raw = C.CDLL(str(_lib.LIB_PATH))
    header = (ROOT / "include" / "petit_amd.h").read_text()
    assert "Batch-invariant GEMM on the native class" in header
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert f" {name}(" in header, name


@pytest.mark.parametrize("a_type", [BF16, FP16])
@pytest.mark.parametrize("n,k", SHAPES)
def test_slabs_and_workspace_are_the_stated_arithmetic(n, k, a_type):
    S, Lk = geometry(n, k, a_type)
    assert 1 <= S <= 16 and Lk % 256 == 0 and S * Lk >= k > (S - 1) * Lk
    r256 = lambda x: (x + 255) // 256 * 256  # noqa: E731
    for m in list(range(1, 70)) + [200, 512, 4096, 65535]:
        split = m <= SPLIT_MAX_M
        assert L.petit_gemm_native_invariant_slabs(m, n, k, a_type) == (S if split else 1)
        slab = r256(S * m * n * 4) if split else 0
        for fmt in (8, 6, 4):
            qbytes = m * (k // 8 * fmt) + m * (k // 32)
            assert qbytes == L.petit_quantized_activation_bytes(m, k, fmt)
            assert L.petit_gemm_native_invariant_workspace_bytes(m, n, k, a_type, fmt, 0) == r256(qbytes) + slab, (m, fmt)
            assert L.petit_gemm_native_invariant_workspace_bytes(m, n, k, a_type, fmt, 1) == slab, (m, fmt)
    assert L.petit_gemm_native_invariant_workspace_bytes(4096, n, k, a_type, 8, 1) == 0          # the whole form on quantised bytes: none
    # refused calls need no workspace
    for args in ((1, n, k + 128, a_type, 8, 0), (1, n + 16, k, a_type, 8, 0), (1, n, k, 3, 8, 0), (0, n, k, a_type, 8, 0), (1, n, k, a_type, 5, 0),
                 (1 << 20, n, k, a_type, 8, 1), (65536, n, k, a_type, 8, 0)):
        assert L.petit_gemm_native_invariant_workspace_bytes(*args) == 0, args
    assert L.petit_gemm_native_invariant_workspace_bytes(65536, n, k, a_type, 8, 1) == 0          # (quantised, whole form: nothing needed)


def test_shapes_of_the_gpu_module():
    assert geometry(64, 1024) == (4, 256) and geometry(4096, 2304) == (5, 512) and geometry(128, 256) == (1, 256)
    assert geometry(4096, 2304, FP16) == (5, 512)


def _call(a_type=BF16, m=4, n=64, k=256, fmt=8, quantized=0, c=PTR, a=PTR, b=PTR, s=PTR, gs=PTR, hints="auto", epi=None, ws=PTR, c_type=None,
          b_type=MX):
    if hints == "auto":
        hints = C.byref(_lib.SolutionHints(a_type, b_type, a_type if c_type is None else c_type, 0))
    return L.petit_gemm_mxfp4_native_invariant(c, a, b, s, gs, m, n, k, hints, fmt, quantized, epi, ws, None)


@pytest.mark.parametrize("quantized", [0, 1])
@pytest.mark.parametrize("a_type", [BF16, FP16])
def test_refusals_and_their_codes(a_type, quantized):
    """Non-null dummy pointers throughout: a call that got as far as a launch would fault here, so every code comes from before any launch."""
    call = lambda **kw: _call(a_type=a_type, quantized=quantized, **kw)  # noqa: E731
    assert call(n=48) == SHAPE and call(n=16) == SHAPE and call(n=0) == SHAPE          # n % 32
    assert call(k=128) == SHAPE and call(k=384) == SHAPE and call(k=0) == SHAPE        # k % 256
    assert call(m=1 << 20) == SHAPE
    for name in ("c", "a", "b", "s"):
        assert call(**{name: None}) == SHAPE, name                                    # null required pointers
        assert call(**{name: C.c_void_p(0x1008)}) == SHAPE, name                      # not 16-byte aligned
    assert call(ws=None) == SHAPE and call(ws=C.c_void_p(0x1010)) == SHAPE            # the byte query is not zero at m = 4
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
    if not quantized:
        assert call(m=65536) == KERNEL                                                # 16-bit input: the quantiser's row limit, before any launch


def test_bad_types_and_the_host_entries():
    for a_type in (NV, _lib.PETIT_DTYPE_FP32, 0, 77):
        assert _call(a_type=a_type) == BAD
    host = L.petit_gemm_native_invariant_host
    assert host(PTR, PTR, PTR, PTR, None, None, 4, 64, 128, BF16, 8) == SHAPE
    assert host(PTR, PTR, PTR, PTR, None, None, 4, 48, 256, BF16, 8) == SHAPE
    assert host(None, PTR, PTR, PTR, None, None, 4, 64, 256, BF16, 8) == SHAPE
    assert host(PTR, PTR, PTR, PTR, None, None, 4, 64, 256, 0, 8) == BAD
    assert host(PTR, PTR, PTR, PTR, None, None, 4, 64, 256, FP16, 5) == BAD
    assert host(None, None, None, None, None, None, 0, 64, 256, FP16, 6) == OK
    q = L.petit_quantize_activations_host
    assert q(PTR, PTR, 4, 1000, BF16, 4) == SHAPE and q(PTR, PTR, 4, 1024, 3, 4) == KERNEL and q(None, PTR, 4, 1024, BF16, 4) == BAD
    assert q(PTR, PTR, 4, 1024, BF16, 5) == BAD and q(PTR, C.c_void_p(0x1008), 4, 1024, BF16, 4) == BAD and q(None, None, 0, 1024, BF16, 4) == OK


# --- the host quantiser ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("fmt", list(FMTS))
def test_host_quantiser_is_the_numpy_statement(fmt, is_bf16):
    """Random rows, zero blocks, -0.0, 16-bit subnormals, block maxima at both ends of the type's exponent range and around the formats'
    saturation points: the decoded bytes equal the numpy quantiser of tests/test_gpu_parity.py, element for element."""
    rng = np.random.default_rng(7)
    m, k = 9, 1024
    blocks = rng.standard_normal((m, k // 32, 32))
    blocks[0, 0] = 0.0
    blocks[0, 1] = -0.0
    blocks[1, 0] = (2.0 ** -133 if is_bf16 else 2.0 ** -24) * rng.integers(0, 8, 32)            # subnormals of the 16-bit type
    blocks[1, 1] = rng.standard_normal(32) * (2.0 ** 120 if is_bf16 else 2.0 ** 13)              # the top of the exponent range
    blocks[1, 2] = rng.standard_normal(32) * (2.0 ** -120 if is_bf16 else 2.0 ** -12)            # the bottom of the normal range
    blocks[1, 3, :] = 0.0
    blocks[1, 3, 9] = 3.3e38 if is_bf16 else 65504.0                                             # the largest finite value alone
    top = 7.5 if fmt == "mxfp6" else 6.0 if fmt == "mxfp4" else 7.0
    for j, mx in enumerate((top * 0.999, top, top * 1.03, 7.99, 4.0, 3.999)):
        blocks[2, j] = rng.uniform(-1, 1, 32)
        blocks[2, j, 7] = mx
        blocks[3, j] = -blocks[2, j]
    bits = to16(blocks.reshape(m, k), is_bf16, exact=False)
    x = from16(bits, is_bf16).astype(np.float32)
    got = decode_qact(host_quantize(bits, is_bf16, fmt), m, k, fmt)
    want = QUANT[fmt](x)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} elements differ; first {tuple(bad[0])}: x {x[tuple(bad[0])]!r} got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}"


@pytest.mark.parametrize("fmt", list(FMTS))
def test_host_quantiser_is_a_function_of_the_row(fmt):
    """A row's decoded values and scale bytes are the same alone and in a batch (only their address in the k-tile-major image moves)."""
    rng = np.random.default_rng(11)
    bits = to16(rng.standard_normal((5, 512)), True, exact=False)
    full = decode_qact(host_quantize(bits, True, fmt), 5, 512, fmt)
    for r in (0, 2, 4):
        assert np.array_equal(decode_qact(host_quantize(bits[r:r + 1], True, fmt), 1, 512, fmt)[0], full[r])


# --- the CPU twin ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("fmt", list(FMTS))
@pytest.mark.parametrize("n,k", [(64, 1024), (4096, 2304), (128, 256)])
def test_twin_is_the_float64_result_on_exact_inputs(n, k, fmt, is_bf16):
    """Quantiser exact, every partial sum exact: the twin equals the float64 product pushed through the stated epilogue -- plain, bias, global
    scale, both; (4096, 2304) has S = 5 slices of 512 and a last slice of 256."""
    m = 3
    b, s, w = exact_weights(n, k, 3)
    a = exact_activations(m, k, 3)
    bits = to16(a, is_bf16)
    qa = host_quantize(bits, is_bf16, fmt)
    assert np.array_equal(decode_qact(qa, m, k, fmt).astype(np.float64), a)           # the quantiser is exact on these
    fold = a @ w.T
    assert (np.abs(a) @ np.abs(w).T).max() < 2 ** 22
    assert np.array_equal(fold.astype(np.float32).astype(np.float64), fold)
    bias = np.random.default_rng(5).integers(-8, 9, n) * 0.5
    for gs in (0.25, 1.0 / 3.0, None):
        for use_bias in (True, False):
            got = twin(qa, b, s, gs, to16(bias, is_bf16) if use_bias else None, m, n, k, is_bf16, fmt)
            want = expect_plain(fold.astype(np.float32), gs, bias if use_bias else None, is_bf16)
            assert np.array_equal(got, want), (gs, use_bias)


@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("fmt", list(FMTS))
def test_twin_stays_inside_the_header_bound_on_random_inputs(fmt, is_bf16):
    n, k, m = 64, 1024, 6
    b, s, w = random_weights(n, k, 21)
    rng = np.random.default_rng(22)
    bits = to16(rng.standard_normal((m, k)), is_bf16, exact=False)
    qa = host_quantize(bits, is_bf16, fmt)
    a_q = decode_qact(qa, m, k, fmt).astype(np.float64)
    gs, bias = 0.0123, rng.standard_normal(n)
    bias = from16(to16(bias, is_bf16, exact=False), is_bf16)
    got = from16(twin(qa, b, s, gs, to16(bias, is_bf16), m, n, k, is_bf16, fmt), is_bf16)
    exact = a_q @ w.T * float(np.float32(gs)) + bias[None, :]
    assert (np.abs(got - exact) <= header_bound(a_q, w, gs, bias, fmt, is_bf16, np.abs(exact))).all()
    # a row alone and in the batch: the same bits
    alone = twin(host_quantize(bits[3:4], is_bf16, fmt), b, s, gs, to16(bias, is_bf16), 1, n, k, is_bf16, fmt)
    assert np.array_equal(alone[0], to16(got, is_bf16)[3])


# --- the operator layers ---------------------------------------------------------------------------------------------------------------------

NAMES = ("mul_mxfp4_native_invariant", "native_invariant_slabs", "native_invariant_workspace_bytes")


def test_both_operator_layers_export_identical_signatures():
    import petit_kernel
    from petit_kernel import compiled, ops
    for name in NAMES:
        assert name in petit_kernel.__all__ and callable(getattr(petit_kernel, name))
        sigs = [inspect.signature(getattr(mod, name)) for mod in (ops, compiled, petit_kernel)]
        rows = [[(p.name, p.default, p.kind) for p in sig.parameters.values()] for sig in sigs]
        assert rows[0] == rows[1], name
        assert [r[0].lower() for r in rows[0]] == [r[0].lower() for r in rows[2]], name
    assert list(inspect.signature(ops.mul_mxfp4_native_invariant).parameters) == ["A", "B", "s", "global_scale", "size_m", "size_n", "size_k", "fmt",
                                                                                   "bias", "activation"]
    assert inspect.signature(ops.mul_mxfp4_native_invariant).parameters["fmt"].default == "mxfp8"


def test_python_queries_agree_with_the_c_abi():
    from petit_kernel import ops
    for (n, k) in SHAPES:
        for m in (1, 32, 33, 64, 65, 4096):
            assert ops.native_invariant_slabs(m, n, k, torch.float16) == L.petit_gemm_native_invariant_slabs(m, n, k, FP16)
            for fmt, code in FMTS.items():
                for quantized in (False, True):
                    assert ops.native_invariant_workspace_bytes(m, n, k, torch.bfloat16, fmt, quantized) == \
                        L.petit_gemm_native_invariant_workspace_bytes(m, n, k, BF16, code, int(quantized))


def _cpu_operands(dtype, m=4, n=64, k=256, quantized=None):
    from petit_kernel import ops
    A = torch.zeros(m, k, dtype=dtype)
    if quantized:
        A = ops.QuantizedActivations(torch.zeros(m * (k // 8 * FMTS[quantized]) + m * (k // 32), dtype=torch.uint8), m, k, quantized, dtype)
    return dict(A=A, B=torch.zeros(n // 16, 2 * k, dtype=torch.int32), s=torch.zeros(n * k // 32, dtype=torch.uint8),
                global_scale=torch.ones(1), size_m=m, size_n=n, size_k=k)


BROKEN = [
    ("fmt", lambda o: o.update(fmt="mxfp5"), "fmt must be 'mxfp8', 'mxfp6' or 'mxfp4'"),
    ("dtype", lambda o: o.update(A=o["A"].float()), "A must be bfloat16 or float16"),
    ("k", lambda o: o.update(size_k=128), "Incompatible problem shape (m=4, n=64, k=128)"),
    ("n", lambda o: o.update(size_n=48), "Incompatible problem shape (m=4, n=48, k=256)"),
    ("activation", lambda o: o.update(activation="relu"), "activation must be one of"),
    ("gated n", lambda o: o.update(size_n=96, activation="silu_mul"), "silu_mul needs size_n % 64 == 0"),
    ("A shape", lambda o: o.update(A=o["A"][:3]), "A must be a contiguous [size_m, size_k] tensor"),
    ("B size", lambda o: o.update(B=o["B"][:1]), "B does not hold size_n * size_k packed 4-bit weights"),
    ("s size", lambda o: o.update(s=o["s"][:7]), "s does not hold size_n * size_k / 32 scales"),
    ("gs dtype", lambda o: o.update(global_scale=torch.ones(1, dtype=torch.float64)), "global_scale must be float32"),
    ("bias", lambda o: o.update(bias=torch.zeros(31, dtype=o["A"].dtype)), "bias must be a contiguous [size_n] tensor of A's dtype on A's device"),
    ("device", lambda o: None, "all tensors must be on GPU"),
]
BROKEN_Q = [
    ("fmt mismatch", lambda o: o.update(fmt="mxfp4"), "quantised activations are mxfp8, the call says fmt='mxfp4'"),
    ("shape mismatch", lambda o: o.update(size_m=5), "quantised activations are [4, 256], the call says [5, 256]"),
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
            layer.mul_mxfp4_native_invariant(**o)
        messages.append(str(e.value))
    assert messages[0] == messages[1] and text in messages[0], messages

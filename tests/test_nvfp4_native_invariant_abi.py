"""The batch-invariant native-class GEMM and MoE launch on NVFP4 images (include/petit_amd.h "Batch-invariant native-class GEMM and MoE launch on
NVFP4 images") without a GPU: the four symbols and their declarations, the operator layers' names and texts, every refusal with its code in the
stated order (none of these calls has a device: every code comes from before any launch), the workspace layout, and the two CPU twins -- the
dense one against a numpy statement of the definition on images the host builder wrote, the MoE one against the dense one per expert.
tests/test_nvfp4_native_invariant.py and tests/test_nvfp4_native_moe_invariant.py import the builders below."""
import ctypes as C
import inspect
from pathlib import Path

import numpy as np
import pytest
import torch

from petit_kernel import _lib, offline
from test_gpu_parity import O, decode_qact
from test_native_invariant_abi import BF16, FMTS, FP16, MX, NV, OK, SHAPE, KERNEL, BAD, PTR, dt, expect_plain, from16, host_quantize, to16

L = _lib.lib
ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("petit_gemm_nvfp4_native_invariant", "petit_gemm_nvfp4_native_moe_invariant", "petit_gemm_nvfp4_native_invariant_host",
           "petit_gemm_nvfp4_native_moe_invariant_host")
NAMES = ("mul_nvfp4_native_invariant", "mul_nvfp4_native_moe_invariant")
SHAPES = [(64, 1024), (96, 768), (128, 1536), (64, 4352)]
SPLIT_MAX_M = 64
E4M3_POW2 = {-1: 0x30, 0: 0x38, 1: 0x40}       # the e4m3 bytes of 0.5, 1, 2
FP4 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0])


# --- problem builders (shared with the GPU modules) --------------------------------------------------------------------------------------------

def geometry(n, k, a_type=BF16):
    S, Lk = C.c_uint(0), C.c_uint(0)
    L.petit_gemm_invariant_geometry(n, k, a_type, NV, C.byref(S), C.byref(Lk))
    return S.value, Lk.value


def image_bytes(n, k):
    return int(L.petit_nvfp4_native_image_bytes(k, n))


def build_image(q: np.ndarray, s: np.ndarray):
    """NVFP4 (q uint8 [n, k / 2], e4m3 bytes [n, k / 16]) -> (the host image, uint8 CPU tensor; the image's weights, float64 [n, k], without the
    global scale).  The image is petit_nvfp4_native_image_host's, its weights oracle.nv6_reencode's -- and the two agree."""
    n, k = q.shape[0], q.shape[1] * 2
    b = offline.repack_nvfp4_cpu(torch.from_numpy(q).view(torch.int32), n, k).contiguous()
    sp = offline.process_nvfp4_scales_cpu(torch.from_numpy(s).view(torch.float8_e4m3fn), n, k).contiguous()
    image = offline.nvfp4_native_image_cpu(b, sp, n, k)
    w, _ = O.nv6_reencode(q, s)
    assert np.array_equal(offline.nvfp4_native_image_dequant_cpu(image, n, k).numpy(), w)
    return image, w.astype(np.float64)


def random_nvfp4(n, k, seed):
    """checkpoint-like NVFP4: every code, group scales over [0.25, 3.75)"""
    rng = np.random.default_rng([seed, n, k, 6])
    q = rng.integers(0, 256, (n, k // 2), dtype=np.uint8)
    s = torch.from_numpy((rng.random((n, k // 16), dtype=np.float32) * 3.5 + 0.25)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return q, s


def exact_nvfp4(n, k, seed):
    """NVFP4 weights whose image is exact: the two group scales of every 32-k block are the same power of two (0.5, 1 or 2), so every fp4 x scale
    is an e2m3 number under the block's E8M0 byte.  -> (q, s, the true weights float64)"""
    rng = np.random.default_rng([seed, n, k, 7])
    code = rng.integers(0, 16, (n, k), dtype=np.uint8)
    e = rng.integers(-1, 2, (n, k // 32))
    q = (code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8)
    s = np.repeat(np.vectorize(E4M3_POW2.get)(e), 2, axis=1).astype(np.uint8)
    return q, s, FP4[code] * np.repeat(np.ldexp(1.0, e), 32, axis=1)


def exact_image(n, k, seed):
    """-> (image, weights float64): asserted exact on the CPU -- the image's dequant equals the oracle's dequant of the NVFP4 tensors"""
    q, s, w = exact_nvfp4(n, k, seed)
    image, w6 = build_image(q, s)
    assert np.array_equal(O.dequant_nvfp4(q, s).astype(np.float64), w) and np.array_equal(w6, w)
    return image, w


def exact_activations(m, k, seed):
    """Activations every format's quantiser keeps exactly, with exact partial sums against exact_image (the builder of
    tests/test_native_invariant_abi.py, re-stated): per 32-k block small integers out of {0, 1, 2, 3, 4, 6} with a 4 or a 6 among them (the
    block maximum then lands on the formats' top binade) or an all-zero block, signs at random, times one power of two per block."""
    rng = np.random.default_rng([seed, m, k, 2])
    v = np.array([0.0, 1, 2, 3, 4, 6])[rng.integers(0, 6, (m, k // 32, 32))] * (rng.random((m, k // 32, 32)) < 0.6)
    v[:, :, 0] = np.array([4.0, 6.0])[rng.integers(0, 2, (m, k // 32))]
    v *= rng.choice([-1.0, 1.0], v.shape)
    v[rng.random((m, k // 32)) < 0.1] = 0.0
    v *= np.ldexp(1.0, rng.integers(-1, 2, (m, k // 32)))[:, :, None]
    return v.reshape(m, k)


def twin(qa: np.ndarray, image: torch.Tensor, gs, bias_bits, m, n, k, is_bf16, fmt) -> np.ndarray:
    """petit_gemm_nvfp4_native_invariant_host on host bytes -> the uint16 patterns of c [m, n]"""
    out = np.full((m, n), 0x7FC1, dtype=np.uint16)
    gsf = None if gs is None else C.byref(C.c_float(gs))
    bias_bits = None if bias_bits is None else np.ascontiguousarray(bias_bits)
    rc = L.petit_gemm_nvfp4_native_invariant_host(out.ctypes.data, qa.ctypes.data, image.data_ptr(), gsf,
                                                  None if bias_bits is None else bias_bits.ctypes.data, m, n, k, BF16 if is_bf16 else FP16,
                                                  FMTS[fmt])
    assert rc == OK
    return out


def numpy_statement(a_q: np.ndarray, w: np.ndarray, S: int, Lk: int):
    """The definition in numpy: every product formed in float64 (exact) and rounded once to fp32, one sequential fp32 sum per slice with k
    ascending, the slices added ascending in fp32.  -> (fold fp32 [m, n], the S partial sums)"""
    m, k = a_q.shape
    parts = []
    for sl in range(S):
        acc = np.zeros((m, w.shape[0]), dtype=np.float32)
        for kk in range(sl * Lk, min(k, (sl + 1) * Lk)):
            acc = acc + (a_q[:, kk, None] * w[None, :, kk]).astype(np.float32)
        parts.append(acc)
    y = parts[0]
    for p in parts[1:]:
        y = y + p
    return y, parts


# --- the ABI ---------------------------------------------------------------------------------------------------------------------------------

def test_symbols_exist_and_are_declared():
    raw = C.CDLL(str(_lib.LIB_PATH))
    header = (ROOT / "include" / "petit_amd.h").read_text()
    assert "Batch-invariant native-class GEMM and MoE launch on NVFP4 images" in header
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert f"int {name}(" in header, name


def test_both_operator_layers_export_the_names():
    import petit_kernel
    from petit_kernel import compiled, ops
    for name in NAMES:
        assert name in petit_kernel.__all__ and callable(getattr(petit_kernel, name))
        sigs = [inspect.signature(getattr(mod, name)) for mod in (ops, compiled, petit_kernel)]
        rows = [[(p.name, p.default, p.kind) for p in sig.parameters.values()] for sig in sigs]
        assert rows[0] == rows[1], name
        assert [r[0].lower() for r in rows[0]] == [r[0].lower() for r in rows[2]], name
    assert list(inspect.signature(ops.mul_nvfp4_native_invariant).parameters) == ["A", "image", "global_scale", "size_m", "size_n", "size_k", "fmt",
                                                                                   "bias", "activation"]
    assert list(inspect.signature(ops.mul_nvfp4_native_moe_invariant).parameters) == [
        "A", "images", "global_scales", "expert_offsets", "size_m", "size_n", "size_k", "num_experts", "a_row_index", "c_row_index", "c_rows", "fmt",
        "bias", "activation"]
    assert inspect.signature(ops.mul_nvfp4_native_invariant).parameters["fmt"].default == "mxfp8"


def test_geometry_facts_of_the_shapes():
    """span sizes 8 / 2 / 4, an odd count of 32-row blocks among them, and S = 9 with a last slice of 256 against L = 512"""
    span = lambda k: 8 if k % 1024 == 0 else 4 if k % 512 == 0 else 2  # noqa: E731  (span_tiles_for_k, csrc/layout.h)
    assert [span(k) for _, k in SHAPES[:3]] == [8, 2, 4]
    assert [n // 32 for n, _ in SHAPES[:3]] == [2, 3, 4] and (96 // 32) % 2 == 1
    assert geometry(64, 1024) == (4, 256) and geometry(96, 768) == (3, 256) and geometry(128, 1536) == (6, 256)
    assert geometry(64, 4352) == (9, 512) and 4352 - 8 * 512 == 256
    for n, k in SHAPES:
        assert geometry(n, k, FP16) == geometry(n, k) and image_bytes(n, k) == n * k * 3 // 4 + n * k // 32


def _dense(a_type=BF16, m=4, n=64, k=256, fmt=8, quantized=0, c=PTR, a=PTR, image=PTR, gs=PTR, hints="auto", epi=None, ws=PTR, c_type=None,
           b_type=NV):
    if hints == "auto":
        hints = C.byref(_lib.SolutionHints(a_type, b_type, a_type if c_type is None else c_type, 0))
    return L.petit_gemm_nvfp4_native_invariant(c, a, image, gs, m, n, k, hints, fmt, quantized, epi, ws, None)


def _moe(a_type=BF16, E=4, m=4, n=64, k=256, fmt=8, quantized=0, c=PTR, a=PTR, images=PTR, gs=PTR, off=PTR, a_idx=None, a_rows=None, c_idx=None,
         c_rows=None, hints="auto", epi=None, ws=PTR, b_type=NV):
    if hints == "auto":
        hints = C.byref(_lib.SolutionHints(a_type, b_type, a_type, 0))
    return L.petit_gemm_nvfp4_native_moe_invariant(c, a, images, gs, off, E, m, n, k, a_idx, m if a_rows is None else a_rows, c_idx,
                                                   m if c_rows is None else c_rows, hints, fmt, quantized, epi, ws, None)


GATED = lambda act: C.byref(_lib.Epilogue(None, act, 0))  # noqa: E731
ODD = C.c_void_p(0x1010)                                   # 16-byte aligned, not 256


@pytest.mark.parametrize("quantized", [0, 1])
@pytest.mark.parametrize("a_type", [BF16, FP16])
@pytest.mark.parametrize("call", [_dense, _moe], ids=["dense", "moe"])
def test_refusals_and_their_codes_in_the_stated_order(call, a_type, quantized):
    """Dummy pointers and a null stream throughout: a call that got as far as a launch would have nothing to run on.  A call that breaks two
    rules returns the code of the earlier one."""
    f = lambda **kw: call(a_type=a_type, quantized=quantized, **kw)  # noqa: E731
    img = "image" if call is _dense else "images"
    # 1. the hints
    assert f(hints=None) == BAD
    for b_type in (MX, BF16, 0):
        assert f(b_type=b_type) == BAD and f(b_type=b_type, n=48) == BAD and f(b_type=b_type, **{img: ODD}) == BAD
    for fmt in (0, 5, 7, 16, -4):
        assert f(fmt=fmt) == BAD and f(fmt=fmt, k=128) == BAD
    for act in (3, -1, 77):
        assert f(epi=GATED(act)) == BAD
    assert f(epi=C.byref(_lib.Epilogue(None, 0, 1))) == BAD
    # 2. the shape
    assert f(n=48) == SHAPE and f(n=16) == SHAPE and f(n=0) == SHAPE                       # n % 32: no padded last block
    assert f(k=128) == SHAPE and f(k=384) == SHAPE and f(k=0) == SHAPE                     # k % 256
    assert f(n=96, epi=GATED(1)) == SHAPE and f(n=96, epi=GATED(2)) == SHAPE               # gated: n % 64
    assert f(n=1 << 18, k=22016, m=1) == SHAPE                                             # n * k * 3 / 4 >= 2^32
    indexed = dict(c_idx=PTR, a_idx=None if quantized else PTR) if call is _moe else {}   # (a NULL index would need m rows behind it)
    assert f(m=1 << 20, **indexed) == SHAPE
    # 3. the image's address, ahead of the row limit
    assert f(**{img: ODD}) == SHAPE and f(**{img: C.c_void_p(0x1080)}) == SHAPE
    if call is _dense and not quantized:
        assert f(m=65536, image=ODD) == SHAPE and f(m=65536, n=48) == SHAPE
        # 4. the quantiser's row limit
        assert f(m=65536) == KERNEL and f(m=65536, ws=None) == KERNEL and f(m=65535, c=None) == SHAPE
    if call is _moe:
        assert f(m=70000, c=None, **indexed) == SHAPE                                      # no row limit: the next refusal is the null c
        assert f(E=0) == SHAPE and f(E=1025) == SHAPE and f(off=None) == SHAPE and f(gs=None) == SHAPE
        assert quantized or f(a_rows=3) == SHAPE                                           # a NULL A index needs m rows behind it (16-bit input)
        assert f(c_rows=3) == SHAPE
        if quantized:
            assert f(a_idx=PTR) == BAD
    # then the pointers and the workspace
    for name in ("c", "a", img):
        assert f(**{name: None}) == SHAPE, name
    assert f(c=C.c_void_p(0x1008)) == SHAPE and f(a=C.c_void_p(0x1008)) == SHAPE
    assert f(ws=None) == SHAPE and f(ws=C.c_void_p(0x1010)) == SHAPE                       # the byte query is not zero at m = 4
    assert f(epi=C.byref(_lib.Epilogue(0x1004, 0, 0))) == SHAPE
    # m == 0: nothing to do
    assert f(m=0, c=None, a=None, ws=None, **{img: None}) == OK


def test_the_mxfp4_entries_still_refuse_nvfp4():
    for a_type in (BF16, FP16):
        hints = C.byref(_lib.SolutionHints(a_type, NV, a_type, 0))
        assert L.petit_gemm_mxfp4_native_invariant(PTR, PTR, PTR, PTR, PTR, 4, 64, 256, hints, 8, 0, None, PTR, None) == BAD
        assert L.petit_gemm_mxfp4_native_moe_invariant(PTR, PTR, PTR, PTR, PTR, PTR, 4, 4, 64, 256, None, 4, None, 4, hints, 8, 0, None, PTR,
                                                       None) == BAD


@pytest.mark.parametrize("a_type", [BF16, FP16])
@pytest.mark.parametrize("n,k", SHAPES)
def test_workspace_is_the_documented_layout(n, k, a_type):
    """quantised bytes (16-bit input only), then the slabs (split form only), each rounded up to 256: the queries of the MXFP4 native entries,
    which answer for these entries because the form constants are shared"""
    S, _ = geometry(n, k, a_type)
    r256 = lambda x: (x + 255) // 256 * 256  # noqa: E731
    for m in (1, 8, 9, 33, 64, 65, 200):
        split = m <= SPLIT_MAX_M
        assert L.petit_gemm_native_invariant_slabs(m, n, k, a_type) == (S if split else 1)
        for fmt in (8, 6, 4):
            qbytes = m * (k // 8 * fmt) + m * (k // 32)
            slab = r256(S * m * n * 4) if split else 0
            assert L.petit_gemm_native_invariant_workspace_bytes(m, n, k, a_type, fmt, 0) == r256(qbytes) + slab
            assert L.petit_gemm_native_invariant_workspace_bytes(m, n, k, a_type, fmt, 1) == slab
            for E in (1, 4, 16):
                msplit = (m + min(E, m) - 1) // min(E, m) <= 8 and m <= 8
                assert L.petit_gemm_native_moe_invariant_form(m, E) == int(msplit)
                mslab = r256(S * m * n * 4) if msplit else 0
                assert L.petit_gemm_native_moe_invariant_workspace_bytes(E, m, n, k, a_type, fmt, 0) == r256(qbytes) + mslab
                assert L.petit_gemm_native_moe_invariant_workspace_bytes(E, m, n, k, a_type, fmt, 1) == mslab


def test_the_host_entries_refuse_before_reading():
    host, mhost = L.petit_gemm_nvfp4_native_invariant_host, L.petit_gemm_nvfp4_native_moe_invariant_host
    assert host(PTR, PTR, PTR, None, None, 4, 64, 128, BF16, 8) == SHAPE and host(PTR, PTR, PTR, None, None, 4, 48, 256, BF16, 8) == SHAPE
    assert host(None, PTR, PTR, None, None, 4, 64, 256, BF16, 8) == SHAPE and host(PTR, PTR, None, None, None, 4, 64, 256, BF16, 8) == SHAPE
    assert host(PTR, PTR, PTR, None, None, 4, 64, 256, 0, 8) == BAD and host(PTR, PTR, PTR, None, None, 4, 64, 256, FP16, 5) == BAD
    assert host(None, None, None, None, None, 0, 64, 256, FP16, 6) == OK
    assert mhost(PTR, PTR, PTR, PTR, None, PTR, 0, 4, 64, 256, None, 4, BF16, 8) == SHAPE
    assert mhost(PTR, PTR, PTR, PTR, None, None, 4, 4, 64, 256, None, 4, BF16, 8) == SHAPE
    assert mhost(None, None, None, None, None, None, 4, 0, 64, 256, None, 0, BF16, 8) == OK


# --- the CPU twins ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("fmt", list(FMTS))
@pytest.mark.parametrize("n,k", SHAPES)
def test_twin_is_the_numpy_statement(n, k, fmt, is_bf16):
    """Random NVFP4 weights through the host image builder, random rows through the host quantiser: the twin's bits are the numpy statement's,
    plain, with a global scale, with a bias, with both; and a row alone gets its bits of the batch."""
    m = 3
    S, Lk = geometry(n, k)
    image, w = build_image(*random_nvfp4(n, k, 3))
    rng = np.random.default_rng([5, n, k])
    bits = to16(rng.standard_normal((m, k)), is_bf16, exact=False)
    qa = host_quantize(bits, is_bf16, fmt)
    a_q = decode_qact(qa, m, k, fmt).astype(np.float64)
    fold, _ = numpy_statement(a_q, w, S, Lk)
    bias = from16(to16(rng.standard_normal(n), is_bf16, exact=False), is_bf16)
    for gs in (0.37, None):
        for use_bias in (True, False):
            got = twin(qa, image, gs, to16(bias, is_bf16) if use_bias else None, m, n, k, is_bf16, fmt)
            want = expect_plain(fold, None if gs is None else float(np.float32(gs)), bias if use_bias else None, is_bf16)
            assert np.array_equal(got, want), (gs, use_bias, int((got != want).sum()))
    alone = twin(host_quantize(bits[1:2], is_bf16, fmt), image, 0.37, None, 1, n, k, is_bf16, fmt)
    assert np.array_equal(alone[0], twin(qa, image, 0.37, None, m, n, k, is_bf16, fmt)[1])


@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("fmt", list(FMTS))
def test_twin_is_the_float64_result_on_exact_inputs(fmt, is_bf16):
    n, k, m = 96, 768, 3
    image, w = exact_image(n, k, 3)
    a = exact_activations(m, k, 3)
    qa = host_quantize(to16(a, is_bf16), is_bf16, fmt)
    assert np.array_equal(decode_qact(qa, m, k, fmt).astype(np.float64), a)
    fold = a @ w.T
    assert (np.abs(a) @ np.abs(w).T).max() < 2 ** 22
    bias = np.random.default_rng(5).integers(-8, 9, n) * 0.5
    got = twin(qa, image, 0.25, to16(bias, is_bf16), m, n, k, is_bf16, fmt)
    assert np.array_equal(got, expect_plain(fold.astype(np.float32), 0.25, bias, is_bf16))


ROUTINGS = {
    "even": lambda m: [0, m // 4, m // 2, 3 * m // 4, m],
    "empty experts": lambda m: [0, 0, m // 2, m // 2, m],
    "all on the last": lambda m: [0, 0, 0, 0, m],
    "decreasing": lambda m: [0, 6, 2, 8, m],
    "beyond m, negative": lambda m: [-3, 4, -1, 3 * m, 5],
    "rows of no expert": lambda m: [2, 4, 6, 6, m - 2],
}


def owners(off, m):
    own, lo = np.full(m, -1), min(max(off[0], 0), m)
    for e in range(len(off) - 1):
        hi = min(max(off[e + 1], lo), m)
        own[lo:hi] = e
        lo = hi
    return own


@pytest.mark.parametrize("routing", list(ROUTINGS))
@pytest.mark.parametrize("fmt,is_bf16", [("mxfp8", True), ("mxfp6", False), ("mxfp4", True)])
def test_moe_twin_is_the_dense_twin_per_expert(fmt, is_bf16, routing):
    E, m, n, k = 4, 11, 64, 1024
    per = image_bytes(n, k)
    images = torch.cat([build_image(*random_nvfp4(n, k, 20 + e))[0] for e in range(E)])
    rng = np.random.default_rng([9, m])
    bits = to16(rng.standard_normal((m, k)), is_bf16, exact=False)
    qa = host_quantize(bits, is_bf16, fmt)
    gs = (0.5 + rng.random(E)).astype(np.float32)
    bias = to16(rng.standard_normal((E, n)), is_bf16, exact=False)
    off = np.array(ROUTINGS[routing](m), dtype=np.int32)
    c_rows = m + 2
    c_idx = ((np.arange(m) * 7 + 3) % c_rows).astype(np.int32)
    c_idx[1], c_idx[3] = c_rows, -2                                                        # outside [0, c_rows): stores nothing
    for idx in (None, c_idx):
        rows_out = m if idx is None else c_rows
        out = np.full((rows_out, n), 0x7FC1, dtype=np.uint16)
        rc = L.petit_gemm_nvfp4_native_moe_invariant_host(out.ctypes.data, qa.ctypes.data, images.data_ptr(), gs.ctypes.data, bias.ctypes.data,
                                                          off.ctypes.data, E, m, n, k, None if idx is None else idx.ctypes.data, rows_out,
                                                          BF16 if is_bf16 else FP16, FMTS[fmt])
        assert rc == OK
        want = np.full((rows_out, n), 0x7FC1, dtype=np.uint16)
        for r, e in enumerate(owners(off.tolist(), m)):
            dst = r if idx is None else int(idx[r])
            if e >= 0 and 0 <= dst < rows_out:
                want[dst] = twin(host_quantize(bits[r:r + 1], is_bf16, fmt), images[e * per:(e + 1) * per], float(gs[e]), bias[e], 1, n, k, is_bf16,
                                 fmt)[0]
        assert np.array_equal(out, want)


# --- the operator layers' texts ----------------------------------------------------------------------------------------------------------------

def _cpu_operands(dtype, moe, m=4, n=64, k=256, E=3):
    A = torch.zeros(m, k, dtype=dtype)
    if moe:
        return dict(A=A, images=torch.zeros(E * image_bytes(n, k), dtype=torch.uint8), global_scales=torch.ones(E),
                    expert_offsets=torch.zeros(E + 1, dtype=torch.int32), size_m=m, size_n=n, size_k=k, num_experts=E)
    return dict(A=A, image=torch.zeros(image_bytes(n, k), dtype=torch.uint8), global_scale=torch.ones(1), size_m=m, size_n=n, size_k=k)


BROKEN = [
    ("fmt", lambda o: o.update(fmt="mxfp5"), "fmt must be 'mxfp8', 'mxfp6' or 'mxfp4'"),
    ("dtype", lambda o: o.update(A=o["A"].float()), "A must be bfloat16 or float16"),
    ("k", lambda o: o.update(size_k=128), "Incompatible problem shape (m=4, n=64, k=128)"),
    ("n", lambda o: o.update(size_n=48), "needs n % 32 == 0, k % 256 == 0, m < 2^20"),
    ("gated n", lambda o: o.update(size_n=96, activation="silu_mul"), "silu_mul needs size_n % 64 == 0"),
    ("image", lambda o: o.update({key: o[key][:-1] for key in o if key.startswith("image")}), "native image"),
    ("device", lambda o: None, "all tensors must be on GPU"),
]


@pytest.mark.parametrize("moe", [False, True], ids=["dense", "moe"])
@pytest.mark.parametrize("case", BROKEN, ids=[b[0] for b in BROKEN])
def test_both_layers_raise_the_same_texts(case, moe):
    from petit_kernel import compiled, ops
    _, breakage, text = case
    name = NAMES[int(moe)]
    messages = []
    for layer in (ops, compiled):
        o = _cpu_operands(torch.bfloat16, moe)
        breakage(o)
        with pytest.raises(RuntimeError) as e:
            getattr(layer, name)(**o)
        messages.append(str(e.value))
    assert messages[0] == messages[1] and text in messages[0], messages
    if case[0] in ("k", "n"):
        assert name in messages[0]

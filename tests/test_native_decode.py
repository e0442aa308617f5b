"""The decode GEMM on the native image (include/petit_amd.h "Decode on the native image"): 1 <= m <= 32 rows against a "petit-cdna4-nv6/1" image.
Without a GPU: the symbols, the names, the refusals and the workspace arithmetic.  On the GPU: float64 bit for bit on exact inputs (every
accumulation order is exact there), the gated epilogues, 16-bit input against quantised input, the class's derived bound on checkpoint-like
weights, and the write contract.  Shapes (n, k): (64, 1024) one part of 8 k-tiles; (96, 768) spans of 2, and 3 k-tiles per part at
k_parts = 2, so W = 3 waves; (80, 1280) a last block with 16 rows >= n, ten k-tiles that do not divide among four waves."""
import ctypes as C
import functools
import inspect
import types
from pathlib import Path

import numpy as np
import pytest
import torch

from petit_kernel import _lib, offline
from test_gated_contract import expect as gated_expect
from test_gpu_parity import DEV, decode_qact, native_exact_bound, pk  # noqa: F401
from test_native_invariant_abi import BAD, BF16, FMTS, FP16, KERNEL, NV, OK, PTR, SHAPE, dt, expect_plain, host_quantize, to16
from test_nvfp4_native_invariant_abi import build_image, exact_activations, exact_image, random_nvfp4

L = _lib.lib
SYMBOLS = ("petit_gemm_nvfp4_native_decode", "petit_gemm_nvfp4_native_decode_parts", "petit_gemm_nvfp4_native_decode_workspace_bytes")
NAMES = ("mul_nvfp4_native_decode", "nvfp4_native_decode_parts", "nvfp4_native_decode_workspace_bytes")
SHAPES = [(64, 1024), (96, 768), (80, 1280)]
CASES = [(fmt, is_bf16) for fmt in FMTS for is_bf16 in (True, False)]
IDS = [f"{fmt}-{'bf16' if b else 'fp16'}" for fmt, b in CASES]
POISON = {True: 0x7FC1, False: 0x7E01}         # a NaN of the output type: no expected value is one
GUARD = 4096
gpu = pytest.mark.gpu


def dev16(bits, is_bf16):
    return torch.from_numpy(bits.view(np.int16).copy()).view(dt(is_bf16)).to(DEV)


def out_bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


@functools.lru_cache(maxsize=8)
def weights(n, k, kind):
    """-> (the image's weights float64, the image on the device), computed once per shape"""
    image, w = exact_image(n, k, 17) if kind == "exact" else build_image(*random_nvfp4(n, k, 17))
    return w, image.to(DEV)


# --- 1. without a GPU ------------------------------------------------------------------------------------------------------------------------

def test_symbols_and_names():
    import petit_kernel
    from petit_kernel import compiled, ops
    raw = C.CDLL(str(_lib.LIB_PATH))
    header = (Path(__file__).resolve().parent.parent / "include" / "petit_amd.h").read_text()
    assert "Decode on the native image" in header
    for name in SYMBOLS:
        assert hasattr(raw, name) and name in _lib.EXPORTED_SYMBOLS and f" {name}(" in header, name
    for name in NAMES:
        assert name in petit_kernel.__all__ and callable(getattr(petit_kernel, name))
        rows = [[(p.name, p.default, p.kind) for p in inspect.signature(getattr(mod, name)).parameters.values()] for mod in (ops, compiled)]
        assert rows[0] == rows[1], name


def _call(m=4, n=64, k=1024, fmt=8, act=0, k_parts=0, ws=None, ws_bytes=0):
    hints = _lib.SolutionHints(BF16, NV, BF16, 0)
    epi = C.byref(_lib.Epilogue(None, act, 0)) if act else None
    return L.petit_gemm_nvfp4_native_decode(PTR, PTR, PTR, None, m, n, k, C.byref(hints), fmt, 0, epi, k_parts, ws, ws_bytes, None)


def test_refusals_and_their_codes():
    """none of these calls has a device: every code comes from before any launch"""
    assert _call(m=0) == SHAPE and _call(m=33) == SHAPE and _call(k=1024 + 128) == SHAPE
    assert _call(n=96, act=1) == SHAPE and _call(n=96, act=2) == SHAPE              # (n / 2) % 32 != 0
    assert _call(k_parts=17) == BAD and _call(k=256, k_parts=3) == BAD              # W P > 16; a part without a k-tile
    assert _call(fmt=5) == BAD
    assert _call(k_parts=2) == KERNEL and _call(k_parts=2, ws=PTR, ws_bytes=2 * 4 * 64 * 4 - 1) == KERNEL   # no / too little workspace


@pytest.mark.parametrize("n,k", SHAPES + [(8192, 8192), (57344, 8192), (1024, 8192)])
def test_workspace_is_the_stated_arithmetic(n, k):
    auto = L.petit_gemm_nvfp4_native_decode_parts(n, k)
    assert 1 <= auto <= 4 and L.petit_gemm_nvfp4_native_decode_parts(n, k + 128) == 0
    for m in (1, 17, 32):
        for parts in (0, 1, 2, 4):
            P = parts or auto
            assert L.petit_gemm_nvfp4_native_decode_workspace_bytes(m, n, k, parts) == (P * m * n * 4 if P > 1 else 0)
    assert L.petit_gemm_nvfp4_native_decode_workspace_bytes(33, n, k, 2) == 0 and L.petit_gemm_nvfp4_native_decode_workspace_bytes(4, n, k, 17) == 0


# --- 2. exact inputs: float64, bit for bit ---------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("layer", ["ops", "compiled"])
@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
@pytest.mark.parametrize("n,k", SHAPES)
def test_exact_inputs_equal_float64(pk, n, k, fmt, is_bf16, layer):
    """The image is exact (asserted by exact_image), the quantiser is exact, every partial sum is exact in any order: every W and P must give
    the float64 product through the plain epilogue, from both operator layers."""
    mul = getattr(pk, layer).mul_nvfp4_native_decode
    w, image = weights(n, k, "exact")
    bias64 = np.random.default_rng(5).integers(-8, 9, n) * 0.5
    bias = dev16(to16(bias64, is_bf16), is_bf16)
    for m in (1, 2, 16, 17, 31, 32):
        a = exact_activations(m, k, 3)
        bits = to16(a, is_bf16)
        assert (np.abs(a) @ np.abs(w).T).max() < 2 ** 22                 # every partial sum is exact, in any order
        assert np.array_equal(decode_qact(host_quantize(bits, is_bf16, fmt), m, k, fmt).astype(np.float64), a)      # the quantiser is exact
        fold, a_dev = (a @ w.T).astype(np.float32), dev16(bits, is_bf16)
        for gs in (0.25, 1.0 / 3.0, None):
            gsd = None if gs is None else torch.tensor([gs], dtype=torch.float32, device=DEV)
            for use_bias in (True, False):
                want = expect_plain(fold, None if gs is None else float(np.float32(gs)), bias64 if use_bias else None, is_bf16)
                for k_parts in (1, 2, 0):
                    got = out_bits(mul(a_dev, image, gsd, m, n, k, fmt, bias if use_bias else None, None, k_parts))
                    assert np.array_equal(got, want), (m, k_parts, gs, use_bias, int((got != want).sum()))


@gpu
@pytest.mark.parametrize("k_parts", [1, 2])
def test_mxfp6_image_without_a_global_scale(pk, k_parts):
    """an image of quantize_mxfp6_cpu: small integers times a power of two per row are exact in e2m3"""
    n, k, m = 96, 768, 17
    rng = np.random.default_rng(11)
    w = rng.integers(-7, 8, (n, k)) * np.ldexp(1.0, rng.integers(-2, 3, (n, 1)))
    image = offline.quantize_mxfp6_cpu(torch.from_numpy(w).bfloat16())
    assert np.array_equal(offline.dequant_native_image_cpu(image, n, k, torch.float32).double().numpy(), w)
    a = exact_activations(m, k, 4)
    got = out_bits(pk.mul_nvfp4_native_decode(dev16(to16(a, True), True), image.to(DEV), None, m, n, k, "mxfp6", k_parts=k_parts))
    assert np.array_equal(got, expect_plain((a @ w.T).astype(np.float32), None, None, True))


# --- 3. gated epilogues ----------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("act,name", [(1, "silu_mul"), (2, "swiglu_oai")])
@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
def test_gated_epilogues_on_exact_inputs(pk, fmt, is_bf16, act, name):
    """y = fma(fold, gs, bias) with an exact fold through the gated epilogue, held to the gated contract's band (tests/test_gated_contract.py)"""
    n, k = 128, 1024
    w, image = weights(n, k, "exact")
    bias64 = np.random.default_rng(6).integers(-8, 9, n) * 0.125
    gs = 2.0 ** -7
    for m in (1, 32):
        a = exact_activations(32, k, 9)[:m]
        y = (a @ w.T * gs + bias64[None, :]).astype(np.float32).astype(np.float64)
        P = gated_expect(types.SimpleNamespace(y=y), is_bf16, act)
        for k_parts in (1, 2):
            got = out_bits(pk.mul_nvfp4_native_decode(dev16(to16(a, is_bf16), is_bf16), image, torch.tensor([gs], dtype=torch.float32, device=DEV),
                                                      m, n, k, fmt, dev16(to16(bias64, is_bf16), is_bf16), name, k_parts))
            assert got.shape == (m, n // 2) and not P.wrong(got).any(), (m, k_parts, int(P.wrong(got).sum()))


# --- 4. the in-lane quantiser is the library's rule ------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
def test_16_bit_input_equals_quantised_input(pk, fmt, is_bf16):
    n, k = 96, 768
    image = weights(n, k, "random")[1]
    for m in (1, 17, 32):
        a = dev16(to16(np.random.default_rng([31, m]).standard_normal((m, k)), is_bf16, exact=False), is_bf16)
        got16 = out_bits(pk.mul_nvfp4_native_decode(a, image, None, m, n, k, fmt))
        gotq = out_bits(pk.mul_nvfp4_native_decode(pk.quantize_activations(a, fmt), image, None, m, n, k, fmt))
        assert np.array_equal(got16, gotq), (m, int((got16 != gotq).sum()))


# --- 5. checkpoint-like weights inside the class's bound --------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
@pytest.mark.parametrize("n,k", SHAPES)
def test_random_weights_stay_inside_the_derived_bound(pk, n, k, fmt, is_bf16):
    """|c - float64(quantised rows x image weights) gs| <= native_exact_bound (the header's, W P <= 16 additions included) + one rounding to
    the output type (bf16: 2^-8 relative; fp16: 2^-11 and half a subnormal step)"""
    w, image = weights(n, k, "random")
    gs = 0.37
    gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
    for m in (1, 32):
        bits = to16(np.random.default_rng([41, m, k]).standard_normal((m, k)), is_bf16, exact=False)
        a_q = decode_qact(host_quantize(bits, is_bf16, fmt), m, k, fmt).astype(np.float64)
        ref = a_q @ w.T * float(np.float32(gs))
        bound = native_exact_bound(a_q, w, float(np.float32(gs)), fmt) + (2.0 ** -8 if is_bf16 else 2.0 ** -11) * np.abs(ref) + (0.0 if is_bf16 else 2.0 ** -25)
        for k_parts in (1, 2):
            got = pk.mul_nvfp4_native_decode(dev16(bits, is_bf16), image, gsd, m, n, k, fmt, k_parts=k_parts).double().cpu().numpy()
            err = np.abs(got - ref)
            print(f"{fmt} bf16={is_bf16} ({n}, {k}) m={m} P={k_parts}: max err / bound = {(err / bound).max():.3f}")
            assert (err <= bound).all(), (m, k_parts, float((err / bound).max()))


# --- 6. the write contract, through the C ABI ------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("k_parts", [1, 2])
@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
def test_nothing_is_written_outside_c_and_the_queried_workspace(pk, fmt, is_bf16, k_parts):
    n, k, m = 80, 1280, 5
    w, image = weights(n, k, "exact")
    a = exact_activations(m, k, 7)
    src = dev16(to16(a, is_bf16), is_bf16)
    nbytes = int(L.petit_gemm_nvfp4_native_decode_workspace_bytes(m, n, k, k_parts))
    assert nbytes == (k_parts * m * n * 4 if k_parts > 1 else 0)
    ws = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)             # exactly the queried bytes between two guards
    ws.view(torch.int32)[GUARD // 4: (GUARD + nbytes) // 4] = 0x7FC00001                     # the slabs start as NaNs
    cbuf = torch.full((m * n + GUARD,), POISON[is_bf16], dtype=torch.int16, device=DEV)
    c = cbuf[GUARD // 2: GUARD // 2 + m * n]
    assert c.data_ptr() % 16 == 0 and (ws.data_ptr() + GUARD) % 256 == 0 and image.data_ptr() % 256 == 0
    a_type = BF16 if is_bf16 else FP16
    hints = _lib.SolutionHints(a_type, NV, a_type, 0)
    rc = L.petit_gemm_nvfp4_native_decode(c.data_ptr(), src.data_ptr(), image.data_ptr(), None, m, n, k, C.byref(hints), FMTS[fmt], 0, None, k_parts,
                                          (ws.data_ptr() + GUARD) if nbytes else None, nbytes, None)
    assert rc == OK
    torch.cuda.synchronize()
    whole = cbuf.cpu().numpy().view(np.uint16)
    want = expect_plain((a @ w.T).astype(np.float32), None, None, is_bf16)
    assert (want != POISON[is_bf16]).all() and np.array_equal(whole[GUARD // 2: GUARD // 2 + m * n].reshape(m, n), want)
    assert (whole[: GUARD // 2] == POISON[is_bf16]).all() and (whole[GUARD // 2 + m * n:] == POISON[is_bf16]).all()
    wsh = ws.cpu().numpy()
    assert (wsh[:GUARD] == 0xA5).all() and (wsh[GUARD + nbytes:] == 0xA5).all()

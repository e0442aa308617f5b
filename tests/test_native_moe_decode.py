"""The routed-expert decode GEMM on the native images (include/petit_amd.h "MoE decode on the native image").  Without a GPU: the symbol, the
names, the option of the layer and every refusal with its code.  On the GPU: float64 bit for bit on exact inputs through both operator layers and
every row form, the write contract through the C ABI, the stated identity with the dense decode entry on random weights (16-bit and quantised
input, plain and gated), and the decode=True layer against its composition.  Shapes (n, k): (64, 1024) one run of 8 k-tiles over W = 4 waves;
(96, 768) 6 k-tiles in uneven runs; (64, 256) two k-tiles, W = 2.

The routing: E = 4, expert_offsets = [0, 0, 1, 34, 37], m = 40 -- an empty expert, one row, 33 rows (two m-tiles, the second holding one row),
three rows, and three grouped rows past offsets[E]."""
import ctypes as C
import functools
import inspect
from pathlib import Path

import numpy as np
import pytest
import torch

from petit_kernel import _lib
from test_gpu_parity import DEV, pk  # noqa: F401
from test_native_decode import CASES, GUARD, IDS, POISON, dev16, out_bits
from test_native_invariant_abi import BAD, BF16, FMTS, FP16, MX, NV, OK, PTR, SHAPE, expect_plain, to16
from test_nvfp4_native_invariant_abi import build_image, exact_activations, exact_image, random_nvfp4

L = _lib.lib
NAME, SYMBOL = "mul_nvfp4_native_moe_decode", "petit_gemm_nvfp4_native_moe_decode"
SHAPES = [(64, 1024), (96, 768), (64, 256)]
E, M, OFFSETS = 4, 40, [0, 0, 1, 34, 37]
ROW_EXPERT = np.repeat(np.arange(E), np.diff(OFFSETS))        # the expert of grouped rows 0 .. 36
TOKENS, NO_TOKEN_ROW, SKIPPED_ROW = 9, 5, 7                      # a_row_index names 9 tokens, is -1 at row 5; c_row_index is c_rows at row 7
GS = [0.25, 1.0 / 3.0, 0.5, 3.0]
gpu = pytest.mark.gpu


def row_indices():
    rng = np.random.default_rng(23)
    a_idx, c_idx = rng.integers(0, TOKENS, M).astype(np.int32), rng.permutation(M).astype(np.int32)
    a_idx[NO_TOKEN_ROW], c_idx[SKIPPED_ROW] = -1, M
    return a_idx, c_idx


@functools.lru_cache(maxsize=8)
def experts(n, k, kind):
    """-> (each expert's weights float64, the E images back to back on the device), computed once per shape"""
    built = [exact_image(n, k, 17 + e) if kind == "exact" else build_image(*random_nvfp4(n, k, 17 + e)) for e in range(E)]
    return [w for _, w in built], torch.cat([image for image, _ in built]).to(DEV)


def i32(values):
    return torch.tensor(np.asarray(values), dtype=torch.int32, device=DEV)


# --- 1. without a GPU ------------------------------------------------------------------------------------------------------------------------

def test_symbol_names_and_the_layer_option():
    import petit_kernel
    from petit_kernel import compiled, ops
    header = (Path(__file__).resolve().parent.parent / "include" / "petit_amd.h").read_text()
    assert "MoE decode on the native image" in header and f" {SYMBOL}(" in header
    assert hasattr(C.CDLL(str(_lib.LIB_PATH)), SYMBOL) and SYMBOL in _lib.EXPORTED_SYMBOLS
    assert NAME in petit_kernel.__all__ and callable(getattr(petit_kernel, NAME))
    rows = [[(p.name, p.default, p.kind) for p in inspect.signature(getattr(mod, NAME)).parameters.values()] for mod in (ops, compiled)]
    assert rows[0] == rows[1]
    assert [r[0] for r in rows[0]] == list(inspect.signature(ops.mul_nvfp4_native_moe_invariant).parameters)
    decode = inspect.signature(petit_kernel.fp4_moe_native).parameters["decode"]
    assert decode.kind is inspect.Parameter.KEYWORD_ONLY and decode.default is False


def _call(c=PTR, images=PTR, off=PTR, e=E, m=4, n=64, k=1024, a_idx=None, a_rows=4, c_rows=4, fmt=8, quantized=0, act=0, reserved=0,
          hints=(BF16, NV, BF16, 0)):
    epi = C.byref(_lib.Epilogue(None, act, reserved)) if act or reserved else None
    return L.petit_gemm_nvfp4_native_moe_decode(c, PTR, images, None, off, e, m, n, k, a_idx, a_rows, None, c_rows, C.byref(_lib.SolutionHints(*hints)),
                                                fmt, quantized, epi, None)


def test_refusals_and_their_codes():
    """none of these calls has a device: every code comes from before any launch"""
    assert L.petit_gemm_nvfp4_native_moe_decode(PTR, PTR, PTR, None, PTR, E, 4, 64, 1024, None, 4, None, 4, None, 8, 0, None, None) == BAD  # hints
    assert _call(hints=(BF16, NV, FP16, 0)) == BAD and _call(hints=(BF16, MX, BF16, 0)) == BAD and _call(hints=(NV, NV, NV, 0)) == BAD
    assert _call(fmt=5) == BAD and _call(quantized=2) == BAD and _call(reserved=1) == BAD and _call(act=3) == BAD
    assert _call(quantized=1, a_idx=PTR) == BAD
    assert _call(c=None) == BAD and _call(images=None) == BAD and _call(off=None) == BAD
    assert _call(images=C.c_void_p(0x1080)) == BAD and _call(c=C.c_void_p(0x1008)) == BAD and _call(off=C.c_void_p(0x1002)) == BAD
    assert _call(e=0) == SHAPE and _call(e=_lib.PETIT_MOE_MAX_EXPERTS + 1) == SHAPE
    assert _call(n=80) == SHAPE and _call(k=1024 + 128) == SHAPE and _call(n=0) == SHAPE and _call(k=0) == SHAPE
    assert _call(k=1 << 24) == SHAPE and _call(m=1 << 20) == SHAPE and _call(a_rows=1 << 21) == SHAPE          # the 32-bit limits
    assert _call(a_rows=3) == SHAPE and _call(c_rows=3) == SHAPE                                              # a null index over too few rows
    assert _call(n=96, act=1) == SHAPE and _call(n=96, act=2) == SHAPE                                       # (n / 2) % 32 != 0
    assert _call(m=0, a_rows=0, c_rows=0) == OK and _call(m=0, c=None, images=None, off=None) == OK           # nothing to launch


@pytest.mark.parametrize("kwargs", [dict(kind="mxfp4"), dict(transient=True), dict(invariant=True), dict(hadamard=32)], ids=lambda d: next(iter(d)))
def test_the_layer_refuses_what_the_decode_path_does_not_have(kwargs):
    import petit_kernel
    t = torch.zeros(1)
    with pytest.raises(RuntimeError, match="decode=True"):
        petit_kernel.fp4_moe_native(t, t, None, t, t, None, t, t, t, **{"kind": "nvfp4", "decode": True, **kwargs})


# --- 2. exact inputs: float64, bit for bit ---------------------------------------------------------------------------------------------------

def exact_problem(n, k, is_bf16, indexed):
    """-> (A bits, the float64 row each grouped row reads, the expected plain outputs of rows 0 .. 36 as a function of (gs?, bias?))"""
    ws, _ = experts(n, k, "exact")
    a = exact_activations(TOKENS if indexed else M, k, 3)
    a_idx = row_indices()[0] if indexed else np.arange(M)
    rows = np.where(a_idx[:, None] >= 0, a[np.maximum(a_idx, 0)], 0.0)
    bias64 = np.random.default_rng(5).integers(-8, 9, (E, n)) * 0.5
    for e in range(E):
        assert (np.abs(rows) @ np.abs(ws[e]).T).max() < 2 ** 22           # every partial sum is exact, in any order

    def want(use_gs, use_bias):
        return np.stack([expect_plain((rows[r: r + 1] @ ws[e].T).astype(np.float32), float(np.float32(GS[e])) if use_gs else None,
                                      bias64[e] if use_bias else None, is_bf16)[0] for r, e in enumerate(ROW_EXPERT)])
    return to16(a, is_bf16), bias64, want


@gpu
@pytest.mark.parametrize("layer", ["ops", "compiled"])
@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
@pytest.mark.parametrize("n,k", SHAPES)
def test_exact_inputs_equal_float64(pk, n, k, fmt, is_bf16, layer):
    """Exact images, exact quantiser, exact partial sums: every written row is the float64 product through the plain epilogue with its
    expert's scale and bias -- identity rows and indexed rows (repeated tokens, one -1 whose row is the bias alone, a permutation of C with one
    index equal to c_rows), with and without global scales and bias."""
    mul = getattr(pk, layer).mul_nvfp4_native_moe_decode
    images, offs, gsd = experts(n, k, "exact")[1], i32(OFFSETS), torch.tensor(GS, dtype=torch.float32, device=DEV)
    a_idx, c_idx = row_indices()
    for indexed in (False, True):
        bits, bias64, want = exact_problem(n, k, is_bf16, indexed)
        a_dev, bias = dev16(bits, is_bf16), dev16(to16(bias64, is_bf16), is_bf16)
        idx = dict(a_row_index=i32(a_idx), c_row_index=i32(c_idx), c_rows=M) if indexed else {}
        c_of = c_idx if indexed else np.arange(M)
        written = [r for r in range(OFFSETS[E]) if c_of[r] < M]
        for use_gs in (True, False):
            for use_bias in (True, False):
                got = out_bits(mul(a_dev, images, gsd if use_gs else None, offs, M, n, k, E, fmt=fmt, bias=bias if use_bias else None, **idx))
                assert got.shape == (M, n)
                assert np.array_equal(got[c_of[written]], want(use_gs, use_bias)[written]), (indexed, use_gs, use_bias)


@gpu
@pytest.mark.parametrize("quantized", [False, True], ids=["a16", "qact"])
@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
def test_only_the_routed_rows_are_written(pk, fmt, is_bf16, quantized):
    """Through the C ABI into a poisoned C with a guard behind it: the poison survives in the rows the three grouped rows past offsets[E] point
    at, in the row nothing points at (its index is c_rows) and in the guard; every other row is the float64 product."""
    n, k = 96, 768
    bits, bias64, want = exact_problem(n, k, is_bf16, True)
    a_idx, c_idx = row_indices()
    a = dev16(bits, is_bf16)
    src = pk.quantize_activation_rows(a, fmt, i32(a_idx)).data if quantized else a
    images, offs, gsd, bias = experts(n, k, "exact")[1], i32(OFFSETS), torch.tensor(GS, dtype=torch.float32, device=DEV), dev16(to16(bias64, is_bf16), is_bf16)
    ai, ci = i32(a_idx), i32(c_idx)
    cbuf = torch.full((M * n + GUARD,), POISON[is_bf16], dtype=torch.int16, device=DEV)
    a_type = BF16 if is_bf16 else FP16
    rc = L.petit_gemm_nvfp4_native_moe_decode(cbuf.data_ptr(), src.data_ptr(), images.data_ptr(), gsd.data_ptr(), offs.data_ptr(), E, M, n, k,
                                              None if quantized else ai.data_ptr(), TOKENS, ci.data_ptr(), M,
                                              C.byref(_lib.SolutionHints(a_type, NV, a_type, 0)), FMTS[fmt], int(quantized),
                                              C.byref(_lib.Epilogue(bias.data_ptr(), 0, 0)), None)
    assert rc == OK
    torch.cuda.synchronize()
    whole = cbuf.cpu().numpy().view(np.uint16)
    expect = np.full((M, n), POISON[is_bf16], dtype=np.uint16)
    written = [r for r in range(OFFSETS[E]) if r != SKIPPED_ROW]
    expect[c_idx[written]] = want(True, True)[written]
    assert (expect[c_idx[written]] != POISON[is_bf16]).all() and np.array_equal(whole[: M * n].reshape(M, n), expect)
    assert (whole[M * n:] == POISON[is_bf16]).all()


# --- 3. the stated identity: a row is the dense decode entry's row --------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
@pytest.mark.parametrize("n,k", SHAPES)
def test_every_row_is_the_dense_decode_entry_on_that_row(pk, n, k, fmt, is_bf16):
    """random images and rows: row r equals, bit for bit, mul_nvfp4_native_decode(m = 1, k_parts = 1) on its 16-bit row -- and on its quantised
    row -- with its expert's image, global scale and bias; plain, SiLU-mul and SwiGLU-OAI (where n / 2 is whole blocks)"""
    images = experts(n, k, "random")[1]
    per = images.numel() // E
    rng = np.random.default_rng([43, n, k])
    a = dev16(to16(rng.standard_normal((M, k)), is_bf16, exact=False), is_bf16)
    bias = dev16(to16(rng.standard_normal((E, n)), is_bf16, exact=False), is_bf16)
    gsd, offs = torch.tensor(GS, dtype=torch.float32, device=DEV), i32(OFFSETS)
    qa = pk.quantize_activation_rows(a, fmt, i32(np.arange(M)))
    for activation in [None] + (["silu_mul", "swiglu_oai"] if n % 64 == 0 else []):
        got16 = out_bits(pk.mul_nvfp4_native_moe_decode(a, images, gsd, offs, M, n, k, E, fmt=fmt, bias=bias, activation=activation))
        gotq = out_bits(pk.mul_nvfp4_native_moe_decode(qa, images, gsd, offs, M, n, k, E, fmt=fmt, bias=bias, activation=activation))
        for r, e in enumerate(ROW_EXPERT):
            dense = (images[e * per: (e + 1) * per], gsd[e: e + 1], 1, n, k, fmt, bias[e], activation)
            assert np.array_equal(got16[r], out_bits(pk.mul_nvfp4_native_decode(a[r: r + 1], *dense, k_parts=1))[0]), (activation, r)
            assert np.array_equal(gotq[r], out_bits(pk.mul_nvfp4_native_decode(pk.quantize_activations(a[r: r + 1], fmt), *dense, k_parts=1))[0]), (activation, r)


# --- 4. the layer ----------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("norm", [False, True], ids=["combine", "norm"])
def test_the_decode_layer_is_its_composition(pk, norm):
    """fp4_moe_native(decode=True) against align, mul_nvfp4_native_decode per slot, moe_combine (or the fused norm end), bit for bit.  T = 5,
    top-k = 2, E = 4, H = 256; I = 256, the smallest down K an image exists for (k % 256 == 0)."""
    from petit_kernel import moe
    T, topk, H, inter, fmt = 5, 2, 256, 256, "mxfp8"
    rng = np.random.default_rng(61)
    w13 = torch.cat([build_image(*random_nvfp4(2 * inter, H, 70 + e))[0] for e in range(E)]).to(DEV)
    w2 = torch.cat([build_image(*random_nvfp4(H, inter, 80 + e))[0] for e in range(E)]).to(DEV)
    gs13, gs2 = torch.tensor(GS, dtype=torch.float32, device=DEV) / 8, torch.tensor(GS[::-1], dtype=torch.float32, device=DEV) / 8
    hidden = torch.from_numpy(rng.standard_normal((T, H))).to(torch.bfloat16).to(DEV)
    ids = torch.from_numpy(np.stack([rng.permutation(E)[:topk] for _ in range(T)])).to(torch.int32).to(DEV)
    weights = torch.from_numpy(rng.random((T, topk))).float().to(DEV)
    nw = torch.from_numpy(rng.standard_normal(H)).to(torch.bfloat16).to(DEV) if norm else None
    got = pk.fp4_moe_native(hidden, w13, None, gs13, w2, None, gs2, weights, ids, "nvfp4", fmt, norm_weight=nw, decode=True)
    sorted_pos, offsets, token_index = (t.cpu().numpy() for t in pk.moe_align_device(ids, E))
    y = torch.zeros((T * topk, H), dtype=torch.bfloat16, device=DEV)
    p13, p2 = w13.numel() // E, w2.numel() // E
    for r in range(offsets[E]):
        e, t = int(np.searchsorted(offsets, r, side="right")) - 1, token_index[r]
        h = pk.mul_nvfp4_native_decode(hidden[t: t + 1], w13[e * p13: (e + 1) * p13], gs13[e: e + 1], 1, 2 * inter, H, fmt, None, "silu_mul", k_parts=1)
        y[sorted_pos[r]] = pk.mul_nvfp4_native_decode(h, w2[e * p2: (e + 1) * p2], gs2[e: e + 1], 1, H, inter, fmt, k_parts=1)[0]
    want = moe._combine(y, weights, ids, E, moe._norm_end(nw, 1e-6, None, 0.0, None))
    for g, w in zip(got if norm else (got,), want if norm else (want,)):
        assert torch.equal(g.view(torch.int16) if g.dtype == torch.bfloat16 else g, w.view(torch.int16) if w.dtype == torch.bfloat16 else w)

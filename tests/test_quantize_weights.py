"""The weight quantiser (include/petit_amd.h "Weight quantiser"): 16-bit weights -> packed NVFP4 / MXFP4 and one global scale per expert.

`rule()` below is a numpy statement of the contract with exact thresholds in f64 and the f32 global scale; the host twin
(petit_quantize_weights_host) is held to it bit for bit, the device kernels to the host twin bit for bit."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import cdna4_layout as LY
from oracle import oracle as O

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import quantize_weights as QW  # noqa: E402  (the CPU tool the recipe comes from)

MID = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
FP4 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
BF16, FP16, NVFP4, MXFP4 = 5, 4, 3, 7   # PETIT_DTYPE_* (include/petit_amd.h)


# --- the rule, in numpy --------------------------------------------------------------------------------------------------------------------

def to_bits(x, bf16: bool) -> np.ndarray:
    """f32 / f64 values -> the 16-bit patterns of their nearest bf16 / fp16 numbers."""
    x = np.asarray(x, dtype=np.float32)
    return O.f32_to_bf16_bits(x).reshape(x.shape) if bf16 else x.astype(np.float16).view(np.uint16)


def magnitudes(bits: np.ndarray, bf16: bool) -> np.ndarray:
    """|w| of 16-bit patterns, f32 (exact)."""
    mag = bits & 0x7FFF
    return (mag.astype(np.uint32) << 16).view(np.float32) if bf16 else mag.view(np.float16).astype(np.float32)


def e4m3_rne_sat(x: np.ndarray) -> np.ndarray:
    """f32 >= 0 -> e4m3fn bytes, round to nearest even, saturating at 448."""
    x = np.minimum(x.astype(np.float64), 448.0)
    sub = np.rint(x * 512.0)                                    # below 2^-6: multiples of 2^-9 (8 = the byte of 2^-6)
    _, ex = np.frexp(np.maximum(x, 2.0 ** -6))
    e = ex - 1
    q = np.rint(x / np.exp2(e - 3.0))                           # 8 .. 16
    e, q = np.where(q == 16, e + 1, e), np.where(q == 16, 8, q)
    return np.where(x < 2.0 ** -6, sub, ((e + 7) << 3) + (q - 8)).astype(np.uint8)


def e4m3_value(b: np.ndarray) -> np.ndarray:
    e, m = (b >> 3).astype(np.int64), (b & 7).astype(np.float64)
    return np.where(e == 0, m / 512.0, (1.0 + m / 8.0) * np.exp2(e - 7.0))


def codes_from_thresholds(a: np.ndarray, sign: np.ndarray, scale: np.ndarray) -> np.ndarray:
    """a [..., g] f64 magnitudes, scale [...] f64 (t_i = mid_i * scale, exact): the e2m1 codes -- the number of t_i < a, the even code at a tie,
    the sign bit only on a non-zero magnitude."""
    t = MID * scale[..., None, None]                            # [..., 1, 7]
    below = t < a[..., None]
    tie_up = (t == a[..., None]) & (np.arange(7) % 2 == 1)       # at t_1, t_3, t_5 the even code is the upper one
    cnt = (below | tie_up).sum(-1).astype(np.uint8)
    return cnt | ((sign & (cnt != 0)).astype(np.uint8) << 3)


def rule(bits: np.ndarray, bf16: bool, fmt: str, gs=None):
    """bits uint16 [E, N, K] -> (codes uint8 [E, N, K], scale bytes uint8 [E, N, K / g], gs float32 [E])."""
    E, n, k = bits.shape
    a, sign = magnitudes(bits, bf16), (bits >> 15).astype(bool)
    if fmt == "nvfp4":
        if gs is None:
            amax = a.reshape(E, -1).max(1)
            gs = np.where(amax == 0, np.float32(1), amax / np.float32(2688.0)).astype(np.float32)     # one f32 division
        gs = np.asarray(gs, dtype=np.float32)
        blk = a.reshape(E, n, k // 16, 16).max(-1)
        with np.errstate(over="ignore"):
            x = (blk / np.float32(6.0)) / gs[:, None, None]
        assert x.dtype == np.float32
        sb = e4m3_rne_sat(x)
        scale = e4m3_value(sb) * gs[:, None, None].astype(np.float64)
        codes = codes_from_thresholds(a.reshape(E, n, k // 16, 16).astype(np.float64), sign.reshape(E, n, k // 16, 16), scale)
        codes = np.where((sb == 0)[..., None], 0, codes)
        return codes.reshape(E, n, k).astype(np.uint8), sb, gs
    blk = a.reshape(E, n, k // 32, 32).max(-1).astype(np.float64)
    m, ex = np.frexp(blk)                                       # blk = m 2^ex, m in [0.5, 1): 6 * 2^e >= blk first holds at ex - 3 (m <= 0.75) or ex - 2
    e = np.clip(np.where(blk == 0, -126, ex - 3 + (m > 0.75)), -126, 127)
    codes = codes_from_thresholds(a.reshape(E, n, k // 32, 32).astype(np.float64), sign.reshape(E, n, k // 32, 32), np.exp2(e.astype(np.float64)))
    return codes.reshape(E, n, k), (e + 127).astype(np.uint8), np.ones(E, dtype=np.float32)


def dequant_rule(codes, sb, gs, fmt):
    """the f64 weights (without the global scale for the oracle GEMM: it takes gs apart) one expert's codes and scale bytes stand for."""
    g = 16 if fmt == "nvfp4" else 32
    v = FP4[codes & 7] * np.where(codes & 8, -1.0, 1.0)
    s = e4m3_value(sb) if fmt == "nvfp4" else np.exp2(sb.astype(np.float64) - 127.0)
    return (v.reshape(codes.shape[0], -1, g) * s[:, :, None]).reshape(codes.shape)


# --- the host twin --------------------------------------------------------------------------------------------------------------------------

def _lib():
    from petit_kernel import _lib as L
    return L


def _p(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def host_twin(bits: np.ndarray, bf16: bool, fmt: str, gs=None):
    """petit_quantize_weights_host -> (codes [E, N, K], scale bytes [E, N, K / g], gs [E], packed weights u32, packed scales u8)."""
    L = _lib()
    E, n, k = bits.shape
    bits = np.ascontiguousarray(bits)
    g = 16 if fmt == "nvfp4" else 32
    pw, ps, out_gs = np.zeros(E * n * k // 8, np.uint32), np.zeros(E * n * k // g, np.uint8), np.zeros(E, np.float32)
    gs_in = None if gs is None else np.ascontiguousarray(gs, dtype=np.float32)
    rc = L.lib.petit_quantize_weights_host(_p(bits), BF16 if bf16 else FP16, NVFP4 if fmt == "nvfp4" else MXFP4, E, n, k,
                                           None if gs_in is None else _p(gs_in), _p(pw), _p(ps), _p(out_gs))
    assert rc == 0, L.error_string(rc)
    q = LY.unpack_weights(pw, E * n, k).view(np.uint8).reshape(E * n, k // 2)     # the packed layout is n-tile-major: the stack is one matrix
    codes = np.empty((E * n, k), np.uint8)
    codes[:, 0::2], codes[:, 1::2] = q & 15, q >> 4
    sb = (LY.unpack_nvscales if fmt == "nvfp4" else LY.unpack_mxscales)(ps, E * n, k)
    return codes.reshape(E, n, k), sb.reshape(E, n, k // g), out_gs, pw, ps


def random_bits(E, n, k, bf16, seed, spread=True):
    """checkpoint-like weights; with spread, experts of very different size (x 2^-9 .. x 2^9)."""
    w = np.stack([QW.synthetic_weights(n, k, seed + e) for e in range(E)])
    if spread:
        w = w * np.exp2(np.linspace(-9, 9, E, dtype=np.float32))[:, None, None] if E > 1 else w
    return to_bits(w, bf16)


def assert_same(got, want, what):
    for name, g, w in zip(("codes", "scale bytes", "gs"), got[:3], want[:3]):
        g, w = np.asarray(g), np.asarray(w)
        gv, wv = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 else (g, w)
        assert gv.shape == wv.shape and np.array_equal(gv, wv), f"{what}: {name} differ in {int((gv != wv).sum())} of {gv.size} places"


@pytest.mark.parametrize("fmt", ["nvfp4", "mxfp4"])
@pytest.mark.parametrize("bf16", [True, False])
def test_host_twin_is_the_rule(fmt, bf16):
    for i, (E, n, k) in enumerate([(1, 16, 256), (1, 48, 512), (2, 32, 1024), (3, 16, 768)]):
        bits = random_bits(E, n, k, bf16, 10 * i)
        assert_same(host_twin(bits, bf16, fmt), rule(bits, bf16, fmt), f"{fmt} {E}x{n}x{k}")
    if fmt == "nvfp4":   # a supplied (here: shared, power-of-two-free) global scale per expert
        bits = random_bits(2, 32, 512, bf16, 77, spread=False)
        gs = np.array([3.1e-4, 1.7e-5], np.float32)
        assert_same(host_twin(bits, bf16, fmt, gs), rule(bits, bf16, fmt, gs), "supplied gs")


@pytest.mark.parametrize("n,k", [(64, 1024), (256, 2048), (512, 4096), (128, 256)])
def test_host_twin_against_the_cpu_tool(n, k):
    """tools/quantize_weights.py on its own synthetic weights.  MXFP4: bit for bit.  NVFP4: scale bytes and gs bit for bit; the tool divides by
    the float64 amax / 2688 where the contract uses the f32 value the GEMM is given, so a code may differ exactly where |w| / (s gs) lies within
    2^-22 relative of a midpoint -- then by one magnitude step -- and nowhere else.  Seen at seed 0: 51 / 698 / 2868 / 0 differing codes of
    65 536 / 524 288 / 2 097 152 / 32 768 (at most 0.14 %), no differing scale byte; the guard against a test that excuses everything is 0.5 %."""
    w = QW.synthetic_weights(n, k, seed=0)
    bits = to_bits(w, True)[None]
    q, sb, _ = QW.quantize_mxfp4(w)
    codes, hsb, _, _, _ = host_twin(bits, True, "mxfp4")
    assert np.array_equal(hsb[0], sb) and np.array_equal(QW.pack_nibbles(codes[0]), q)

    q, sb, ws2 = QW.quantize_nvfp4(w)
    codes, hsb, gs, _, _ = host_twin(bits, True, "nvfp4")
    assert np.array_equal(hsb[0], sb)
    assert gs[0] == np.float32(ws2) and gs.dtype == np.float32
    tool = np.empty((n, k), np.uint8)
    tool[:, 0::2], tool[:, 1::2] = q & 15, q >> 4
    diff = np.argwhere(tool != codes[0])
    print(f"{n} x {k}: {len(diff)} codes differ of {n * k}")
    assert len(diff) <= 0.005 * n * k
    s = (e4m3_value(sb) * np.float64(gs[0]))
    for r, c in diff:
        lo, hi = sorted((int(tool[r, c] & 7), int(codes[0, r, c] & 7)))
        assert hi == lo + 1, "not neighbouring magnitude codes"
        x = abs(np.float64(w[r, c])) / s[r, c // 16]
        assert abs(x - MID[lo]) <= 2.0 ** -22 * MID[lo]


def tie_block(s, gs, bf16, extra):
    """16 weights whose block scale is s: the block maximum 6 s gs, the seven ties +-mid_i s gs, one value below 0.25 s gs -- all exact."""
    unit = np.float64(s) * np.float64(gs)
    vals = np.concatenate([[6.0], MID, -MID, [extra]]) * unit
    bits = to_bits(vals, bf16)
    assert np.array_equal(magnitudes(bits, bf16).astype(np.float64), np.abs(vals)), "a tie value is not a 16-bit number"
    return bits


@pytest.mark.parametrize("bf16", [True, False])
def test_exact_ties_go_to_the_even_code(bf16):
    tie_codes = [0, 2, 2, 4, 4, 6, 6]                                             # 0.25 -> 0, 0.75 -> 1.0, 1.25 -> 1.0, ..., 5 -> the code of 4
    want = np.array([7] + tie_codes + [c | 8 if c else 0 for c in tie_codes] + [0], np.uint8)   # no -0
    # NVFP4, supplied gs = 2^-10; scales: normal, odd mantissa, the smallest normal, subnormal
    gs, scales = np.float32(2.0 ** -10), [1.0, 1.75, 13.0, 2.0 ** -6, 3 * 2.0 ** -9, 0.5]
    rows = [np.concatenate([tie_block(s, gs, bf16, extra=(0.125 if j % 2 else -0.125)) for j in range(16)]) for s in scales]
    # a block whose scale rounds DOWN (6.375 / 6 = 1.0625: the tie between 1.0 and 1.125 goes to the even 1.0): 6.375 s gs lies above 6 and saturates
    sat = np.array([6.375, -6.375, -0.125, 0.125] + [0.0] * 12) * np.float64(gs)
    rows += [np.concatenate([to_bits(sat, bf16)] * 16)] * (16 - len(rows))
    bits = np.stack(rows)[None]                                                   # [1, 16, 256]
    got = host_twin(bits, bf16, "nvfp4", [gs])
    assert_same(got, rule(bits, bf16, "nvfp4", [gs]), "nvfp4 ties")
    for i, s in enumerate(scales):
        assert (got[1][0, i] == e4m3_rne_sat(np.float32([s]))[0]).all()
        assert np.array_equal(got[0][0, i].reshape(16, 16), np.tile(want[:15].tolist() + [0], (16, 1)))
    assert (got[1][0, len(scales):] == 0x38).all()                                # 1.0
    assert np.array_equal(got[0][0, -1, :16], np.array([7, 15, 0, 0] + [0] * 12, np.uint8))

    # MXFP4: the same with mid_i 2^e and a block maximum of exactly 6 * 2^e (the scale is e, not e + 1); 32 per block: two tie groups
    es = [0, -7, 5, -14] if not bf16 else [0, -7, 5, -40, 60, -120]
    rows = [np.concatenate([tie_block(2.0 ** e, 1.0, bf16, extra=0.125) for _ in range(16)]) for e in es]
    rows += [rows[0]] * (16 - len(rows))
    bits = np.stack(rows)[None]
    got = host_twin(bits, bf16, "mxfp4")
    assert_same(got, rule(bits, bf16, "mxfp4"), "mxfp4 ties")
    for i, e in enumerate(es):
        assert (got[1][0, i] == e + 127).all()
        assert np.array_equal(got[0][0, i].reshape(16, 16), np.tile(want, (16, 1)))


def test_scale_edge_cases():
    bf16 = True
    # MXFP4: amax exactly 6 * 2^e -> e; one bf16 step above -> e + 1; a zero block -> byte 1
    row = np.zeros(256, np.float32)
    row[0], row[32], row[64 + 5] = 6.0 * 2.0 ** -3, 6.03125 * 2.0 ** -3, -6.0 * 2.0 ** 9
    bits = to_bits(np.tile(row, (16, 1)), bf16)[None]
    got = host_twin(bits, bf16, "mxfp4")
    assert_same(got, rule(bits, bf16, "mxfp4"), "mxfp4 scale edges")
    assert got[1][0, 0].tolist() == [124, 125, 127 + 9, 1, 1, 1, 1, 1]
    assert got[0][0, 0, 0] == 7 and got[0][0, 0, 32] == 5 and got[0][0, 0, 69] == 15 and not got[0][0, 0, 96:].any()
    # a zero expert between two others: gs = 1, NV scale bytes 0 / MX bytes 1, every code +0 (also for -0 weights)
    bits = random_bits(3, 16, 256, bf16, 5, spread=False)
    bits[1] = 0
    bits[1, 3, 7] = 0x8000
    for fmt in ("nvfp4", "mxfp4"):
        got = host_twin(bits, bf16, fmt)
        assert_same(got, rule(bits, bf16, fmt), f"{fmt} zero expert")
        assert got[2][1] == 1.0 and not got[0][1].any() and (got[1][1] == (0 if fmt == "nvfp4" else 1)).all()
    # a zero block inside a live NVFP4 row: scale byte 0, codes 0
    bits = random_bits(1, 16, 256, bf16, 6)
    bits[0, :, 16:32] = 0
    got = host_twin(bits, bf16, "nvfp4")
    assert_same(got, rule(bits, bf16, "nvfp4"), "nvfp4 zero block")
    assert (got[1][0, :, 1] == 0).all() and not got[0][0, :, 16:32].any()
    # a supplied gs so small that blk_amax / 6 / gs passes 448: the byte saturates at 0x7e (torch's cast would give NaN), codes saturate at 6
    bits = to_bits(np.random.default_rng(3).standard_normal((1, 16, 256)), bf16)
    gs = [np.float32(2.0 ** -20)]
    got = host_twin(bits, bf16, "nvfp4", gs)
    assert_same(got, rule(bits, bf16, "nvfp4", gs), "saturating scale")
    assert (got[1] == 0x7E).all() and ((got[0] & 7) == 7).mean() > 0.9


def test_refusals():
    import petit_kernel as pk
    from petit_kernel import offline
    L = _lib()
    q = L.lib.petit_quantize_weights
    buf = np.zeros(1 << 16, np.uint8)
    ptr = C.c_void_p((buf.ctypes.data + 255) & ~255)

    def dev_call(a_type=BF16, b_type=NVFP4, E=1, n=16, k=256, gs=None, ws=None, ws_bytes=0):
        # every refusal comes before the first launch: no pointer is dereferenced and no device is touched
        return q(ptr, a_type, b_type, E, n, k, gs, ptr, ptr, ptr, ws, ws_bytes, None)

    def host_call(a_type=BF16, b_type=NVFP4, E=1, n=16, k=256):
        return L.lib.petit_quantize_weights_host(ptr, a_type, b_type, E, n, k, None, ptr, ptr, ptr)

    for call in (dev_call, host_call):
        assert call(n=24) == L.PETIT_ERROR_PROBLEM_SHAPE
        assert call(k=384) == L.PETIT_ERROR_PROBLEM_SHAPE and call(k=128) == L.PETIT_ERROR_PROBLEM_SHAPE
        assert call(a_type=100) == L.PETIT_ERROR_BAD_ARGUMENT and call(a_type=NVFP4) == L.PETIT_ERROR_BAD_ARGUMENT
        assert call(b_type=BF16) == L.PETIT_ERROR_BAD_ARGUMENT
        assert call(E=1 << 20, n=1 << 12) == L.PETIT_ERROR_PROBLEM_SHAPE
    # the amax scratch: 4 bytes per expert for NVFP4 without a supplied scale, none otherwise
    need = L.lib.petit_quantize_weights_workspace_bytes
    assert (need(NVFP4, 5, 0), need(NVFP4, 5, 1), need(MXFP4, 5, 0)) == (20, 0, 0)
    assert dev_call(E=5) == L.PETIT_ERROR_KERNEL_SHAPE                       # missing
    assert dev_call(E=5, ws=ptr, ws_bytes=16) == L.PETIT_ERROR_BAD_ARGUMENT   # short
    assert q(None, BF16, NVFP4, 1, 16, 256, None, ptr, ptr, ptr, ptr, 4, None) == L.PETIT_ERROR_BAD_ARGUMENT
    assert host_call(n=0) == L.PETIT_OK and dev_call(E=0) == L.PETIT_OK

    # the Python surface: one rule set for both operator layers' CPU twins (and, on the GPU, for the ops)
    w = torch.zeros(32, 256, dtype=torch.bfloat16)
    for bad, text in ((torch.zeros(24, 256, dtype=torch.bfloat16), "size_n = 24 is not divisible"),
                      (torch.zeros(32, 384, dtype=torch.bfloat16), "size_k = 384 is not divisible"),
                      (torch.zeros(32, 512, dtype=torch.bfloat16)[:, ::2], "w is not contiguous"),
                      (torch.zeros(32, 256, dtype=torch.float32), "w must be bfloat16 or float16"),
                      (torch.zeros(256, dtype=torch.bfloat16), "w must be [size_n, size_k] or")):
        for fn in (offline.quantize_nvfp4_cpu, offline.quantize_mxfp4_cpu):
            with pytest.raises(RuntimeError, match=text.replace("[", r"\[")):
                fn(bad)
    with pytest.raises(RuntimeError, match="global_scale must be a contiguous float32"):
        offline.quantize_nvfp4_cpu(w, torch.ones(2))
    with pytest.raises(RuntimeError, match="global_scale must be a contiguous float32"):
        offline.quantize_nvfp4_cpu(w.view(2, 16, 256), torch.ones(1))
    with pytest.raises(RuntimeError, match="MX scale tile"):
        offline.quantize_mxfp4_cpu(w[:16])
    for layer in (pk.ops, pk.compiled):   # a CPU tensor reaches the device ops' own checks
        with pytest.raises(RuntimeError, match="w is not on GPU"):
            layer.quantize_nvfp4(w)
        with pytest.raises(RuntimeError, match="w must be bfloat16 or float16"):
            layer.quantize_mxfp4(torch.zeros(32, 256, dtype=torch.float32))
    assert "quantize_nvfp4" in pk.__all__ and "quantize_mxfp4" in pk.__all__
    # shapes and dtypes of the CPU twins' results: what repack_* / process_*_scales give for the stacked tensor
    b, s, gs = offline.quantize_nvfp4_cpu(w.view(2, 16, 256))
    assert (b.shape, b.dtype, s.shape, s.dtype, gs.shape, gs.dtype) == ((2, 512), torch.int32, (32, 16), torch.float8_e4m3fn, (2,), torch.float32)
    b, s, gs = offline.quantize_mxfp4_cpu(w)
    assert (b.shape, b.dtype, s.shape, s.dtype, gs.tolist()) == ((2, 512), torch.int32, (1, 256), torch.uint8, [1.0])


def test_meta_kernel_gives_the_shapes():
    from petit_kernel import compiled
    assert compiled.available(), compiled.why_unavailable()
    w = torch.empty(3, 32, 512, dtype=torch.float16, device="meta")
    b, s, gs = torch.ops.petit_kernel.quantize_weights(w, NVFP4, None)
    assert (b.shape, b.dtype, s.shape, s.dtype, gs.shape, gs.dtype) == ((6, 1024), torch.int32, (96, 32), torch.float8_e4m3fn, (3,), torch.float32)
    b, s, gs = torch.ops.petit_kernel.quantize_weights(w, MXFP4, None)
    assert (b.shape, s.shape, s.dtype) == ((6, 1024), (3, 512), torch.uint8)


# --- on the GPU -----------------------------------------------------------------------------------------------------------------------------

def device_quantize(bits: np.ndarray, bf16: bool, fmt: str, gs=None, dev="cuda"):
    """petit_quantize_weights through the C ABI (it takes every N % 16, also where the Python surface's MX scale shape needs N % 32) ->
    (packed weights u32, packed scales u8, gs f32) as numpy arrays."""
    L = _lib()
    E, n, k = bits.shape
    g = 16 if fmt == "nvfp4" else 32
    w = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev)
    pw = torch.zeros(E * n * k // 8, dtype=torch.int32, device=dev)
    ps = torch.zeros(E * n * k // g, dtype=torch.uint8, device=dev)
    out_gs = torch.zeros(E, dtype=torch.float32, device=dev)
    gs_in = None if gs is None else torch.tensor(np.asarray(gs, np.float32), device=dev)
    b_type = NVFP4 if fmt == "nvfp4" else MXFP4
    ws_bytes = int(L.lib.petit_quantize_weights_workspace_bytes(b_type, E, int(gs is not None)))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    rc = L.lib.petit_quantize_weights(w.data_ptr(), BF16 if bf16 else FP16, b_type, E, n, k, None if gs_in is None else gs_in.data_ptr(),
                                      pw.data_ptr(), ps.data_ptr(), out_gs.data_ptr(), ws.data_ptr() if ws_bytes else None, ws_bytes,
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.error_string(rc)
    torch.cuda.synchronize()
    return pw.cpu().numpy().view(np.uint32), ps.cpu().numpy(), out_gs.cpu().numpy()


def assert_device_is_host(bits, bf16, fmt, gs=None, what=""):
    pw, ps, ogs = device_quantize(bits, bf16, fmt, gs)
    _, _, hgs, hpw, hps = host_twin(bits, bf16, fmt, gs)
    assert np.array_equal(ogs.view(np.uint32), hgs.view(np.uint32)), f"{what}: gs {ogs} vs {hgs}"
    assert np.array_equal(ps, hps), f"{what}: {int((ps != hps).sum())} of {ps.size} packed scale bytes differ"
    assert np.array_equal(pw, hpw), f"{what}: {int((pw != hpw).sum())} of {pw.size} packed weight words differ"
    return pw, ps, ogs


SHAPES = [(16, 256), (48, 512), (32, 1024), (80, 1280), (16, 1536), (64, 2048)]   # every KS, one and several spans, odd tile counts


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["nvfp4", "nvfp4_gs", "mxfp4"])
@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("n,k", SHAPES)
def test_device_equals_host_twin(n, k, bf16, mode):
    bits = random_bits(1, n, k, bf16, n + k)
    bits[0, n // 2, 32:64] = 0                      # a zero block, and a few exact ties, in every case
    bits[0, 0, :16] = tie_block(1.5, 2.0 ** -10, bf16, 0.125)
    assert_device_is_host(bits, bf16, mode[:5], [np.float32(2.0 ** -10)] if mode == "nvfp4_gs" else None, f"{mode} {n}x{k}")


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["nvfp4", "mxfp4"])
@pytest.mark.parametrize("E,n,k", [(3, 48, 512), (9, 16, 256)])
def test_stacked_experts_are_quantised_on_their_own(E, n, k, fmt):
    bf16 = E == 3
    bits = random_bits(E, n, k, bf16, 40 + E)       # experts x 2^-9 .. x 2^9: very different amax
    bits[1] = 0                                     # and an all-zero one
    pw, ps, gs = assert_device_is_host(bits, bf16, fmt, None, f"{fmt} E={E}")
    g = 16 if fmt == "nvfp4" else 32
    for e in range(E):                              # the per-expert offsets and gs: each expert equals its own E = 1 call
        pw1, ps1, gs1 = device_quantize(bits[e:e + 1], bf16, fmt)
        assert gs[e] == gs1[0]
        assert np.array_equal(pw[e * n * k // 8:(e + 1) * n * k // 8], pw1) and np.array_equal(ps[e * n * k // g:(e + 1) * n * k // g], ps1)
    assert gs[1] == 1.0 and (fmt == "mxfp4" or len(set(gs.tolist())) == E)


def _layers():
    import petit_kernel as pk
    return [pk.ops, pk.compiled]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["nvfp4", "mxfp4"])
def test_the_bytes_are_the_repacks(fmt):
    """quantize_*(w) = repack_nvfp4 / process_*_scales of the host twin's row-major FP4: pins the layout, and the shapes / dtypes, on both layers."""
    E, n, k = 2, 32, 1280
    bits = random_bits(E, n, k, True, 9)
    codes, sb, gs, _, _ = host_twin(bits, True, fmt)
    q = torch.from_numpy(QW.pack_nibbles(codes.reshape(E * n, k))).cuda().view(torch.int32)
    w = torch.from_numpy(bits.view(np.int16)).cuda().view(torch.bfloat16)
    for layer in _layers():
        b_ref = layer.repack_nvfp4(q, E * n, k)
        if fmt == "nvfp4":
            s_ref = layer.process_nvfp4_scales(torch.from_numpy(sb.reshape(E * n, -1)).cuda().view(torch.float8_e4m3fn), E * n, k)
            b, s, g = layer.quantize_nvfp4(w)
        else:
            s_ref = layer.process_mxfp4_scales(torch.from_numpy(sb.reshape(E * n, -1)).cuda(), E * n, k)
            b, s, g = layer.quantize_mxfp4(w)
        assert (b.shape, b.dtype, s.shape, s.dtype) == (b_ref.shape, b_ref.dtype, s_ref.shape, s_ref.dtype)
        assert torch.equal(b, b_ref) and torch.equal(s.view(torch.uint8), s_ref.view(torch.uint8))
        assert g.dtype == torch.float32 and g.shape == (E,) and np.array_equal(g.cpu().numpy().view(np.uint32), gs.view(np.uint32))
    # a 2-D weight is E = 1; a supplied global scale comes back as it is
    b2, s2, g2 = _layers()[0].quantize_nvfp4(w[0], torch.tensor([2.0 ** -9], device="cuda")) if fmt == "nvfp4" else _layers()[0].quantize_mxfp4(w[0])
    assert b2.shape == (n // 16, 2 * k) and g2.tolist() == [2.0 ** -9 if fmt == "nvfp4" else 1.0]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["nvfp4", "mxfp4"])
@pytest.mark.parametrize("bf16", [True, False])
def test_gemm_on_the_quantisers_output(fmt, bf16):
    """mul_*_a16 at M = 4 on quantize_*'s tensors against the oracle GEMM on the rule's dequantised weights, under the suite's bound."""
    import petit_kernel as pk
    m, n, k = 4, 64, 512
    bits = random_bits(1, n, k, bf16, 21) if fmt == "mxfp4" else to_bits(QW.synthetic_weights(n, k, 21) * 40.0, bf16)[None]
    dtype = torch.bfloat16 if bf16 else torch.float16
    w = torch.from_numpy(bits[0].view(np.int16)).cuda().view(dtype)
    a = torch.from_numpy(np.random.default_rng(2).standard_normal((m, k), dtype=np.float32)).to(dtype)
    a_bits = a.view(torch.int16).numpy().view(np.uint16)
    codes, sb, gs = rule(bits, bf16, fmt)
    _, ref = O.gemm_ref(a_bits, bf16, dequant_rule(codes[0], sb[0], gs, fmt).astype(np.float32), float(gs[0]))
    for layer in _layers():
        b, s, g = layer.quantize_nvfp4(w) if fmt == "nvfp4" else layer.quantize_mxfp4(w)
        mul = layer.mul_nvfp4_a16 if fmt == "nvfp4" else layer.mul_mxfp4_a16
        got = mul(a.cuda(), b, s, g, m, n, k, -1).float().cpu().numpy()
        err = np.abs(got - ref)
        print(f"{fmt} {dtype}: max err {err.max():.4g}, max |ref| {np.abs(ref).max():.4g}")
        assert (err <= np.maximum(1e-2, 1e-2 * np.abs(ref))).all(), f"max err {err.max()}"


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["nvfp4", "mxfp4"])
def test_moe_layer_on_the_quantisers_output(fmt):
    """fp4_moe_fused on quantize_*([E, 2I, H]) / quantize_*([E, H, I]) is bit-identical to the layer fed the host twin's packed tensors.
    E = 4, H = 256, T = 8, topk = 2 with I = 256, the smallest intermediate size whose down projection [E, H, I] has K % 256 == 0."""
    import petit_kernel as pk
    from petit_kernel import offline
    E, H, I, T, topk = 4, 256, 256, 8, 2     # (I = 256: the down projection's K, and the quantiser takes K % 256 == 0)
    rng = np.random.default_rng(4)
    w13 = torch.from_numpy(to_bits(rng.standard_normal((E, 2 * I, H)) / 16.0, True).view(np.int16)).view(torch.bfloat16)
    w2 = torch.from_numpy(to_bits(rng.standard_normal((E, H, I)) / 16.0, True).view(np.int16)).view(torch.bfloat16)
    hidden = torch.from_numpy(rng.standard_normal((T, H), dtype=np.float32)).bfloat16().cuda()
    ids = torch.from_numpy(np.stack([rng.choice(E, topk, replace=False) for _ in range(T)])).cuda()
    wts = torch.softmax(torch.from_numpy(rng.standard_normal((T, topk), dtype=np.float32)), -1).cuda()
    cpu_q = offline.quantize_nvfp4_cpu if fmt == "nvfp4" else offline.quantize_mxfp4_cpu
    ref_args = [t.cuda() for t in cpu_q(w13) + cpu_q(w2)]
    ref = pk.fp4_moe_fused(hidden, *ref_args, wts, ids, fmt)
    for layer in _layers():
        dev_q = layer.quantize_nvfp4 if fmt == "nvfp4" else layer.quantize_mxfp4
        got = pk.fp4_moe_fused(hidden, *dev_q(w13.cuda()), *dev_q(w2.cuda()), wts, ids, fmt)
        assert torch.isfinite(got.float()).all() and got.float().abs().max() > 0
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["nvfp4", "mxfp4"])
def test_capturable_and_deterministic(fmt):
    """One quantise call in a graph, replayed after w was overwritten in place, gives the new weights' bits; a repeated launch is bit-identical."""
    import petit_kernel as pk
    E, n, k = 2, 32, 1024
    first, second = random_bits(E, n, k, True, 1), random_bits(E, n, k, True, 2)
    w = torch.from_numpy(first.view(np.int16)).cuda().view(torch.bfloat16)
    quant = pk.quantize_nvfp4 if fmt == "nvfp4" else pk.quantize_mxfp4
    eager = quant(w)
    again = quant(w)
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(eager, again))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        quant(w)                                    # warm-up on the capturing stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = quant(w)
    w.copy_(torch.from_numpy(second.view(np.int16)).cuda().view(torch.bfloat16))
    graph.replay()
    torch.cuda.synchronize()
    _, _, hgs, hpw, hps = host_twin(second, True, fmt)
    assert np.array_equal(out[0].cpu().numpy().view(np.uint32).reshape(-1), hpw)
    assert np.array_equal(out[1].view(torch.uint8).cpu().numpy().reshape(-1), hps)
    assert np.array_equal(out[2].cpu().numpy().view(np.uint32), hgs.view(np.uint32))

"""The weight quantiser under method = "search" (include/petit_amd.h "Weight quantiser", "The search"): per block the better, by squared error,
of the amax rule's scale byte and one second candidate.  The device is held to the host twin bit for bit; the twin to the properties the rule
promises (never worse than the amax rule, bytes only where allowed) and to blocks whose answer is known."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import cdna4_layout as LY
from test_quantize_weights import BF16, FP16, FP4, MXFP4, NVFP4, SHAPES, _lib, e4m3_rne_sat, e4m3_value, magnitudes, random_bits, to_bits

ABSMAX, SEARCH = 0, 1
gpu = pytest.mark.gpu


def gaussian_bits(E, n, k, bf16, seed):
    """Gaussian weights (sigma = 0.02) with a few blocks of zeros and a few outlier elements."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((E, n, k)).astype(np.float32) * 0.02
    w[:, n // 2, 32:64], w[:, 0, k - 16:] = 0, 0
    w[:, rng.integers(0, n, 6), rng.integers(0, k, 6)] *= 30.0
    return to_bits(w, bf16)


def quantize(bits, bf16, fmt, method, gs=None, device=False):
    """petit_quantize_weights_ex_host / _ex on [E, n, k] 16-bit patterns -> (packed weights u32, packed scale bytes u8, gs f32) as numpy arrays."""
    L, (E, n, k), dev = _lib(), bits.shape, "cuda" if device else "cpu"
    g, a_type, b_type = (16 if fmt == "nvfp4" else 32), (BF16 if bf16 else FP16), (NVFP4 if fmt == "nvfp4" else MXFP4)
    w = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev)
    pw, ps = torch.zeros(E * n * k // 8, dtype=torch.int32, device=dev), torch.zeros(E * n * k // g, dtype=torch.uint8, device=dev)
    out_gs = torch.zeros(E, dtype=torch.float32, device=dev)
    gs_in = None if gs is None else torch.tensor(np.asarray(gs, np.float32), device=dev)
    args = (w.data_ptr(), a_type, b_type, method, E, n, k, None if gs is None else gs_in.data_ptr(), pw.data_ptr(), ps.data_ptr(), out_gs.data_ptr())
    if device:
        ws_bytes = int(L.lib.petit_quantize_weights_workspace_bytes(b_type, E, int(gs is not None)))
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
        rc = L.lib.petit_quantize_weights_ex(*args, ws.data_ptr() if ws_bytes else None, ws_bytes, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    else:
        rc = L.lib.petit_quantize_weights_ex_host(*args)
    assert rc == 0, L.error_string(rc)
    return pw.cpu().numpy().view(np.uint32), ps.cpu().numpy(), out_gs.cpu().numpy()


def unpacked(out, rows, k, fmt):
    """a quantize() result -> (float32 dequantised [rows, k] with one rounding, at the global scale; scale bytes [rows, k / g]; codes [rows, k])."""
    (pw, ps, gs), g = out, 16 if fmt == "nvfp4" else 32
    q = LY.unpack_weights(pw, rows, k).view(np.uint8).reshape(rows, k // 2)
    codes = np.empty((rows, k), np.uint8)
    codes[:, 0::2], codes[:, 1::2] = q & 15, q >> 4
    sb = (LY.unpack_nvscales if fmt == "nvfp4" else LY.unpack_mxscales)(ps, rows, k).reshape(rows, k // g)
    s = e4m3_value(sb) if fmt == "nvfp4" else np.exp2(sb.astype(np.float64) - 127.0)
    v = FP4[codes & 7] * np.where(codes & 8, -1.0, 1.0)
    dq = (v.reshape(rows, -1, g) * s[:, :, None]).reshape(rows, k).astype(np.float32)     # (exact in f32)
    return dq * np.repeat(gs, rows // len(gs))[:, None].astype(np.float32), sb, codes


@gpu
@pytest.mark.parametrize("mode", ["nvfp4", "nvfp4_gs", "mxfp4"])
@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("E,n,k", [(1, n, k) for n, k in SHAPES] + [(3, 48, 512)])
def test_device_equals_host_twin(E, n, k, bf16, mode):
    bits = gaussian_bits(E, n, k, bf16, n + k)
    gs = np.full(E, 2.0 ** -10, np.float32) if mode == "nvfp4_gs" else None
    dev, host = quantize(bits, bf16, mode[:5], SEARCH, gs, device=True), quantize(bits, bf16, mode[:5], SEARCH, gs)
    for name, d, h in zip(("packed weights", "packed scales", "gs"), dev, host):
        assert d.tobytes() == h.tobytes(), f"{mode} {E}x{n}x{k}: {name} differ in {int((d != h).sum())} of {d.size} places"
    assert not np.array_equal(host[1], quantize(bits, bf16, mode[:5], ABSMAX, gs)[1]), "the search changed no scale byte"


@pytest.mark.parametrize("fmt", ["nvfp4", "mxfp4"])
@pytest.mark.parametrize("where,bf16", [("host", True), ("host", False), pytest.param("device", True, marks=gpu)])
def test_search_never_loses_to_the_amax_rule(where, bf16, fmt):
    """Per block, in float64 on the float32 dequantised tensors: err_search <= err_absmax (1 + 2^-16) -- the margin covers the f32 rounding of
    the kernel's own sums, under 40 x 2^-24 per side --; some block is strictly better; a scale byte is one of the block's two candidates."""
    (E, n, k, g), bits = (2, 64, 1024, 16 if fmt == "nvfp4" else 32), gaussian_bits(2, 64, 1024, bf16, 7)
    bits[1] = to_bits(magnitudes(bits[1], bf16) * np.where(bits[1] >> 15, -64.0, 64.0), bf16)     # experts of different size
    a = magnitudes(bits, bf16).reshape(E * n, k)
    w64 = np.where(bits.reshape(E * n, k) >> 15, -1.0, 1.0) * a.astype(np.float64)
    outs = [quantize(bits, bf16, fmt, m, device=where == "device") for m in (ABSMAX, SEARCH)]
    (dq0, sb0, _), (dq1, sb1, _) = [unpacked(o, E * n, k, fmt) for o in outs]
    if where == "device":   # the dequantised tensors are dequant_packed's there
        import petit_kernel as pk
        for (pw, ps, gs), dq in zip(outs, (dq0, dq1)):
            s = torch.from_numpy(ps).cuda()
            s = s.view(torch.float8_e4m3fn).view(E * n, k // 16) if fmt == "nvfp4" else s.view(E * n // 32, k)
            dev = pk.ops.dequant_packed(torch.from_numpy(pw.view(np.int32)).cuda().view(E * n // 16, 2 * k), s, E * n, k, fmt).cpu().numpy()
            assert np.array_equal(dev * np.repeat(gs, n)[:, None], dq)
    err0, err1 = [((w64 - dq.astype(np.float64)) ** 2).reshape(E * n, k // g, g).sum(-1) for dq in (dq0, dq1)]
    print(f"{fmt} {where}: {(err1 < err0).mean():.1%} of blocks strictly better, squared error x {err1.sum() / err0.sum():.4f}")
    assert (err1 <= err0 * (1 + 2.0 ** -16)).all() and (err1 < err0).sum() > 0, f"{int((err1 > err0 * (1 + 2.0 ** -16)).sum())} blocks lose"
    amax = a.reshape(E * n, k // g, g).max(-1)
    if fmt == "nvfp4":
        gs = np.repeat(outs[0][2], n)[:, None]
        with np.errstate(over="ignore"):
            b0, b1 = e4m3_rne_sat((amax / np.float32(6.0)) / gs), e4m3_rne_sat((amax / np.float32(4.0)) / gs)
        assert np.array_equal(outs[0][2].view(np.uint32), outs[1][2].view(np.uint32)), "the global scale is not searched"
    else:
        b0, b1 = sb0, np.maximum(sb0.astype(np.int32) - 1, 1)
    assert np.array_equal(sb0, b0) and ((sb1 == b0) | (sb1 == b1)).all()


@pytest.mark.parametrize("device", [False, pytest.param(True, marks=gpu)])
def test_blocks_with_a_known_answer(device):
    bf16 = True
    # NVFP4, supplied gs = 1, row 0: {+-4, +-2, +-1, +-0.5, 0} -- the amax rule's byte 0.6875 misses every element, 1.0 reproduces the block --;
    # a block the amax rule gets exactly (+-3 = 6 x 0.5, 0: the tie keeps b0); a zero block
    w = np.zeros((16, 256), np.float32)
    w[0, :16] = [4, -4, 2, -2, 1, -1, .5, -.5, 0, 0, 4, 2, 1, .5, -1, -2]
    w[0, 16:32] = [3, -3, 0, 3] * 4
    bits = to_bits(w, bf16)[None]
    out0, out1 = [unpacked(quantize(bits, bf16, "nvfp4", m, [1.0], device), 16, 256, "nvfp4") for m in (ABSMAX, SEARCH)]
    assert out0[1][0, 0] == e4m3_rne_sat(np.float32([0.6875]))[0] and (out0[0][0, :16] != w[0, :16])[w[0, :16] != 0].all()
    assert out1[1][0, 0] == e4m3_rne_sat(np.float32([1.0]))[0] and np.array_equal(out1[0][0, :16], w[0, :16])
    assert out1[1][0, 1] == out0[1][0, 1] == e4m3_rne_sat(np.float32([0.5]))[0] and np.array_equal(out1[0][0, 16:32], w[0, 16:32])
    assert (out1[1][0, 2:] == 0).all() and not out1[2][0, 32:].any()
    # MXFP4, row 0: one 7 among elements on the 0.5 grid up to 3 (b0 = 128: step 1; b0 - 1 loses 1 on the 7 and a quarter on each 2.5);
    # all +-6 x 2^-3 or 0 (exact: b0); a zero block (byte 1); a block whose b0 is already the smallest byte, 1 (b0 - 1 clamps to it)
    w = np.zeros((16, 256), np.float32)
    w[0, :32] = [7] + [0.5, -1.5, 2.5, -3.0, 1.0, 0.0, -0.5, 2.0] * 3 + [1.5] * 7
    w[0, 32:64] = [0.75, -0.75, 0, 0.75] * 8
    w[0, 96:128] = [2.0 ** -126, -(2.0 ** -126), 0, 2.0 ** -125] * 8
    bits = to_bits(w, bf16)[None]
    out0, out1 = [unpacked(quantize(bits, bf16, "mxfp4", m, None, device), 16, 256, "mxfp4") for m in (ABSMAX, SEARCH)]
    assert out0[1][0, :4].tolist() == [128, 124, 1, 1] and out1[1][0, :4].tolist() == [127, 124, 1, 1]
    want = w[0, :32].copy()
    want[0], want[np.abs(want) == 2.5] = 6.0, 2.0          # (7 saturates; 2.5 is the tie between 2 and 3: the even code, 2)
    assert np.array_equal(out1[0][0, :32], want)
    assert np.array_equal(out1[2][0, 32:], out0[2][0, 32:]) and np.array_equal(out1[0][0, 32:64], w[0, 32:64])


@gpu
@pytest.mark.parametrize("fmt", ["nvfp4", "mxfp4"])
def test_gemm_on_the_search_output(fmt):
    """mul_*_a16 at M = 8 on quantize_*(w, method="search") of both layers against float64 on the dequantised tensors, under the bound of
    test_quantize_weights.test_gemm_on_the_quantisers_output."""
    import petit_kernel as pk
    import quantize_weights as QW      # (tools/, on the path since test_quantize_weights was imported)
    m, n, k = 8, 64, 1024
    bits = random_bits(1, n, k, True, 21) if fmt == "mxfp4" else to_bits(QW.synthetic_weights(n, k, 21) * 40.0, True)[None]
    w = torch.from_numpy(bits[0].view(np.int16)).cuda().view(torch.bfloat16)
    a = torch.from_numpy(np.random.default_rng(2).standard_normal((m, k), dtype=np.float32)).bfloat16()
    for layer in (pk.ops, pk.compiled):
        b, s, g = layer.quantize_nvfp4(w, method="search") if fmt == "nvfp4" else layer.quantize_mxfp4(w, method="search")
        dq = pk.ops.dequant_packed(b, s, n, k, fmt).double().cpu().numpy() * float(g.item())
        ref = a.double().numpy() @ dq.T
        got = (layer.mul_nvfp4_a16 if fmt == "nvfp4" else layer.mul_mxfp4_a16)(a.cuda(), b, s, g, m, n, k, -1).double().cpu().numpy()
        err = np.abs(got - ref)
        print(f"{fmt}: max err {err.max():.4g}, max |ref| {np.abs(ref).max():.4g}")
        assert (err <= np.maximum(1e-2, 1e-2 * np.abs(ref))).all(), f"max err {err.max()}"
        host = quantize(bits, True, fmt, SEARCH)
        assert np.array_equal(b.cpu().numpy().view(np.uint32).reshape(-1), host[0]) and np.array_equal(s.view(torch.uint8).cpu().numpy().reshape(-1), host[1])


def test_refusals_and_the_default():
    import petit_kernel as pk
    from petit_kernel import offline
    L = _lib()
    buf = np.zeros(1 << 16, np.uint8)
    ptr = C.c_void_p((buf.ctypes.data + 255) & ~255)
    for method in (2, -1):
        assert L.lib.petit_quantize_weights_ex_host(ptr, BF16, NVFP4, method, 1, 16, 256, None, ptr, ptr, ptr) == L.PETIT_ERROR_BAD_ARGUMENT
        assert L.lib.petit_quantize_weights_ex(ptr, BF16, MXFP4, method, 1, 16, 256, None, ptr, ptr, ptr, None, 0, None) == L.PETIT_ERROR_BAD_ARGUMENT
    w = torch.from_numpy(gaussian_bits(1, 32, 512, True, 3)[0].view(np.int16)).view(torch.bfloat16)
    for fn in (offline.quantize_nvfp4_cpu, offline.quantize_mxfp4_cpu, pk.quantize_nvfp4, pk.ops.quantize_mxfp4, pk.compiled.quantize_nvfp4):
        for bad in ("best", 1, None):
            with pytest.raises(RuntimeError, match="method must be 'absmax' or 'search'"):
                fn(w, method=bad)
    for fn in (offline.quantize_nvfp4_cpu, offline.quantize_mxfp4_cpu):
        plain, named, search = fn(w), fn(w, method="absmax"), fn(w, method="search")
        assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(plain, named))
        assert not torch.equal(plain[1].view(torch.uint8), search[1].view(torch.uint8))

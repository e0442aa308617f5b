"""The block-Hadamard rotation inside the quantising gated epilogue (include/petit_amd.h "out_block"; out_hadamard= of the native entries)."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gpu_parity import DEV, NATIVE_SENTINEL, _mx_problem_on_device, decode_qact, from_bits, pk, random_problem  # noqa: F401 (pk: fixture)
from test_hadamard_quant import sylvester
from test_moe import _hints, _routing
from test_moe_native import FMTS, SENTINEL, NativeExperts, _offsets_dev, _rows_of, _u8

pytestmark = pytest.mark.gpu
BLOCKS = (32, 128)
ROT_FMTS = ("mxfp8", "mxfp4")


def _device_weights(pk, q, s, n, k):
    return (pk.repack_mxfp4(torch.from_numpy(q).to(DEV).view(torch.int32), n, k), pk.process_mxfp4_scales(torch.from_numpy(s).to(DEV), n, k))


@pytest.mark.parametrize("m,n,k", [(5, 512, 256), (130, 1024, 256), (128, 512, 512)])
@pytest.mark.parametrize("fmt", ROT_FMTS)
@pytest.mark.parametrize("B", BLOCKS)
def test_every_hadamard_row_is_transformed_exactly(pk, B, fmt, m, n, k):
    """Per block of B output columns: one gate row, and up row c = the base up row with its FP4 signs flipped where H_B[r][c] = -1,
    r = (37 block + 5) % B.  The gated values are exactly H_B[r][c] v, every stage gives 0 or +-2^s v, z is B v at r and 0 elsewhere: the
    rotated call decodes to B times the unrotated column 0 (H_B[r][0] = 1) at r, 0 elsewhere, and the scale byte moves by log2 B."""
    a_bits, q, s, _ = random_problem("mx", m, n, k, 8100 + m + n + k + B, True)
    s[:] = np.random.default_rng(B + n).integers(118, 124, s.shape, dtype=np.uint8)   # products of 2^-9 .. 2^-4: scale bytes far from 1 and 254
    H, half = sylvester(B), n // 2
    rows = [(37 * blk + 5) % B for blk in range(half // B)]
    for blk, r in enumerate(rows):
        j0 = blk * B
        q[j0:j0 + B], s[j0:j0 + B] = q[j0], s[j0]
        flip = np.where(H[r] < 0, 0x88, 0).astype(np.uint8)[:, None]
        q[half + j0:half + j0 + B], s[half + j0:half + j0 + B] = q[half + j0] ^ flip, s[half + j0]
    a = from_bits(a_bits, torch.bfloat16).to(DEV)
    b, sp = _device_weights(pk, q, s, n, k)
    gsd = torch.ones(1, dtype=torch.float32, device=DEV)
    sid = NATIVE_SENTINEL(pk, fmt)
    unrot = pk.mul_mxfp4_native(a, b, sp, gsd, m, n, k, sid, activation="silu_mul", out_quantized=fmt, out_hadamard=0)
    rot = pk.mul_mxfp4_native(a, b, sp, gsd, m, n, k, sid, activation="silu_mul", out_quantized=fmt, out_hadamard=B)
    raw0 = _u8(unrot.data)
    sc0 = raw0[m * half // 8 * FMTS[fmt]:]
    assert sc0.min() >= 1 and sc0.max() + int(np.log2(B)) <= 254, (sc0.min(), sc0.max())
    deq0, deq = decode_qact(raw0, m, half, fmt), decode_qact(_u8(rot.data), m, half, fmt)
    want = np.zeros_like(deq0)
    for blk, r in enumerate(rows):
        assert (np.abs(deq0[:, blk * B:(blk + 1) * B]) == np.abs(deq0[:, blk * B:blk * B + 1])).all()   # the premise: one |v| per block
        want[:, blk * B + r] = B * deq0[:, blk * B]
    sc = _u8(rot.data)[m * half // 8 * FMTS[fmt]:].reshape(-1, m, 4)           # [k-tile][row][32-column block]
    for blk, r in enumerate(rows):                                             # the block that holds position r: the unrotated byte + log2 B
        c = blk * B + r
        got_b, want_b = sc[c // 128, :, c % 128 // 32], sc0.reshape(-1, m, 4)[c // 128, :, c % 128 // 32] + int(np.log2(B))
        assert (got_b == np.where(deq0[:, blk * B] == 0, 127, want_b)).all(), (blk, r)   # (v = 0: a zero block keeps byte 127)
    bad = np.argwhere(deq != want)
    assert bad.size == 0, f"{len(bad)} elements differ; first {bad[0]}: got {deq[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}"


@pytest.mark.parametrize("activation", ["silu_mul", "swiglu_oai"])
@pytest.mark.parametrize("m,n,k,with_bias", [(64, 512, 1024, False), (130, 1024, 512, True)])
@pytest.mark.parametrize("fmt", ROT_FMTS)
@pytest.mark.parametrize("B", BLOCKS)
def test_rotated_output_against_float64_rotation_of_the_16_bit_result(pk, B, fmt, m, n, k, with_bias, activation):
    """test_quantized_silu_mul_output_feeds_the_next_gemm's method and per-element bound: ref = H_B in float64 on the 16-bit result c16 of
    the same call without out_quantized, `step` from ref's block maximum.  Its 2^-7 |ref| slack becomes 2^-8 sum |c16| over the rotation
    block (B bf16 roundings through +-1 sums) plus the kernel's log2(B) f32 stages on partial sums <= sum |v|: <= 2^-20 sum |c16|."""
    _, _, _, _, a, b, sp, gsd = _mx_problem_on_device(pk, m, n, k, 7300 + m + n + k)
    bias = (torch.randn(n, device=DEV) * 0.5).bfloat16() if with_bias else None
    sid = NATIVE_SENTINEL(pk, fmt)
    c16 = pk.mul_mxfp4_native(a, b, sp, gsd, m, n, k, sid, bias=bias, activation=activation).float().cpu().numpy().astype(np.float64)
    rot = pk.mul_mxfp4_native(a, b, sp, gsd, m, n, k, sid, bias=bias, activation=activation, out_quantized=fmt, out_hadamard=B)
    deq = decode_qact(_u8(rot.data), m, n // 2, fmt)
    ref = (c16.reshape(m, -1, B) @ sylvester(B)).reshape(m, -1)
    slack = np.repeat((2.0 ** -8 + 2.0 ** -20) * np.abs(c16).reshape(m, -1, B).sum(axis=2), B, axis=1)
    blk = np.abs(ref).reshape(m, -1, 32).max(axis=2)
    step = np.repeat(np.exp2(np.floor(np.log2(np.maximum(blk, 1e-30)))), 32, axis=1)
    err = np.abs(deq - ref)
    bound = 0.5 * step + slack if fmt == "mxfp4" else 2.0 ** -4 * np.abs(ref) + 2.0 ** -9 * step + slack
    assert (err <= bound).all(), (err / bound).max()


@pytest.mark.parametrize("fmt", ROT_FMTS)
@pytest.mark.parametrize("B", BLOCKS)
def test_rotated_hand_over_feeds_a_rotated_down(pk, B, fmt):
    """down on quantize_mxfp4(w2, hadamard=B): the fused rotated hand-over against quantize_activations(c16, fmt, hadamard=B) (the unrotated
    test's constants), and against the float64 MLP on dequant(quantize_mxfp4(w2, hadamard=B)) . H_B (test_mlp_block_accuracy_budget's budgets):
    the rotation cancels.  NOT the separately quantised unrotated w2, another MXFP4 rounding (~10 % per weight) that no kernel brings under
    8 %: test_fp4_moe_native_rotated_layer compares the two pipelines on separately quantised weights, with a bound that allows for it."""
    m, n, k, n2 = 64, 1024, 512, 256
    _, q, s, _ = random_problem("mx", m, n, k, 7400 + B, True, mx_band=(122, 127))
    gs = 0.05
    x = torch.randn(m, k, device=DEV).bfloat16()
    b, sp = _device_weights(pk, q, s, n, k)
    gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
    w2 = (torch.randn(n2, n // 2, device=DEV) * 0.05).bfloat16()
    b2r, s2r, g2r = pk.quantize_mxfp4(w2, hadamard=B)
    sid = NATIVE_SENTINEL(pk, fmt)
    c16 = pk.mul_mxfp4_native(x, b, sp, gsd, m, n, k, sid, activation="silu_mul")
    hq = pk.mul_mxfp4_native(x, b, sp, gsd, m, n, k, sid, activation="silu_mul", out_quantized=fmt, out_hadamard=B)
    y_fused = pk.mul_mxfp4_native(hq, b2r, s2r, g2r, m, n2, n // 2, sid).float()
    y_chain = pk.mul_mxfp4_native(pk.quantize_activations(c16, fmt, hadamard=B), b2r, s2r, g2r, m, n2, n // 2, sid).float()
    diff = (y_fused - y_chain).pow(2).mean().sqrt().item() / y_chain.pow(2).mean().sqrt().item()
    assert diff <= {"mxfp4": 0.08, "mxfp8": 0.02}[fmt], diff
    # ((x H) . Wr^T = x . (Wr H)^T, H symmetric)
    dq2 = pk.ops.dequant_packed(b2r, s2r, n2, n // 2, "mxfp4", global_scale=float(g2r.item())).cpu().numpy().astype(np.float64)
    dq2 = (dq2.reshape(n2, -1, B) @ sylvester(B)).reshape(n2, -1)
    y1 = x.float().cpu().numpy().astype(np.float64) @ O.dequant_mxfp4(q, s).astype(np.float64).T * gs
    ref = (y1[:, :n // 2] / (1.0 + np.exp(-y1[:, :n // 2])) * y1[:, n // 2:]) @ dq2.T
    rel = np.sqrt(np.mean((y_fused.cpu().numpy() - ref) ** 2) / np.mean(ref ** 2))
    assert rel <= {"mxfp4": 0.45, "mxfp8": 8e-2}[fmt], rel


@pytest.mark.parametrize("kind,fmt", [("mx", "mxfp8"), ("mx", "mxfp4"), ("nv", "mxfp4")])
@pytest.mark.parametrize("B", BLOCKS)
def test_moe_rotated_rows_equal_the_dense_call_per_expert(pk, B, kind, fmt):
    E, n, k, counts, m = 3, 512, 256, [37, 0, 93], 130
    ne = NativeExperts(pk, kind, E, n, k, 51)
    a = torch.randn(m, k, device=DEV).bfloat16()
    sid = pk.native_moe_resolve_solution(_hints(pk, kind, True), E, m, n, k, SENTINEL[fmt], activation="silu_mul", out_quantized=fmt)
    got = ne.moe(pk, a, _offsets_dev(counts), m, sid, activation="silu_mul", out_quantized=fmt, out_hadamard=B)
    rows = _rows_of(got.data, m, n // 2, FMTS[fmt])
    o = np.concatenate([[0], np.cumsum(counts)])
    for e in range(E):
        if counts[e]:
            ref = ne.dense(pk, a[o[e]:o[e + 1]].contiguous(), e, sid, activation="silu_mul", out_quantized=fmt, out_hadamard=B)
            assert np.array_equal(rows[o[e]:o[e + 1]], _rows_of(ref.data, counts[e], n // 2, FMTS[fmt])), f"expert {e}"


def test_refusals_and_block_zero(pk):
    m, n, k = 5, 512, 256
    _, _, _, _, a, b, sp, gsd = _mx_problem_on_device(pk, m, n, k, 7500)
    call = lambda fmt, **kw: pk.mul_mxfp4_native(a, b, sp, gsd, m, n, k, NATIVE_SENTINEL(pk, fmt), activation="silu_mul", **kw)  # noqa: E731
    with pytest.raises(RuntimeError, match="MXFP6"):
        call("mxfp6", out_quantized="mxfp6", out_hadamard=32)
    with pytest.raises(RuntimeError, match="32 or 128"):
        call("mxfp4", out_quantized="mxfp4", out_hadamard=64)
    with pytest.raises(RuntimeError, match="out_quantized"):
        call("mxfp4", out_hadamard=32)
    for fmt in ROT_FMTS:
        assert torch.equal(call(fmt, out_quantized=fmt, out_hadamard=0).data, call(fmt, out_quantized=fmt).data)
    # the C ABI's own refusals (the Python layer makes them first): codes, before any launch (C keeps its fill), and the queries answer 0
    import ctypes as C
    from petit_kernel import _lib
    L, kern, bad = _lib.lib, _lib.PETIT_ERROR_KERNEL_SHAPE, _lib.PETIT_ERROR_BAD_ARGUMENT
    hints, epi = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_MXFP4_E2M1, _lib.CXX_DTYPE_BF16, 0), _lib.Epilogue(None, 1, 0)
    pk.ops.enable_native_fp4(True)
    try:
        fp6_id = next(x for x in pk.ops.get_fp4_solutions(_hints(pk, "mx"), m, n, k) if (x >> 48) & 0xF == 13 and (x >> 32) & 7 == 4 and (x >> 52) & 0xF == 4)
    finally:
        pk.ops.enable_native_fp4(False)
    out = torch.full((int(L.petit_quantized_activation_bytes(m, n // 2, 8)),), 0xA5, dtype=torch.uint8, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    s4, s6 = _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP4, _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP6
    for out_fmt, block, sid, want in ((6, 32, s6, kern), (4, 64, s4, bad), (0, 32, s4, bad), (4, 32, s6, kern), (4, 128, fp6_id, kern)):
        na = _lib.NativeArgs(C.sizeof(_lib.NativeArgs), 0, out_fmt, block)
        rc = L.petit_gemm_mxfp4_native(out.data_ptr(), a.data_ptr(), b.data_ptr(), sp.data_ptr(), gsd.data_ptr(), m, n, k, C.byref(hints),
                                       C.c_uint64(sid), C.byref(epi), C.byref(na), ws.data_ptr(), C.c_uint64(ws.numel()), None)
        assert rc == want, (out_fmt, block, hex(sid), rc)
        assert L.petit_gemm_native_workspace_bytes(C.byref(hints), m, n, k, C.c_uint64(sid), C.byref(epi), C.byref(na)) == 0
        assert L.petit_gemm_native_moe_resolve_solution(C.byref(hints), 3, m, n, k, C.c_uint64(sid), C.byref(epi), C.byref(na)) == 0
    assert (out == 0xA5).all()


@pytest.mark.parametrize("B", BLOCKS)
def test_fp4_moe_native_rotated_layer(pk, B):
    """fp4_moe_native(hadamard=B) on quantize_mxfp4(w, hadamard=B) experts against the unrotated layer on quantize_mxfp4(w): two MXFP4
    roundings of the same weights (~10 % per weight and GEMM, independent: <= 0.3 between the outputs; a rotation that did not cancel: ~1.4)."""
    E, T, H, I = 4, 24, 512, 256
    g = torch.Generator(device=DEV).manual_seed(B)
    w13, w2 = (torch.randn(E, 2 * I, H, device=DEV, generator=g) * 0.05).bfloat16(), (torch.randn(E, H, I, device=DEV, generator=g) * 0.05).bfloat16()
    x, nw = torch.randn(T, H, device=DEV, generator=g).bfloat16(), torch.ones(H, device=DEV).bfloat16()
    tw, ids = (t.to(DEV) for t in _routing(T, E, 2, B))
    run = lambda had, **kw: pk.fp4_moe_native(x, *pk.quantize_mxfp4(w13, hadamard=had), *pk.quantize_mxfp4(w2, hadamard=had), tw, ids, "mxfp4",  # noqa: E731
                                              "mxfp8", hadamard=had, **kw)
    y0, y = run(0).float(), run(B).float()
    assert ((y - y0).pow(2).mean().sqrt() / y0.pow(2).mean().sqrt()).item() <= 0.3
    (h, y16), (q, h2) = run(B, norm_weight=nw), run(B, norm_weight=nw, norm_fmt="mxfp8", norm_hadamard=B)
    assert q.hadamard == B and torch.equal(h, h2) and torch.equal(q.data, pk.quantize_activations(y16, "mxfp8", hadamard=B).data)
    with pytest.raises(RuntimeError, match="invariant"):
        run(B, invariant=True)

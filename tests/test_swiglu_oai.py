"""activation="swiglu_oai" (PETIT_ACTIVATION_SWIGLU_OAI = 2), the gated epilogue of gpt-oss: with y = acc * gs + bias,
g = min(y_gate, 7), u = clamp(y_up, -7, 7), c = round16(g * sigmoid(1.702 g) * (u + 1)).  It shares every shape rule, pick and refusal with
"silu_mul"; only the epilogue arithmetic differs.  The oracle yields the plain product y; the activation is applied to it here in float64.

Bound of the dense GPU test: test_fused_silu_mul_epilogue's |c - ref| <= max(1e-2, 2e-2 |ref|) -- two f32 factors rounded once, and the
clamps are 1-Lipschitz, so an error of y passes through them no larger than it came.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gpu_parity import (NATIVE_SENTINEL, _mx_problem_on_device, bits, check_gemm, decode_qact, from_bits, oracle_ref, random_problem,
                             to_f32)
from test_moe import Experts, _hints, _offsets
from test_moe_native import ROUTINGS, SENTINEL, NativeExperts, _offsets_dev

DEV = "cuda"
ALPHA, LIMIT = 1.702, 7.0


def swiglu_oai_np(y):
    """float64 [m, n] -> [m, n / 2]: the activation on the [gate; up] halves."""
    h = y.shape[1] // 2
    g = np.minimum(y[:, :h], LIMIT)
    u = np.clip(y[:, h:], -LIMIT, LIMIT)
    with np.errstate(over="ignore"):
        return g / (1.0 + np.exp(-ALPHA * g)) * (u + 1.0)


# --- without a GPU ----------------------------------------------------------------------------------------------------------------

def _aligned(buf, align=256):
    return C.c_void_p((C.addressof(buf) + align - 1) & ~(align - 1))


def test_abi_activation_2_answers_as_1_and_3_is_refused():
    from petit_kernel import _lib
    L = _lib.lib
    assert _lib.PETIT_OK == 0
    bad, shape = _lib.PETIT_ERROR_BAD_ARGUMENT, _lib.PETIT_ERROR_PROBLEM_SHAPE
    silu, oai, three = _lib.Epilogue(None, 1, 0), _lib.Epilogue(None, 2, 0), _lib.Epilogue(None, 3, 0)
    auto = _lib.PETIT_SOLUTION_AUTO
    natives = (_lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP8, _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP6, _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP4)

    def na(a_fmt=0, out_fmt=0):
        return C.byref(_lib.NativeArgs(C.sizeof(_lib.NativeArgs), a_fmt, out_fmt, 0))

    answered = 0
    for b_type in (_lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_MXFP4_E2M1):
        h = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, b_type, _lib.CXX_DTYPE_BF16, 0)
        for m, n, k in ((1, 5760, 3072), (16, 1024, 8192), (300, 6144, 3072), (4096, 2048, 1024), (64, 96, 768)):
            sids = [auto] + (list(natives) if b_type == _lib.CXX_DTYPE_MXFP4_E2M1 else [])
            for sid in sids:
                q = [L.petit_gemm_workspace_bytes_ex(C.byref(h), m, n, k, C.c_uint64(sid), C.byref(e)) for e in (silu, oai)]
                r = [L.petit_gemm_resolve_solution(C.byref(h), m, n, k, C.c_uint64(sid), C.byref(e), C.c_uint64(1 << 34)) for e in (silu, oai)]
                s = [L.petit_gemm_row_split(C.byref(h), m, n, k, C.c_uint64(sid), C.byref(e)) for e in (silu, oai)]
                assert q[0] == q[1] and r[0] == r[1] and s[0] == s[1], (b_type, m, n, k, sid)
                answered += r[0] != 0
                assert L.petit_gemm_workspace_bytes_ex(C.byref(h), m, n, k, C.c_uint64(sid), C.byref(three)) == 0
                assert L.petit_gemm_resolve_solution(C.byref(h), m, n, k, C.c_uint64(sid), C.byref(three), C.c_uint64(1 << 34)) == 0
            for E in (8, 128):
                r = [L.petit_gemm_moe_resolve_solution(C.byref(h), E, m, n, k, C.c_uint64(auto), C.byref(e)) for e in (silu, oai)]
                assert r[0] == r[1] and r[0] != 0, (b_type, E, m, n, k)
                assert L.petit_gemm_moe_resolve_solution(C.byref(h), E, m, n, k, C.c_uint64(auto), C.byref(three)) == 0
                for sid in natives:
                    for nat in (None, na(0, 8) if n % 512 == 0 else None):
                        r = [L.petit_gemm_native_moe_resolve_solution(C.byref(h), E, m, n, k, C.c_uint64(sid), C.byref(e), nat) for e in (silu, oai)]
                        w = [L.petit_gemm_native_moe_workspace_bytes(C.byref(h), E, m, n, k, C.c_uint64(sid), C.byref(e), nat) for e in (silu, oai)]
                        assert r[0] == r[1] and w[0] == w[1] and r[0] != 0, (b_type, E, m, n, k, sid)
                    assert L.petit_gemm_native_moe_resolve_solution(C.byref(h), E, m, n, k, C.c_uint64(sid), C.byref(three), None) == 0
                    assert L.petit_gemm_native_moe_workspace_bytes(C.byref(h), E, m, n, k, C.c_uint64(sid), C.byref(three), None) == 0
    assert answered >= 10

    # the entry points themselves: every call is refused before anything is launched (host scratch for pointers)
    buf = (C.c_uint8 * 8192)()
    p = _aligned(buf)
    mx = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_MXFP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
    nv = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
    s8 = C.c_uint64(natives[0])
    au = C.c_uint64(auto)

    def dense(epi, n=512, hints=nv):
        fn = L.petit_gemm_fp4_fp16_grid_ex if hints is nv else L.petit_gemm_mxfp4_fp16_grid_ex
        return fn(p, p, p, p, p, 4, n, 256, C.byref(hints), au, C.byref(epi), None)

    def dense_ws(epi, hints=nv):
        fn = L.petit_gemm_fp4_fp16_grid_ws if hints is nv else L.petit_gemm_mxfp4_fp16_grid_ws
        return fn(p, p, p, p, p, 4, 512, 256, C.byref(hints), au, C.byref(epi), None, C.c_uint64(0), None)

    def moe(epi, n=512):
        return L.petit_gemm_fp4_fp16_moe(p, p, p, p, p, p, 8, 4, n, 256, C.byref(nv), au, C.byref(epi), None)

    def moe_ex(epi, n=512):
        return L.petit_gemm_fp4_fp16_moe_ex(p, p, p, p, p, p, 8, 4, n, 256, None, 4, None, 4, C.byref(nv), au, C.byref(epi), None)

    def native(epi, n=512, nat=None):
        return L.petit_gemm_mxfp4_native(p, p, p, p, p, 256, n, 256, C.byref(mx), s8, C.byref(epi), nat, p, C.c_uint64(0), None)

    def nv_native(epi):
        return L.petit_gemm_nvfp4_native(p, p, p, p, 256, 512, 256, C.byref(nv), s8, C.byref(epi), None, p, C.c_uint64(0), None)

    def nv_transient(epi):
        return L.petit_gemm_nvfp4_native_transient(p, p, p, p, p, 256, 512, 256, C.byref(nv), s8, C.byref(epi), None, p, C.c_uint64(1 << 30), None)   # (scratch for the image: its absence is refused first)

    def native_moe(epi, n=512, nat=None, c_idx=None):
        return L.petit_gemm_native_moe(p, p, p, p, p, p, 8, 256, n, 256, None, 256, c_idx, 256, C.byref(mx), s8, C.byref(epi), nat, p, C.c_uint64(0), None)

    for call in (dense, dense_ws, moe, moe_ex, native, nv_native, nv_transient, native_moe):
        assert call(three) == bad, call.__name__
    assert dense(three, hints=mx) == bad and dense_ws(three, hints=mx) == bad
    # the SiLU-mul shape refusals, for 1 and for 2 alike
    for epi in (silu, oai):
        assert dense(epi, n=48) == shape and moe(epi, n=48) == shape and moe_ex(epi, n=48) == shape           # n % 32
        assert native(epi, n=768, nat=na(0, 8)) == shape and native_moe(epi, n=256, nat=na(0, 8)) == shape     # out_format: n % 512
        assert native_moe(epi, nat=na(0, 8), c_idx=p) == bad                                                   # out_format is identity-only
    assert native(_lib.Epilogue(None, 0, 0), nat=na(0, 8)) == bad                                              # ... and a gated epilogue's
    assert L.petit_gemm_native_workspace_bytes(C.byref(mx), 256, 1024, 512, s8, C.byref(silu), na(0, 8)) == \
        L.petit_gemm_native_workspace_bytes(C.byref(mx), 256, 1024, 512, s8, C.byref(oai), na(0, 8)) != 0
    assert L.petit_gemm_native_workspace_bytes(C.byref(mx), 256, 1024, 512, s8, C.byref(three), None) == 0
    assert L.petit_gemm_nvfp4_native_transient_workspace_bytes(C.byref(nv), 256, 1024, 512, s8, C.byref(silu), None) == \
        L.petit_gemm_nvfp4_native_transient_workspace_bytes(C.byref(nv), 256, 1024, 512, s8, C.byref(oai), None) != 0


def test_python_queries_accept_swiglu_oai():
    import petit_kernel as pk
    for kind in ("nv", "mx"):
        h = _hints(pk, kind)
        for m, n, k in ((4, 5760, 3072), (512, 6144, 3072)):
            assert pk.moe_resolve_solution(h, 32, m, n, k, -1, "swiglu_oai") == pk.moe_resolve_solution(h, 32, m, n, k, -1, "silu_mul") != 0
            assert pk.ops.resolve_solution(h, m, n, k, -1, "swiglu_oai") == pk.ops.resolve_solution(h, m, n, k, -1, "silu_mul") != 0
            assert pk.ops.auto_row_split(h, m, n, k, "swiglu_oai") == pk.ops.auto_row_split(h, m, n, k, "silu_mul")
            for fmt, sid in SENTINEL.items():
                oq = fmt if n % 512 == 0 else None
                assert pk.native_moe_resolve_solution(h, 32, m, n, k, sid, "swiglu_oai", out_quantized=oq) == \
                    pk.native_moe_resolve_solution(h, 32, m, n, k, sid, "silu_mul", out_quantized=oq) != 0
    assert pk.nvfp4_native_transient_workspace_bytes(256, 1024, 512, -2, activation="swiglu_oai", out_quantized="mxfp8") == \
        pk.nvfp4_native_transient_workspace_bytes(256, 1024, 512, -2, activation="silu_mul", out_quantized="mxfp8") != 0
    with pytest.raises((RuntimeError, KeyError)):
        pk.ops.resolve_solution(_hints(pk, "nv"), 4, 512, 512, -1, "gelu")


def test_torch_ops_meta_shapes_with_activation_2():
    import petit_kernel  # noqa: F401
    from petit_kernel import compiled
    assert compiled.available(), compiled.why_unavailable()
    ops = torch.ops.petit_kernel
    E, n, k, m = 8, 1024, 512, 12
    a = torch.empty(m, k, dtype=torch.bfloat16, device="meta")
    b = torch.empty(n * k // 2, dtype=torch.uint8, device="meta")
    s = torch.empty(n * k // 32, dtype=torch.uint8, device="meta")
    gs1 = torch.empty(1, dtype=torch.float32, device="meta")
    be = torch.empty(E * n * k // 2, dtype=torch.uint8, device="meta")
    se = torch.empty(E * n * k // 32, dtype=torch.uint8, device="meta")
    gs = torch.empty(E, dtype=torch.float32, device="meta")
    off = torch.empty(E + 1, dtype=torch.int32, device="meta")
    idx = torch.empty(m, dtype=torch.int32, device="meta")
    for act, cols in ((0, n), (1, n // 2), (2, n // 2)):
        assert ops.mul_mxfp4_a16(a, b, s, gs1, m, n, k, -1, None, act).shape == (m, cols)
        assert ops.mul_nvfp4_a16(a.half(), b, s, gs1, m, n, k, -1, None, act).shape == (m, cols)
        assert ops.mul_mxfp4_a16_moe(a, be, se, gs, off, m, n, k, E, -1, None, act).shape == (m, cols)
        assert ops.mul_nvfp4_a16_moe_indexed(a, be, se, gs, off, m, n, k, E, idx, None, -1, -1, None, act).shape == (m, cols)
        assert ops.mul_mxfp4_a16_moe_indexed(a, be, se, gs, off, m, n, k, E, None, idx, 40, -1, None, act).shape == (40, cols)
        c = ops.mul_mxfp4_native_moe(a, be, se, gs, off, m, n, k, E, idx, None, -1, -2, None, act)
        assert c.shape == (m, cols) and c.dtype == torch.bfloat16 and c.device.type == "meta"
    for f, per8 in ((8, 8), (6, 6), (4, 4)):
        want = m * (n // 2 // 8 * per8) + m * (n // 2 // 32)
        for act in (1, 2):
            c = ops.mul_nvfp4_native_moe(a, be, None, gs, off, m, n, k, E, idx, None, -1, -2, None, act, 0, 5, f)
            assert c.shape == (want,) and c.dtype == torch.uint8
            c = ops.mul_nvfp4_native_transient(a, b, s, gs1, m, n, k, -2, None, act, 0, 5, f)
            assert c.shape == (want,) and c.dtype == torch.uint8
        assert ops.mul_nvfp4_native_transient(a, b, s, gs1, m, n, k, -2, None, 2, 0, 5, 0).shape == (m, n // 2)


# --- on the GPU -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pk():
    import petit_kernel
    assert torch.cuda.is_available()
    assert torch.cuda.get_device_properties(0).gcnArchName.startswith("gfx950")
    return petit_kernel


def _clamps_exercised(y):
    """The float64 reference must reach both clamps and still live mostly inside them."""
    h = y.shape[1] // 2
    gate, up = y[:, :h], y[:, h:]
    assert (gate > LIMIT).mean() >= 0.01, (gate > LIMIT).mean()
    assert (np.abs(up) > LIMIT).mean() >= 0.01, (np.abs(up) > LIMIT).mean()
    assert (gate <= LIMIT).mean() >= 0.5 and (np.abs(up) <= LIMIT).mean() >= 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [(1, 256, 2048), (7, 96, 1024), (16, 64, 1024), (40, 128, 3072), (130, 256, 1024), (300, 544, 512)])
@pytest.mark.parametrize("kind,is_bf16,with_bias", [("nv", True, False), ("nv", True, True), ("nv", False, True), ("mx", True, False), ("mx", False, True)])
def test_fused_swiglu_oai_epilogue(pk, kind, is_bf16, with_bias, m, n, k):
    """test_fused_silu_mul_epilogue's grid with activation="swiglu_oai": the default pick and every enumerated id (odd n-tiles per wave and
    the shared kernel refused with the same message), then every id through a 2-way K split (the reduce pass).  The product is scaled so
    that y has a standard deviation of about 3.5: ~2 % of the gates lie above 7, ~4 % of |up| above 7 (asserted on the reference)."""
    dtype = torch.bfloat16 if is_bf16 else torch.float16
    a, q, s, gs = random_problem(kind, m, n, k, 555 + m + n + k, is_bf16, mx_band=(122, 130))
    y = oracle_ref(kind, a, is_bf16, q, s, gs).astype(np.float64)
    scale = 3.5 / y.std()
    y, gs = y * scale, gs * scale
    bias = (torch.randn(n, generator=torch.Generator().manual_seed(n)) * 0.5).to(dtype) if with_bias else None
    if bias is not None:
        y = y + bias.float().numpy().astype(np.float64)[None, :]
    _clamps_exercised(y)
    ref = swiglu_oai_np(y)
    ad, qd = from_bits(a, dtype).to(DEV), torch.from_numpy(q).to(DEV)
    gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
    if kind == "nv":
        b, sp = pk.repack_nvfp4(qd.view(torch.int32), n, k), pk.process_nvfp4_scales(torch.from_numpy(s).to(DEV).view(torch.float8_e4m3fn), n, k)
        mul = pk.mul_nvfp4_a16
    else:
        b, sp = pk.repack_mxfp4(qd.view(torch.int32), n, k), pk.process_mxfp4_scales(torch.from_numpy(s).to(DEV), n, k)
        mul = pk.mul_mxfp4_a16
    bd = bias.to(DEV) if bias is not None else None
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = dtype
    h.b_type = pk.DataType.float4_e2m1 if kind == "nv" else pk.DataType.mxfloat4_e2m1

    def check(c, sid):
        assert c.shape == (m, n // 2) and c.dtype == dtype
        err = np.abs(to_f32(bits(c), is_bf16).astype(np.float64) - ref)
        print(f"sid {sid:#x}: max err {err.max():.4g}, max err / bound {(err / np.maximum(1e-2, 2e-2 * np.abs(ref))).max():.3f}")
        assert (err <= np.maximum(1e-2, 2e-2 * np.abs(ref))).all(), f"sid {sid:#x}: max err {err.max()}"

    served = refused = 0
    for sid in [-1] + list(pk.ops.get_fp4_solutions(h, m, n, k)):
        nt = (sid >> 52) & 0xF if sid >= 0 else 2
        shared = sid >= 0 and (sid >> 48) & 0xF == 12 and (sid >> 36) & 0xF == 5   # gemm_shared.hpp: plain / bias epilogue only
        if nt % 2 or shared:
            with pytest.raises(RuntimeError, match="No kernel implementation"):
                mul(ad, b, sp, gsd, m, n, k, sid, bias=bd, activation="swiglu_oai")
            refused += 1
            continue
        check(mul(ad, b, sp, gsd, m, n, k, sid, bias=bd, activation="swiglu_oai"), sid)
        served += 1
    assert served >= 2
    split_served = 0
    for sid in pk.ops.get_fp4_solutions(h, m, n, k):
        ks = ((sid >> 16) & 0x1F) // 2                        # k-tiles per span: a split needs a span per part
        kind_nib = (sid >> 48) & 0xF
        if kind_nib in (9, 13) or k // (128 * ks) < 2:        # (the native class has its own accuracy bound)
            continue
        if kind_nib == 0 and (sid >> 36) & 0xF == 2 and k // (128 * ks) < 2 * ((sid >> 44) & 0xF):
            continue                                          # (gemm_batch.hpp splits K over its WK in-workgroup parts first)
        sid2 = (sid & ~(0xF << 60)) | (2 << 60)
        try:
            plain = mul(ad, b, sp, gsd, m, n, k, sid2)        # does this kernel take a 2-way split of this K at all?
        except RuntimeError:
            continue
        del plain
        check(mul(ad, b, sp, gsd, m, n, k, sid2, bias=bd, activation="swiglu_oai"), sid2)
        split_served += 1
    assert split_served >= 2 or k < 2048


@pytest.mark.gpu
@pytest.mark.parametrize("kind,is_bf16", [("nv", True), ("mx", False)])
def test_gate_of_minus_1e4_gives_signed_zero(pk, kind, is_bf16):
    """g -> -inf: exp(1.702e4) overflows to inf and g / inf = -0, so the output is -0 or +0 (the sign of -(u + 1)), never NaN.  The weights are
    the code of +1.0 under unit scales, the gate rows get the bias -1e4 (a 16-bit value after rounding); unsplit and through the reduce pass."""
    dtype = torch.bfloat16 if is_bf16 else torch.float16
    m, n, k = 9, 256, 2048
    q = np.full((n, k // 2), 0x22, dtype=np.uint8)            # e2m1 code 2 = +1.0 in both nibbles
    qd = torch.from_numpy(q).to(DEV).view(torch.int32)
    if kind == "nv":
        s = torch.ones(n, k // 16).to(torch.float8_e4m3fn)
        b, sp, mul = pk.repack_nvfp4(qd, n, k), pk.process_nvfp4_scales(s.to(DEV), n, k), pk.mul_nvfp4_a16
    else:
        s = torch.full((n, k // 32), 127, dtype=torch.uint8)
        b, sp, mul = pk.repack_mxfp4(qd, n, k), pk.process_mxfp4_scales(s.to(DEV), n, k), pk.mul_mxfp4_a16
    a = (torch.randn(m, k, generator=torch.Generator().manual_seed(3)) * 0.05).to(dtype).to(DEV)
    bias = torch.zeros(n)
    bias[: n // 2] = -1e4
    bias = bias.to(dtype).to(DEV)
    gsd = torch.ones(1, device=DEV)
    h = _hints(pk, kind, is_bf16)
    sids = [-1] + [x for x in pk.ops.get_fp4_solutions(h, m, n, k) if ((x >> 52) & 0xF) % 2 == 0 and (x >> 48) & 0xF not in (9, 12, 13)][:8]
    two_way = [(x & ~(0xF << 60)) | (2 << 60) for x in sids[1:4]]
    ran = 0
    for sid in sids + two_way:
        try:
            c = mul(a, b, sp, gsd, m, n, k, sid, bias=bias, activation="swiglu_oai")
        except RuntimeError:
            assert sid in two_way                                 # (a kernel that does not take a 2-way split of this K)
            continue
        cb = bits(c)
        assert ((cb & 0x7FFF) == 0).all(), f"sid {sid:#x}: {np.unique(cb)[:8]}"
        ran += 1
    assert ran >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("k", [768, 2048])
@pytest.mark.parametrize("kind,is_bf16", [("nv", True), ("mx", True), ("mx", False)])
def test_moe_swiglu_oai_bit_identical_to_dense_per_expert(pk, kind, is_bf16, k):
    """The plain and the indexed MoE launch with activation="swiglu_oai" and a bias: each expert's rows equal, bit for bit, the dense call
    with the same id, activation and that expert's bias on those rows.  The ids cover the decode-, staged- and tiled-form kernels."""
    dtype = torch.bfloat16 if is_bf16 else torch.float16
    counts = np.array([1, 0, 3, 16, 40, 130, 0])
    E, m, n = len(counts), int(counts.sum()), 288 if kind == "nv" else 320
    ex = Experts(pk, kind, E, n, k, seed=199 + k, mx_band=(122, 127), gs_scale=0.1)
    offs = _offsets(counts)
    offd = torch.from_numpy(offs).to(DEV)
    ad = torch.randn(m, k, generator=torch.Generator().manual_seed(5)).to(dtype).to(DEV)
    bias = (torch.randn(E, n, generator=torch.Generator().manual_seed(6)) * 0.5).to(dtype).to(DEV)
    h = _hints(pk, kind, is_bf16)
    ids = set()
    for r in (1, 3, 16, 40, 130):
        ids.update(pk.ops.get_fp4_solutions(h, r, n, k))
    accepted = sorted(i for i in ids if pk.moe_resolve_solution(h, E, m, n, k, i, "swiglu_oai"))
    assert accepted == sorted(i for i in ids if pk.moe_resolve_solution(h, E, m, n, k, i, "silu_mul"))
    desc = [pk.ops._lib.describe_solution(i) for i in accepted]
    # (K % 512 != 0: the MXFP4 table has two staged kernels of that span size, one of them with an odd n-tile count per wave)
    assert sum(d.startswith("tiled") for d in desc) >= 1 and sum(not d.startswith("tiled") for d in desc) >= (1 if k % 512 else 2), desc
    fn_dense = pk.mul_nvfp4_a16 if kind == "nv" else pk.mul_mxfp4_a16
    fn_idx = pk.mul_nvfp4_a16_moe_indexed if kind == "nv" else pk.mul_mxfp4_a16_moe_indexed
    ident = torch.arange(m, dtype=torch.int32, device=DEV)
    total = 0
    for sid in accepted + [-1]:
        c = ex.mul(pk, ad, offd, m, sid, bias=bias, activation="swiglu_oai")
        assert c.shape == (m, n // 2)
        ci = fn_idx(ad, ex.b, ex.sp, ex.gsd, offd, m, n, k, E, a_row_index=ident, c_row_index=ident, c_rows=m, solution_id=sid, bias=bias,
                    activation="swiglu_oai")
        assert torch.equal(c.view(torch.int16), ci.view(torch.int16)), f"indexed differs from plain: {sid:#x}"
        silu = ex.mul(pk, ad, offd, m, sid, bias=bias, activation="silu_mul")
        assert not torch.equal(c.view(torch.int16), silu.view(torch.int16))
        if sid == -1:
            continue
        for e in range(E):
            lo, hi = offs[e], offs[e + 1]
            if hi == lo:
                continue
            per_s = n * k // (16 if kind == "nv" else 32)
            bw = ex.b.view(-1)[e * n * k // 8:(e + 1) * n * k // 8].view(n // 16, 2 * k)
            sw = ex.sp.view(-1)[e * per_s:(e + 1) * per_s]
            sw = sw.view(n, k // 16) if kind == "nv" else sw.view(n // 32, k)
            try:
                d = fn_dense(ad[lo:hi].contiguous(), bw, sw, ex.gsd[e:e + 1], hi - lo, n, k, sid, bias=bias[e].contiguous(), activation="swiglu_oai")
            except RuntimeError:
                continue   # (a staged kernel holds fewer rows than this expert has: the dense call refuses it)
            assert np.array_equal(bits(c[lo:hi]), bits(d)), f"{pk.ops._lib.describe_solution(sid)}: expert {e} differs from the dense call"
            total += 1
    assert total >= 3 * len(accepted) // 2


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp6", "mxfp4"])
@pytest.mark.parametrize("kind,is_bf16", [("mx", True), ("mx", False), ("nv", True)])
def test_native_moe_swiglu_oai_bit_identical_to_dense_native(pk, kind, is_bf16, fmt):
    """The native MoE launch with activation="swiglu_oai" and a bias, 16-bit and quantised output: per expert the rows equal the dense native
    call with the same id on that expert's rows, bit for bit (the quantised form: byte for byte after the fixed re-layout by rows)."""
    from test_moe_native import FMTS, _rows_of
    E, n, k = 6, 512, 768
    ne = NativeExperts(pk, kind, E, n, k, 17 + k)
    dt = torch.bfloat16 if is_bf16 else torch.float16
    bias = (torch.randn(E, n, device=DEV) * 0.5).to(dt)
    h = _hints(pk, kind, is_bf16)
    for counts in ROUTINGS:
        m = sum(counts)
        sid = pk.native_moe_resolve_solution(h, E, m, n, k, SENTINEL[fmt], activation="swiglu_oai")
        assert sid and sid == pk.native_moe_resolve_solution(h, E, m, n, k, SENTINEL[fmt], activation="silu_mul")
        a = torch.randn(m, k, device=DEV).to(dt) * 4.0
        off = _offsets_dev(counts)
        got = ne.moe(pk, a, off, m, sid, bias=bias, activation="swiglu_oai")
        assert got.shape == (m, n // 2)
        assert not torch.equal(got, ne.moe(pk, a, off, m, sid, bias=bias, activation="silu_mul"))
        gq = ne.moe(pk, a, off, m, sid, bias=bias, activation="swiglu_oai", out_quantized=fmt)
        gq_rows = _rows_of(gq.data, m, n // 2, FMTS[fmt])
        o = np.concatenate([[0], np.cumsum(counts)])
        for e in range(E):
            if counts[e] == 0:
                continue
            rows = a[o[e]:o[e + 1]].contiguous()
            ref = ne.dense(pk, rows, e, sid, bias=bias[e].contiguous(), activation="swiglu_oai")
            assert torch.equal(got[o[e]:o[e + 1]].view(torch.int16), ref.view(torch.int16)), f"expert {e}, counts {counts}"
            rq = ne.dense(pk, rows, e, sid, bias=bias[e].contiguous(), activation="swiglu_oai", out_quantized=fmt)
            assert np.array_equal(gq_rows[o[e]:o[e + 1]], _rows_of(rq.data, counts[e], n // 2, FMTS[fmt])), f"quantised: expert {e}"


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp6", "mxfp4"])
@pytest.mark.parametrize("m,n,k,with_bias", [(64, 512, 1024, False), (130, 1024, 512, True), (512, 1536, 2048, False), (5, 512, 768, False)])
def test_quantized_swiglu_oai_output_feeds_the_next_gemm(pk, m, n, k, with_bias, fmt):
    """test_quantized_silu_mul_output_feeds_the_next_gemm's construction and bounds with activation="swiglu_oai": the emitted bytes decode to
    the 16-bit fused result within one quantisation step of their block, and `down` run on them is the oracle's product of the decoded bytes."""
    a_bits, q, s, gs, a, b, sp, gsd = _mx_problem_on_device(pk, m, n, k, 7300 + m + n + k)
    bias = (torch.randn(n, device=DEV) * 0.5).bfloat16() if with_bias else None
    sentinel = NATIVE_SENTINEL(pk, fmt)
    c16 = pk.mul_mxfp4_native(a, b, sp, gsd, m, n, k, sentinel, bias=bias, activation="swiglu_oai")
    qout = pk.mul_mxfp4_native(a, b, sp, gsd, m, n, k, sentinel, bias=bias, activation="swiglu_oai", out_quantized=fmt)
    assert isinstance(qout, pk.QuantizedActivations) and (qout.m, qout.k, qout.fmt) == (m, n // 2, fmt)
    assert not torch.equal(c16, pk.mul_mxfp4_native(a, b, sp, gsd, m, n, k, sentinel, bias=bias, activation="silu_mul"))
    ref16 = c16.float().cpu().numpy()
    deq = decode_qact(qout.data.cpu().numpy(), m, n // 2, fmt)
    blk = np.abs(ref16).reshape(m, -1, 32).max(axis=2)
    step = np.repeat(np.exp2(np.floor(np.log2(np.maximum(blk, 1e-30)))), 32, axis=1).reshape(m, -1)   # 2^E of the block maximum
    err = np.abs(deq - ref16)
    if fmt == "mxfp4":
        assert (err <= 0.5 * step + 2.0 ** -7 * np.abs(ref16)).all(), err.max()
    elif fmt == "mxfp6":
        assert (err <= 2.0 ** -4 * np.abs(ref16) + 2.0 ** -6 * step + 2.0 ** -7 * np.abs(ref16) + np.where(np.abs(ref16) > 1.875 * step, 0.125 * step, 0.0)).all(), err.max()
    else:
        assert (err <= 2.0 ** -4 * np.abs(ref16) + 2.0 ** -9 * step + 2.0 ** -7 * np.abs(ref16)).all(), err.max()
    assert np.sqrt(np.mean(err ** 2)) <= {"mxfp4": 0.15, "mxfp6": 0.04, "mxfp8": 0.03}[fmt] * np.sqrt(np.mean(ref16 ** 2))
    n2 = 256
    _, q2, s2, gs2 = random_problem("mx", 1, n2, n // 2, 99 + n, True)
    b2 = pk.repack_mxfp4(torch.from_numpy(q2).to(DEV).view(torch.int32), n2, n // 2)
    sp2 = pk.process_mxfp4_scales(torch.from_numpy(s2).to(DEV), n2, n // 2)
    gsd2 = torch.tensor([gs2], dtype=torch.float32, device=DEV)
    y_fused = pk.mul_mxfp4_native(qout, b2, sp2, gsd2, m, n2, n // 2, sentinel).float()
    y_two = pk.mul_mxfp4_native(pk.quantize_activations(c16, fmt), b2, sp2, gsd2, m, n2, n // 2, sentinel).float()
    diff = (y_fused - y_two).pow(2).mean().sqrt().item() / max(y_two.pow(2).mean().sqrt().item(), 1e-9)
    assert diff <= {"mxfp4": 0.08, "mxfp6": 0.03, "mxfp8": 0.02}[fmt], diff
    dq2 = O.dequant_mxfp4(q2, s2)
    _, want = O.gemm_ref(O.f32_to_bf16_bits(deq), True, dq2, gs2)
    check_gemm(bits(pk.mul_mxfp4_native(qout, b2, sp2, gsd2, m, n2, n // 2, sentinel)), want, True,
               (np.abs(deq) @ np.abs(dq2).T) * gs2, sum_abs_coef=1e-4)
    with pytest.raises(RuntimeError):
        pk.mul_mxfp4_native(a, b, sp, gsd, m, n, k, sentinel, out_quantized=fmt)                             # no gated activation

"""NVFP4 weights on the native class without a resident image: petit_gemm_nvfp4_native_transient / mul_nvfp4_native_transient (the image is
built per call into the front of the call's workspace, then the native call runs on it) and the image builder it runs on every call
(csrc/nvnative.hip nv6_image_kernel).

Unmarked tests run without a GPU (symbols, the workspace query against its documented layout, refusals that return before any device work,
Meta shapes of the torch op); the @pytest.mark.gpu ones check the builder against its host twin byte for byte, bit-identity with the
attached-image call it stands for (every sentinel and listed native id, bias, SiLU-mul, pre-quantised activations, quantised output, the
bulk + tail row split), and the semantics of a per-call image (graph replay after the weights change, a shared workspace, exact sizing).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_parity import from_bits, random_problem

DEV = "cuda"
SENTINELS = {"mxfp8": -2, "mxfp4": -3, "mxfp6": -4}


def _align256(x):
    return (x + 255) // 256 * 256


def _lib():
    import petit_kernel  # noqa: F401
    from petit_kernel import _lib
    return _lib


def _hints(_lib, bf16=True):
    a = _lib.CXX_DTYPE_BF16 if bf16 else _lib.CXX_DTYPE_FP16
    return _lib.SolutionHints(a, _lib.CXX_DTYPE_FP4_E2M1, a, 0)


def _csid(_lib, sentinel):
    return {-2: _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP8, -3: _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP4, -4: _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP6}[sentinel]


# --- without a GPU ----------------------------------------------------------------------------------------------------------------

def test_transient_symbols_exist():
    import petit_kernel as pk
    L = _lib().lib
    assert L.petit_gemm_nvfp4_native_transient and L.petit_gemm_nvfp4_native_transient_workspace_bytes
    assert callable(pk.mul_nvfp4_native_transient) and callable(pk.nvfp4_native_transient_workspace_bytes)
    assert "mul_nvfp4_native_transient" in pk.__all__ and "nvfp4_native_transient_workspace_bytes" in pk.__all__
    assert callable(pk.ops.mul_nvfp4_native_transient) and callable(pk.compiled.mul_nvfp4_native_transient)
    from petit_kernel import compiled
    assert compiled.available(), compiled.why_unavailable()
    assert hasattr(torch.ops.petit_kernel, "mul_nvfp4_native_transient")


@pytest.mark.parametrize("m,n,k", [(1024, 8192, 8192), (512, 1024, 2048), (256, 2048, 768), (64, 48, 512)])
def test_transient_workspace_is_image_then_native_scratch(m, n, k):
    """The query returns align256(image bytes) + the scratch of the call it stands for: petit_gemm_native_workspace_bytes with native args
    (pre-quantised activations, quantised output), petit_gemm_workspace_bytes_ex with the sentinel for 16-bit in and out (the attached-image
    call, its row split included)."""
    _lib_ = _lib()
    L = _lib_.lib
    img = _align256(int(L.petit_nvfp4_native_image_bytes(k, n)))
    assert img > 0
    for bf16 in (True, False):
        h = _hints(_lib_, bf16)
        for sentinel, fmt in ((-2, 8), (-3, 4), (-4, 6)):
            sid = C.c_uint64(_csid(_lib_, sentinel))
            attached = int(L.petit_gemm_workspace_bytes_ex(C.byref(h), m, n, k, sid, None))
            assert attached > 0
            assert int(L.petit_gemm_nvfp4_native_transient_workspace_bytes(C.byref(h), m, n, k, sid, None, None)) == img + attached
            na0 = _lib_.NativeArgs(C.sizeof(_lib_.NativeArgs), 0, 0, 0)
            assert int(L.petit_gemm_nvfp4_native_transient_workspace_bytes(C.byref(h), m, n, k, sid, None, C.byref(na0))) == img + attached
            na = _lib_.NativeArgs(C.sizeof(_lib_.NativeArgs), fmt, 0, 0)
            native = int(L.petit_gemm_native_workspace_bytes(C.byref(h), m, n, k, sid, None, C.byref(na)))
            assert int(L.petit_gemm_nvfp4_native_transient_workspace_bytes(C.byref(h), m, n, k, sid, None, C.byref(na))) == img + native
            if n % 512 == 0:
                epi = _lib_.Epilogue(None, 1, 0)
                nq = _lib_.NativeArgs(C.sizeof(_lib_.NativeArgs), 0, fmt, 0)
                native = int(L.petit_gemm_native_workspace_bytes(C.byref(h), m, n, k, sid, C.byref(epi), C.byref(nq)))
                assert native > 0
                assert int(L.petit_gemm_nvfp4_native_transient_workspace_bytes(C.byref(h), m, n, k, sid, C.byref(epi), C.byref(nq))) == img + native
    import petit_kernel as pk
    assert pk.nvfp4_native_transient_workspace_bytes(m, n, k) == img + int(L.petit_gemm_workspace_bytes_ex(
        C.byref(_hints(_lib_)), m, n, k, C.c_uint64(_lib_.PETIT_SOLUTION_AUTO_NATIVE_MXFP8), None))


def test_transient_refusals_without_a_gpu():
    """Refusals return before any device work: PETIT_SOLUTION_AUTO and exact-class ids, shapes the image does not take, a workspace that is missing,
    smaller than the image or misaligned, bad native args.  The queries answer 0 for them."""
    _lib_ = _lib()
    L = _lib_.lib
    buf = (C.c_uint8 * 4096)()
    p = C.c_void_p((C.addressof(buf) + 255) & ~255)
    shape, kern, bad = _lib_.PETIT_ERROR_PROBLEM_SHAPE, _lib_.PETIT_ERROR_KERNEL_SHAPE, _lib_.PETIT_ERROR_BAD_ARGUMENT
    h = _hints(_lib_)
    m, n, k = 256, 1024, 2048
    big = 1 << 40
    s8 = C.c_uint64(_lib_.PETIT_SOLUTION_AUTO_NATIVE_MXFP8)

    def call(sid, m=m, n=n, k=k, ws=p, ws_bytes=big, native=None):
        return L.petit_gemm_nvfp4_native_transient(p, p, p, p, p, m, n, k, C.byref(h), C.c_uint64(sid) if isinstance(sid, int) else sid, None, native,
                                                   ws, C.c_uint64(ws_bytes), None)

    def query(sid, m=m, n=n, k=k, native=None):
        return int(L.petit_gemm_nvfp4_native_transient_workspace_bytes(C.byref(h), m, n, k, C.c_uint64(sid) if isinstance(sid, int) else sid, None, native))

    assert call(_lib_.PETIT_SOLUTION_AUTO) == kern and query(_lib_.PETIT_SOLUTION_AUTO) == 0
    count = C.c_uint(0)
    assert L.petit_gemm_get_solutions(C.byref(h), m, n, k, None, C.byref(count)) == 0
    ids = (C.c_uint64 * max(count.value, 1))()
    assert L.petit_gemm_get_solutions(C.byref(h), m, n, k, ids, C.byref(count)) == 0
    exact = [int(x) for x in ids[: count.value] if (int(x) >> 48) & 0xF != 13]
    assert exact
    for sid in exact[:8]:
        assert call(sid) == kern and query(sid) == 0, hex(sid)
    assert call(s8, n=1000) == shape and query(s8, n=1000) == 0          # N % 16
    assert call(s8, k=2000) == shape and query(s8, k=2000) == 0          # K % 256
    img = _align256(int(L.petit_nvfp4_native_image_bytes(k, n)))
    assert call(s8, ws=None, ws_bytes=0) == kern                          # no workspace (a registered one never holds the image)
    assert call(s8, ws_bytes=img - 256) == kern                           # smaller than the image
    assert call(s8, ws=C.c_void_p(p.value + 16)) == bad                   # misaligned
    na_bad = _lib_.NativeArgs(C.sizeof(_lib_.NativeArgs), 7, 0, 0)
    assert call(s8, native=C.byref(na_bad)) == bad and query(s8, native=C.byref(na_bad)) == 0
    na_q = _lib_.NativeArgs(C.sizeof(_lib_.NativeArgs), 0, 8, 0)
    assert call(s8, native=C.byref(na_q)) == bad                          # a quantised output needs SiLU-mul
    assert call(s8, m=0) == _lib_.PETIT_OK                                # nothing to do


def test_transient_op_meta_shapes():
    import petit_kernel  # noqa: F401
    from petit_kernel import compiled
    assert compiled.available(), compiled.why_unavailable()
    ops = torch.ops.petit_kernel
    m, n, k = 12, 1024, 512
    a = torch.empty(m, k, dtype=torch.bfloat16, device="meta")
    b = torch.empty(n // 16, 2 * k, dtype=torch.int32, device="meta")
    s = torch.empty(n, k // 16, dtype=torch.float8_e4m3fn, device="meta")
    gs = torch.empty(1, dtype=torch.float32, device="meta")
    c = ops.mul_nvfp4_native_transient(a, b, s, gs, m, n, k, -2)
    assert c.shape == (m, n) and c.dtype == torch.bfloat16 and c.device.type == "meta"
    c = ops.mul_nvfp4_native_transient(a.half(), b, s, gs, m, n, k, -4, None, 1)
    assert c.shape == (m, n // 2) and c.dtype == torch.float16
    L = _lib().lib
    for f in (8, 6, 4):
        c = ops.mul_nvfp4_native_transient(a, b, s, gs, m, n, k, -2, None, 1, 0, 5, f)
        assert c.shape == (int(L.petit_quantized_activation_bytes(m, n // 2, f)),) and c.dtype == torch.uint8
        qa = torch.empty(int(L.petit_quantized_activation_bytes(m, k, f)), dtype=torch.uint8, device="meta")
        c = ops.mul_nvfp4_native_transient(qa, b, s, gs, m, n, k, -2, None, 0, f, 4, 0)
        assert c.shape == (m, n) and c.dtype == torch.float16


# --- on the GPU -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pk():
    import petit_kernel
    assert torch.cuda.is_available()
    assert torch.cuda.get_device_properties(0).gcnArchName.startswith("gfx950")
    return petit_kernel


def _weights(pk, n, k, seed, special=False):
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (n, k // 2), dtype=np.uint8)
    s = torch.from_numpy(rng.random((n, k // 16), dtype=np.float32) * 3.5 + 0.25).to(torch.float8_e4m3fn).view(torch.uint8).numpy().copy()
    if special:
        u = rng.random(s.shape)
        s[u < 0.04] |= 0x80                                   # negative scales
        s[(u >= 0.04) & (u < 0.06)] = 0x80                    # negative zero
        s[(u >= 0.06) & (u < 0.07)] = 0x7F                    # NaN
        s[(u >= 0.07) & (u < 0.08)] = 0xFF                    # NaN, negative
        s[(u >= 0.08) & (u < 0.10)] = rng.integers(1, 8, int(((u >= 0.08) & (u < 0.10)).sum()))   # e4m3 subnormals
        q[rng.random((n, 1)).repeat(k // 2, axis=1) < 0.05] = 0
        q[rng.random(q.shape) < 0.05] = 0x88                  # negative-zero nibbles
    b = pk.repack_nvfp4(torch.from_numpy(q).to(DEV).view(torch.int32), n, k)
    sp = pk.process_nvfp4_scales(torch.from_numpy(s).to(DEV).view(torch.float8_e4m3fn), n, k)
    return b, sp


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", [(32, 256), (48, 768), (272, 1024), (528, 512), (1040, 2048), (2048, 8192)])
def test_builder_equals_host_twin(pk, n, k):
    """The device builder equals the host twin byte for byte: span sizes KS = 8 / 4 / 2, N % 32 == 16, NaN / negative / negative-zero / subnormal
    scales, zero rows and negative-zero nibbles."""
    b, sp = _weights(pk, n, k, n * 7 + k, special=True)
    image = pk.nvfp4_native_image(b, sp, n, k)
    host = pk.offline.nvfp4_native_image_cpu(b.cpu(), sp.cpu(), n, k)
    got = image.cpu()
    assert got.numel() == host.numel()
    diff = int((got != host).sum())
    assert diff == 0, f"{diff} of {host.numel()} image bytes differ from the host twin"


@pytest.mark.gpu
def test_transient_workspace_holds_the_image(pk):
    """After a transient call the image region of the workspace (offset 0) holds nvfp4_native_image(b, s), and C equals the call on that image."""
    _lib_ = _lib()
    L = _lib_.lib
    m, n, k = 300, 1040, 2048
    a_bits, _, _, gs = random_problem("nv", m, n, k, 5, True)
    b, sp = _weights(pk, n, k, 11, special=False)
    a = from_bits(a_bits, torch.bfloat16).to(DEV)
    gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
    h = _hints(_lib_)
    sid = C.c_uint64(_lib_.PETIT_SOLUTION_AUTO_NATIVE_MXFP8)
    need = int(L.petit_gemm_nvfp4_native_transient_workspace_bytes(C.byref(h), m, n, k, sid, None, None))
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)
    c = torch.zeros((m, n), dtype=torch.bfloat16, device=DEV)
    rc = L.petit_gemm_nvfp4_native_transient(c.data_ptr(), a.data_ptr(), b.data_ptr(), sp.data_ptr(), gsd.data_ptr(), m, n, k, C.byref(h), sid, None,
                                             None, ws.data_ptr(), need, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    image = pk.nvfp4_native_image(b, sp, n, k)
    assert torch.equal(ws[: image.numel()], image)
    pk.attach_nvfp4_native(b, image)
    try:
        assert torch.equal(c.view(torch.int16), pk.mul_nvfp4_a16(a, b, sp, gsd, m, n, k, -2).view(torch.int16))
    finally:
        pk.attach_nvfp4_native(b, None)


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [(1, 512, 2048), (64, 512, 2048), (300, 1024, 768), (2084, 2048, 1024), (1024, 8192, 8192)])
@pytest.mark.parametrize("is_bf16", [True, False])
def test_transient_equals_attached_image(pk, m, n, k, is_bf16):
    """Bit-identity with the call a transient call stands for: every sentinel against mul_nvfp4_a16(..., -2 / -3 / -4) on the attached image (its
    row split at a ragged M included), with bias and with SiLU-mul; pre-quantised activations and the quantised SiLU-mul output against
    mul_nvfp4_native on the image; both Python layers."""
    dtype = torch.bfloat16 if is_bf16 else torch.float16
    a_bits, _, _, gs = random_problem("nv", m, n, k, 31 + m + n, is_bf16)
    b, sp = _weights(pk, n, k, 17 + n + k)
    a = from_bits(a_bits, dtype).to(DEV)
    gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
    bias = (torch.randn(n, device=DEV) * 0.5).to(dtype)
    image = pk.nvfp4_native_image(b, sp, n, k)
    pk.attach_nvfp4_native(b, image)
    try:
        for fmt, sid in SENTINELS.items():
            want = pk.mul_nvfp4_a16(a, b, sp, gsd, m, n, k, sid)
            for layer in (pk, pk.ops, pk.compiled):
                got = layer.mul_nvfp4_native_transient(a, b, sp, gsd, m, n, k, sid)
                assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"{fmt} {layer.__name__}"
            want = pk.mul_nvfp4_a16(a, b, sp, gsd, m, n, k, sid, bias=bias)
            assert torch.equal(pk.mul_nvfp4_native_transient(a, b, sp, gsd, m, n, k, sid, bias=bias).view(torch.int16), want.view(torch.int16)), fmt
            want = pk.mul_nvfp4_a16(a, b, sp, gsd, m, n, k, sid, activation="silu_mul")
            got = pk.mul_nvfp4_native_transient(a, b, sp, gsd, m, n, k, sid, activation="silu_mul")
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"{fmt} silu_mul"
            qa = pk.quantize_activations(a, fmt)
            want = pk.mul_nvfp4_native(qa, image, gsd, m, n, k, sid, bias=bias)
            assert torch.equal(pk.mul_nvfp4_native_transient(qa, b, sp, gsd, m, n, k, sid, bias=bias).view(torch.int16), want.view(torch.int16)), fmt
            if n % 512 == 0:
                want = pk.mul_nvfp4_native(a, image, gsd, m, n, k, sid, activation="silu_mul", out_quantized=fmt)
                got = pk.mul_nvfp4_native_transient(a, b, sp, gsd, m, n, k, sid, activation="silu_mul", out_quantized=fmt)
                assert torch.equal(got.data, want.data), f"{fmt} out_quantized"
    finally:
        pk.attach_nvfp4_native(b, None)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [64, 300])
def test_transient_every_listed_native_id(pk, m):
    """Every explicit native id of the NVFP4 family that get_fp4_solutions lists runs transient bit for bit as on the image (K split 1 and 2)."""
    n, k = 512, 2048
    a_bits, _, _, gs = random_problem("nv", m, n, k, 77 + m, True)
    b, sp = _weights(pk, n, k, 78)
    a = from_bits(a_bits, torch.bfloat16).to(DEV)
    gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
    image = pk.nvfp4_native_image(b, sp, n, k)
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = torch.bfloat16
    h.b_type = pk.DataType.float4_e2m1
    pk.ops.enable_native_fp4(True)
    try:
        native = [sid for sid in pk.ops.get_fp4_solutions(h, m, n, k) if (sid >> 48) & 0xF == 13]
    finally:
        pk.ops.enable_native_fp4(False)
    assert native
    for sid in native:
        for splitk in (1, 2):
            sk = (sid & ~(0xF << 60)) | (splitk << 60)
            want = pk.mul_nvfp4_native(a, image, gsd, m, n, k, sk)
            got = pk.mul_nvfp4_native_transient(a, b, sp, gsd, m, n, k, sk)
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), hex(sk)


@pytest.mark.gpu
def test_transient_graph_replay_follows_new_weights(pk):
    """A captured transient call reads b / s at every replay: overwrite them in place with a second weight set and the replay computes with it
    (an image attached at capture time would not)."""
    m, n, k = 256, 1024, 2048
    a_bits, _, _, gs = random_problem("nv", m, n, k, 3, True)
    a = from_bits(a_bits, torch.bfloat16).to(DEV)
    gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
    b1, s1 = _weights(pk, n, k, 101)
    b2, s2 = _weights(pk, n, k, 202)
    b, sp = b1.clone(), s1.clone()
    want1 = pk.mul_nvfp4_native_transient(a, b1, s1, gsd, m, n, k, -2)
    want2 = pk.mul_nvfp4_native_transient(a, b2, s2, gsd, m, n, k, -2)
    assert not torch.equal(want1, want2)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        pk.mul_nvfp4_native_transient(a, b, sp, gsd, m, n, k, -2)     # warm-up outside the capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            out = pk.mul_nvfp4_native_transient(a, b, sp, gsd, m, n, k, -2)
        g.replay()
        st.synchronize()
        assert torch.equal(out.view(torch.int16), want1.view(torch.int16))
        b.copy_(b2)
        sp.copy_(s2)
        g.replay()
        st.synchronize()
        assert torch.equal(out.view(torch.int16), want2.view(torch.int16))
    torch.cuda.current_stream().wait_stream(st)


@pytest.mark.gpu
def test_transient_shared_workspace_exact_size_and_refusals(pk):
    """Two transient calls on different weights share one workspace back to back; a workspace of exactly the queried bytes runs, 256 fewer is
    refused with C untouched; an exact-class id through petit_gemm_nvfp4_native is refused."""
    _lib_ = _lib()
    L = _lib_.lib
    m, n, k = 512, 1024, 2048
    a_bits, _, _, gs = random_problem("nv", m, n, k, 9, True)
    a = from_bits(a_bits, torch.bfloat16).to(DEV)
    gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
    (b1, s1), (b2, s2) = _weights(pk, n, k, 301), _weights(pk, n, k, 302)
    h = _hints(_lib_)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pk.ops.enable_native_fp4(True)
    try:
        ph = pk.PetitSolutionHints()
        ph.a_type = ph.c_type = torch.bfloat16
        ph.b_type = pk.DataType.float4_e2m1
        ids = pk.ops.get_fp4_solutions(ph, m, n, k)
    finally:
        pk.ops.enable_native_fp4(False)
    explicit = [x for x in ids if (x >> 48) & 0xF == 13 and (x >> 32) & 7 == 2][0] & ~(0xF << 60) | (1 << 60)
    exact = [x for x in ids if (x >> 48) & 0xF != 13][0]
    for sid in (C.c_uint64(_lib_.PETIT_SOLUTION_AUTO_NATIVE_MXFP8), C.c_uint64(explicit)):
        need = int(L.petit_gemm_nvfp4_native_transient_workspace_bytes(C.byref(h), m, n, k, sid, None, None))
        assert need > _align256(int(L.petit_nvfp4_native_image_bytes(k, n)))
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        c1 = torch.zeros((m, n), dtype=torch.bfloat16, device=DEV)
        c2 = torch.zeros_like(c1)
        for c, b, s in ((c1, b1, s1), (c2, b2, s2)):
            rc = L.petit_gemm_nvfp4_native_transient(c.data_ptr(), a.data_ptr(), b.data_ptr(), s.data_ptr(), gsd.data_ptr(), m, n, k, C.byref(h), sid,
                                                     None, None, ws.data_ptr(), need, stream)
            assert rc == 0
        for c, b, s in ((c1, b1, s1), (c2, b2, s2)):
            image = pk.nvfp4_native_image(b, s, n, k)
            want = pk.mul_nvfp4_native(a, image, gsd, m, n, k, -2 if sid.value == _lib_.PETIT_SOLUTION_AUTO_NATIVE_MXFP8 else sid.value)
            assert torch.equal(c.view(torch.int16), want.view(torch.int16))
        if sid.value == explicit:
            c3 = torch.zeros((m, n), dtype=torch.bfloat16, device=DEV)
            rc = L.petit_gemm_nvfp4_native_transient(c3.data_ptr(), a.data_ptr(), b1.data_ptr(), s1.data_ptr(), gsd.data_ptr(), m, n, k, C.byref(h), sid,
                                                     None, None, ws.data_ptr(), need - 256, stream)
            assert rc == _lib_.PETIT_ERROR_BAD_ARGUMENT
            torch.cuda.synchronize()
            assert torch.count_nonzero(c3) == 0
    # an exact-class id on an image: refused by both entry points, C untouched
    image = pk.nvfp4_native_image(b1, s1, n, k)
    c = torch.zeros((m, n), dtype=torch.bfloat16, device=DEV)
    ws = torch.empty(1 << 26, dtype=torch.uint8, device=DEV)
    rc = L.petit_gemm_nvfp4_native(c.data_ptr(), a.data_ptr(), image.data_ptr(), gsd.data_ptr(), m, n, k, C.byref(h), C.c_uint64(exact), None, None,
                                   ws.data_ptr(), ws.numel(), stream)
    assert rc == _lib_.PETIT_ERROR_KERNEL_SHAPE
    rc = L.petit_gemm_nvfp4_native_transient(c.data_ptr(), a.data_ptr(), b1.data_ptr(), s1.data_ptr(), gsd.data_ptr(), m, n, k, C.byref(h),
                                             C.c_uint64(exact), None, None, ws.data_ptr(), ws.numel(), stream)
    assert rc == _lib_.PETIT_ERROR_KERNEL_SHAPE
    torch.cuda.synchronize()
    assert torch.count_nonzero(c) == 0
    with pytest.raises(RuntimeError, match="No kernel implementation"):
        pk.mul_nvfp4_native(a, image, gsd, m, n, k, exact)

"""Native-class MoE on NVFP4 experts without resident images: the multi-expert image builder with its routing skip
(petit_nvfp4_native_images / _host, csrc/nvnative.hip nv6_images_kernel), the transient launch (petit_gemm_native_moe_transient /
mul_nvfp4_native_moe_transient) and the layers' switch (fp4_moe_native / fp4_moe_routed with transient=True).

Every comparison is bit for bit.  Unmarked tests run without a GPU (symbols, the workspace query against its documented layout, refusals
that return before any device work, the host twin of the builder and of its skip rule, Meta shapes of the torch op); the @pytest.mark.gpu
ones check the device builder against the host twin on a poisoned buffer with a guard behind it, the transient launch against
mul_nvfp4_native_moe on nvfp4_native_images of the same tensors, the workspace's contents and sizing, graph replays after the routing and
the weights change, and the layers.

The layer shapes: down's K is the intermediate size I, so I % 256 == 0 and n13 = 2 I is always a multiple of 512 -- a layer whose gate_up
cannot hand quantised rows to down does not exist; the 16-bit hand-over is covered at the launch level (SiLU-mul without out_quantized).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_moe import Experts, _hints, _make_layer, _routing

DEV = "cuda"
FMTS = {"mxfp8": 8, "mxfp6": 6, "mxfp4": 4}
SENTINEL = {"mxfp8": -2, "mxfp4": -3, "mxfp6": -4}
POISON = 0xA5


def _L():
    import petit_kernel  # noqa: F401
    from petit_kernel import _lib
    return _lib


def _csid(_lib, py_sid):
    return {-2: _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP8, -3: _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP4, -4: _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP6}[py_sid]


def _nv_hints(_lib, bf16=True):
    a = _lib.CXX_DTYPE_BF16 if bf16 else _lib.CXX_DTYPE_FP16
    return _lib.SolutionHints(a, _lib.CXX_DTYPE_FP4_E2M1, a, 0)


def _has_rows(offsets, m):
    """The MoE launch's rule (csrc/gemm_moe.hpp): every offset clamped into [0, m], then a running maximum; an expert has rows when its
    upper end exceeds its lower one.  Written out here independently of the library."""
    lo = min(max(int(offsets[0]), 0), m)
    out = []
    for e in range(len(offsets) - 1):
        hi = max(lo, min(max(int(offsets[e + 1]), 0), m))
        out.append(hi > lo)
        lo = hi
    return out


# (offsets [E + 1] for E = 5, m): some experts empty; all rows on the last expert; no rows at all; decreasing offsets; offsets beyond m and
# below 0; a first offset that is not 0
SKIP_ROUTINGS = [
    ([0, 3, 3, 7, 7, 9], 9),
    ([0, 0, 0, 0, 0, 9], 9),
    ([0, 0, 0, 0, 0, 0], 0),
    ([0, 5, 2, 4, 9, 9], 9),
    ([0, 20, 3, 50, -4, 7], 9),
    ([4, 2, 6, 6, 100, 100], 8),
    ([-3, -1, 0, 2, 2, 1 << 30], 6),
]


def test_skip_routings_cover_what_they_should():
    assert _has_rows(*SKIP_ROUTINGS[0]) == [True, False, True, False, True]
    assert _has_rows(*SKIP_ROUTINGS[1]) == [False, False, False, False, True]
    assert _has_rows(*SKIP_ROUTINGS[2]) == [False] * 5
    assert _has_rows(*SKIP_ROUTINGS[3]) == [True, False, False, True, False]
    assert _has_rows(*SKIP_ROUTINGS[4]) == [True, False, False, False, False]
    assert _has_rows(*SKIP_ROUTINGS[5]) == [False, True, False, True, False]
    assert _has_rows(*SKIP_ROUTINGS[6]) == [False, False, True, False, True]


# --- without a GPU ----------------------------------------------------------------------------------------------------------------

def test_symbols_exist():
    import petit_kernel as pk
    _lib = _L()
    L = _lib.lib
    assert L.petit_nvfp4_native_images and L.petit_nvfp4_native_images_host
    assert L.petit_gemm_native_moe_transient and L.petit_gemm_native_moe_transient_workspace_bytes
    void_p, uint = C.c_void_p, C.c_uint
    assert L.petit_nvfp4_native_images.argtypes == [void_p] * 3 + [uint] * 3 + [void_p, uint, void_p]
    assert L.petit_nvfp4_native_images_host.argtypes == [void_p] * 3 + [uint] * 3 + [void_p, uint]
    assert L.petit_gemm_native_moe_transient.argtypes == L.petit_gemm_native_moe.argtypes
    assert L.petit_gemm_native_moe_transient_workspace_bytes.argtypes == L.petit_gemm_native_moe_workspace_bytes.argtypes
    assert L.petit_gemm_native_moe_transient_workspace_bytes.restype == C.c_uint64
    header = open(__import__("os").path.join(__import__("os").path.dirname(__file__), "..", "include", "petit_amd.h")).read()
    for name in ("petit_nvfp4_native_images(", "petit_nvfp4_native_images_host(", "petit_gemm_native_moe_transient(",
                 "petit_gemm_native_moe_transient_workspace_bytes("):
        assert name in header, name
    for name in ("mul_nvfp4_native_moe_transient", "nvfp4_native_moe_transient_workspace_bytes"):
        assert callable(getattr(pk, name)) and name in pk.__all__ and callable(getattr(pk.ops, name))
    assert callable(pk.compiled.mul_nvfp4_native_moe_transient)
    from petit_kernel import compiled
    assert compiled.available(), compiled.why_unavailable()
    assert hasattr(torch.ops.petit_kernel, "mul_nvfp4_native_moe_transient")


@pytest.mark.parametrize("E,m,n,k", [(8, 300, 512, 2048), (5, 33, 48, 768), (8, 1, 1024, 512), (256, 4096, 4096, 7168)])
def test_workspace_is_images_then_native_scratch(E, m, n, k):
    """The query is E * I + petit_gemm_native_moe_workspace_bytes of the same call, in 64 bits (the last shape: E * I > 2^32); the scratch
    part is 0 with pre-quantised a."""
    import petit_kernel as pk
    _lib = _L()
    L = _lib.lib
    per = int(L.petit_nvfp4_native_image_bytes(k, n))
    assert per > 0 and per % 256 == 0
    if E == 256:
        assert E * per > 1 << 32
    q_t, q_r = L.petit_gemm_native_moe_transient_workspace_bytes, L.petit_gemm_native_moe_workspace_bytes
    for bf16 in (True, False):
        h = _nv_hints(_lib, bf16)
        for fmt, f in FMTS.items():
            sid = C.c_uint64(_csid(_lib, SENTINEL[fmt]))
            res = int(q_r(C.byref(h), E, m, n, k, sid, None, None))
            assert res > 0
            assert int(q_t(C.byref(h), E, m, n, k, sid, None, None)) == E * per + res
            na = _lib.NativeArgs(C.sizeof(_lib.NativeArgs), f, 0, 0)
            assert int(q_r(C.byref(h), E, m, n, k, sid, None, C.byref(na))) == 0
            assert int(q_t(C.byref(h), E, m, n, k, sid, None, C.byref(na))) == E * per
            if n % 512 == 0:
                epi = _lib.Epilogue(None, 1, 0)
                nq = _lib.NativeArgs(C.sizeof(_lib.NativeArgs), 0, f, 0)
                assert int(q_t(C.byref(h), E, m, n, k, sid, C.byref(epi), C.byref(nq))) == E * per + int(q_r(C.byref(h), E, m, n, k, sid, C.byref(epi), C.byref(nq)))
            assert pk.nvfp4_native_moe_transient_workspace_bytes(E, m, n, k, SENTINEL[fmt], torch.bfloat16 if bf16 else torch.float16) == E * per + res
            assert pk.nvfp4_native_moe_transient_workspace_bytes(E, m, n, k, SENTINEL[fmt], a_format=fmt) == E * per


def test_refusals_without_a_gpu():
    """Every refusal returns its code before any device work (the pointers are host scratch), and the query answers 0 for it."""
    _lib = _L()
    L = _lib.lib
    buf = (C.c_uint8 * 8192)()
    p = C.c_void_p((C.addressof(buf) + 255) & ~255)
    shape, kern, bad, ok = _lib.PETIT_ERROR_PROBLEM_SHAPE, _lib.PETIT_ERROR_KERNEL_SHAPE, _lib.PETIT_ERROR_BAD_ARGUMENT, _lib.PETIT_OK
    s8 = _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP8
    hn = _nv_hints(_lib)
    hm = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_MXFP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
    silu = _lib.Epilogue(None, 1, 0)
    big = 1 << 40

    def na(a_fmt=0, out_fmt=0):
        return C.byref(_lib.NativeArgs(C.sizeof(_lib.NativeArgs), a_fmt, out_fmt, 0))

    def run(E=8, m=256, n=512, k=256, c=p, a=p, b=p, s=p, gs=p, off=p, a_idx=None, a_rows=256, c_idx=None, c_rows=256, sid=s8, epi=None,
            native=None, ws=p, ws_bytes=big, hints=hn):
        return L.petit_gemm_native_moe_transient(c, a, b, s, gs, off, E, m, n, k, a_idx, a_rows, c_idx, c_rows, C.byref(hints), C.c_uint64(sid),
                                                 epi, native, ws, C.c_uint64(ws_bytes), None)

    def query(E=8, m=256, n=512, k=256, sid=s8, epi=None, native=None, hints=hn):
        return int(L.petit_gemm_native_moe_transient_workspace_bytes(C.byref(hints), E, m, n, k, C.c_uint64(sid), epi, native))

    need = query()
    per = int(L.petit_nvfp4_native_image_bytes(256, 512))
    assert need == 8 * per + 256 * (256 + 8)                                             # MXFP8 rows: k bytes + k / 32 scales each
    # never another accuracy class
    exact_id = L.petit_gemm_moe_resolve_solution(C.byref(hn), 8, 256, 512, 256, C.c_uint64(_lib.PETIT_SOLUTION_AUTO), None)
    assert exact_id != 0
    assert run(sid=_lib.PETIT_SOLUTION_AUTO) == kern and query(sid=_lib.PETIT_SOLUTION_AUTO) == 0
    assert run(sid=exact_id) == kern and query(sid=exact_id) == 0
    # MXFP4 needs no image
    assert run(hints=hm) == bad and query(hints=hm) == 0
    assert run(s=None) == shape
    assert run(c=None) == shape and run(a=None) == shape and run(b=None) == shape and run(gs=None) == shape and run(off=None) == shape
    # the workspace: the rules of petit_gemm_native_moe
    assert run(ws=None, ws_bytes=0) == kern
    assert run(ws_bytes=need - 1) == kern and run(ws_bytes=8 * per) == kern
    assert run(ws=C.c_void_p(p.value + 16)) == bad
    assert run(native=na(8), ws_bytes=8 * per - 1) == kern                               # pre-quantised a: the images still need their room
    # the shape limits of the plan and of the image
    assert run(E=0) == shape and run(E=_lib.PETIT_MOE_MAX_EXPERTS + 1) == shape and query(E=0) == 0
    assert run(n=24) == shape and run(k=384) == shape and query(n=24) == 0 and query(k=384) == 0
    assert run(n=1 << 20, k=8192) == shape and query(n=1 << 20, k=8192) == 0             # an element part of 2^32 bytes or more
    assert run(a_idx=p, native=na(8)) == bad and run(native=na(0, 8)) == bad and run(c_idx=p, epi=C.byref(silu), native=na(0, 8)) == bad
    assert run(n=256, epi=C.byref(silu), native=na(0, 8)) == shape
    assert run(native=C.byref(_lib.NativeArgs(C.sizeof(_lib.NativeArgs), 5, 0, 0))) == bad
    assert run(a_rows=255) == shape and run(c_rows=255) == shape
    assert run(b=C.c_void_p(p.value + 4)) == bad
    assert run(m=0) == ok and run(m=0, ws=None, ws_bytes=0) == ok and query(m=0) == 0
    # the builder's own entry points
    assert L.petit_nvfp4_native_images(p, p, p, 0, 256, 32, None, 0, None) == shape
    assert L.petit_nvfp4_native_images(p, p, p, _lib.PETIT_MOE_MAX_EXPERTS + 1, 256, 32, None, 0, None) == shape
    assert L.petit_nvfp4_native_images(p, p, p, 4, 384, 32, None, 0, None) == shape and L.petit_nvfp4_native_images(p, p, p, 4, 256, 24, None, 0, None) == shape
    assert L.petit_nvfp4_native_images(None, p, p, 4, 256, 32, None, 0, None) == bad
    assert L.petit_nvfp4_native_images(C.c_void_p(p.value + 16), p, p, 4, 256, 32, None, 0, None) == bad
    assert L.petit_nvfp4_native_images(p, p, p, 4, 256, 32, p, 0, None) == ok            # offsets over no rows: nothing to build
    assert L.petit_nvfp4_native_images_host(p, p, p, 0, 256, 32, None, 0) == shape and L.petit_nvfp4_native_images_host(p, None, p, 4, 256, 32, None, 0) == bad


def _packed_bytes(E, n, k, seed):
    """Random bytes as the stacked packed tensors: every byte pattern is a packed tensor (NaN, negative and subnormal scales included)."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, E * n * k // 2, dtype=np.uint8), rng.integers(0, 256, E * n * k // 16, dtype=np.uint8)


def _per_expert_host(b, s, E, n, k):
    """E calls of petit_nvfp4_native_image_host: [E, I] uint8."""
    L = _L().lib
    per = int(L.petit_nvfp4_native_image_bytes(k, n))
    out = np.zeros((E, per), np.uint8)
    for e in range(E):
        be, se = np.ascontiguousarray(b[e * n * k // 2:(e + 1) * n * k // 2]), np.ascontiguousarray(s[e * n * k // 16:(e + 1) * n * k // 16])
        assert L.petit_nvfp4_native_image_host(out[e].ctypes.data, be.ctypes.data, se.ctypes.data, k, n) == 0
    return out


_HOST_IMAGES = {}


def _host_case(E, n, k):
    key = (E, n, k)
    if key not in _HOST_IMAGES:
        b, s = _packed_bytes(E, n, k, 1000 * n + k)
        want = _per_expert_host(b, s, E, n, k)
        want.setflags(write=False)
        _HOST_IMAGES[key] = (b, s, want)
    return _HOST_IMAGES[key]


@pytest.mark.parametrize("n,k", [(48, 768), (32, 256)])
def test_images_host_equals_per_expert_twin(n, k):
    E = 5
    b, s, want = _host_case(E, n, k)
    got = np.full((E, want.shape[1]), POISON, np.uint8)
    assert _L().lib.petit_nvfp4_native_images_host(got.ctypes.data, b.ctypes.data, s.ctypes.data, E, k, n, None, 0) == 0
    assert np.array_equal(got, want)


@pytest.mark.parametrize("offsets,m", SKIP_ROUTINGS, ids=[str(i) for i in range(len(SKIP_ROUTINGS))])
@pytest.mark.parametrize("n,k", [(48, 768), (32, 256)])
def test_images_host_skips_experts_without_rows(n, k, offsets, m):
    E = 5
    b, s, want = _host_case(E, n, k)
    got = np.full((E, want.shape[1]), POISON, np.uint8)
    off = np.array(offsets, np.int32)
    assert _L().lib.petit_nvfp4_native_images_host(got.ctypes.data, b.ctypes.data, s.ctypes.data, E, k, n, off.ctypes.data, m) == 0
    for e, active in enumerate(_has_rows(offsets, m)):
        if active:
            assert np.array_equal(got[e], want[e]), f"expert {e}"
        else:
            assert (got[e] == POISON).all(), f"expert {e} has no rows and was written"


def test_op_meta_shapes():
    import petit_kernel  # noqa: F401
    from petit_kernel import compiled
    if not compiled.available():
        pytest.skip(compiled.why_unavailable())
    ops = torch.ops.petit_kernel
    L = _L().lib
    E, n, k, m = 8, 1024, 512, 12
    a = torch.empty(5, k, dtype=torch.bfloat16, device="meta")
    b = torch.empty(E * n * k // 2, dtype=torch.uint8, device="meta")
    s = torch.empty(E * n * k // 16, dtype=torch.uint8, device="meta")
    gs = torch.empty(E, dtype=torch.float32, device="meta")
    off = torch.empty(E + 1, dtype=torch.int32, device="meta")
    idx = torch.empty(m, dtype=torch.int32, device="meta")
    c = ops.mul_nvfp4_native_moe_transient(a, b, s, gs, off, m, n, k, E, idx, None, -1, -2, None, 1)
    assert c.shape == (m, n // 2) and c.dtype == torch.bfloat16 and c.device.type == "meta"
    c = ops.mul_nvfp4_native_moe_transient(a.half(), b, s, gs, off, m, n, k, E, None, idx, 40, -3, None, 0)
    assert c.shape == (40, n) and c.dtype == torch.float16
    for f in (8, 6, 4):
        c = ops.mul_nvfp4_native_moe_transient(a, b, s, gs, off, m, n, k, E, idx, None, -1, -2, None, 2, 0, 5, f)
        assert c.shape == (int(L.petit_quantized_activation_bytes(m, n // 2, f)),) and c.dtype == torch.uint8
        qa = torch.empty(int(L.petit_quantized_activation_bytes(m, k, f)), dtype=torch.uint8, device="meta")
        c = ops.mul_nvfp4_native_moe_transient(qa, b, s, gs, off, m, n, k, E, None, idx, 30, -2, None, 0, f, 4, 0)
        assert c.shape == (30, n) and c.dtype == torch.float16


def test_layers_refuse_transient_mxfp4():
    import petit_kernel as pk
    t = torch.empty(0)
    with pytest.raises(RuntimeError, match="transient"):
        pk.fp4_moe_native(t, t, t, t, t, t, t, t, t, kind="mxfp4", transient=True)
    with pytest.raises(RuntimeError, match="transient"):
        pk.fp4_moe_routed(t, t, t, t, t, t, t, t, 2, "mxfp4", path="native", transient=True)
    with pytest.raises(RuntimeError, match="transient"):
        pk.fp4_moe_routed(t, t, t, t, t, t, t, t, 2, "nvfp4", path="fused", transient=True)


# --- on the GPU -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pk():
    import petit_kernel
    assert torch.cuda.is_available()
    assert torch.cuda.get_device_properties(0).gcnArchName.startswith("gfx950")
    return petit_kernel


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _offsets_dev(counts):
    return torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(DEV)


def _bits(t):
    return (t.data if hasattr(t, "fmt") else t).contiguous().view(torch.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [256, 512, 1024])       # span sizes 2 / 4 / 8
@pytest.mark.parametrize("n", [32, 48, 272])          # one block; N % 32 == 16; several blocks with a half one at the end
def test_builder_equals_host_twin(pk, n, k):
    """One launch for E = 5 experts equals the per-expert host twin byte for byte; with a routing, the regions of experts without rows keep
    the poison; the guard behind the images is never written.  nvfp4_native_images (now that one launch) equals nvfp4_native_image per expert."""
    L = _L().lib
    E = 5
    b, s, want = _host_case(E, n, k)
    per = want.shape[1]
    guard = 4096
    bd, sd = torch.from_numpy(b).to(DEV), torch.from_numpy(s).to(DEV)
    want_d = torch.from_numpy(want.copy()).to(DEV)
    for offsets, m in [(None, 0)] + SKIP_ROUTINGS:
        buf = torch.full((E * per + guard,), POISON, dtype=torch.uint8, device=DEV)
        off = torch.tensor(offsets, dtype=torch.int32, device=DEV) if offsets is not None else None
        rc = L.petit_nvfp4_native_images(buf.data_ptr(), bd.data_ptr(), sd.data_ptr(), E, k, n, off.data_ptr() if off is not None else None, m, _stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert (buf[E * per:] == POISON).all(), "guard region written"
        got = buf[:E * per].view(E, per)
        for e, active in enumerate(_has_rows(offsets, m) if offsets is not None else [True] * E):
            if active:
                assert torch.equal(got[e], want_d[e]), f"expert {e}, offsets {offsets}"
            else:
                assert (got[e] == POISON).all(), f"expert {e} has no rows and was written, offsets {offsets}"
    images = pk.nvfp4_native_images(bd, sd, E, n, k)
    for e in range(E):
        one = pk.nvfp4_native_image(bd[e * n * k // 2:(e + 1) * n * k // 2], sd[e * n * k // 16:(e + 1) * n * k // 16], n, k)
        assert torch.equal(images[e * per:(e + 1) * per], one), f"expert {e}"


def _many_expert_routings(E, seed):
    """(offsets, m) for many experts: a sparse well-formed routing, and a malformed one -- an early offset far ahead of its successors (the
    experts behind it stay without rows until the offsets pass it: a running maximum that crosses the kernel's 64-offset chunks), a negative
    offset, an offset beyond m, and empty experts at the end."""
    rng = np.random.default_rng(seed)
    counts = np.where(rng.random(E) < 0.3, rng.integers(1, 6, E), 0)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    m = int(off[-1])
    bad = off.copy()
    bad[3] = off[85]                                 # (E > 100)
    bad[E // 2] = -7
    tail = E - E // 5
    bad[tail - 1] = m + 1000
    bad[tail:] = off[tail - 1]
    return [(off.tolist(), m), (bad.tolist(), m)]


def _check_builder(E, n, k, routings, seed):
    """petit_nvfp4_native_images on a poisoned buffer with a guard behind it, for each (offsets, m): the experts with rows equal the host twin of
    their slice, the others keep the poison.  The host twin is computed for the experts some routing needs."""
    L = _L().lib
    per = int(L.petit_nvfp4_native_image_bytes(k, n))
    wb, sb = n * k // 2, n * k // 16
    b, s = _packed_bytes(E, n, k, seed)
    bd, sd = torch.from_numpy(b).to(DEV), torch.from_numpy(s).to(DEV)
    host = {}
    guard = 4096
    for offsets, m in routings:
        active = _has_rows(offsets, m) if offsets is not None else [True] * E
        buf = torch.full((E * per + guard,), POISON, dtype=torch.uint8, device=DEV)
        off = torch.tensor(offsets, dtype=torch.int32, device=DEV) if offsets is not None else None
        rc = L.petit_nvfp4_native_images(buf.data_ptr(), bd.data_ptr(), sd.data_ptr(), E, k, n, off.data_ptr() if off is not None else None, m, _stream())
        assert rc == 0
        got = buf.cpu().numpy()
        assert (got[E * per:] == POISON).all(), "guard region written"
        got = got[:E * per].reshape(E, per)
        for e in range(E):
            if not active[e]:
                assert (got[e] == POISON).all(), f"expert {e} has no rows and was written"
                continue
            if e not in host:
                host[e] = np.zeros(per, np.uint8)
                be, se = np.ascontiguousarray(b[e * wb:(e + 1) * wb]), np.ascontiguousarray(s[e * sb:(e + 1) * sb])
                assert L.petit_nvfp4_native_image_host(host[e].ctypes.data, be.ctypes.data, se.ctypes.data, k, n) == 0
            assert np.array_equal(got[e], host[e]), f"expert {e} differs from the host twin"
    return routings


@pytest.mark.gpu
@pytest.mark.parametrize("E", [256, 130])
def test_builder_skip_with_more_than_64_experts(pk, E):
    """One item per expert (n = 32, k = 256), more experts than one 64-offset chunk of the kernel's running maximum (E = 130: a last chunk of
    two): every expert, a sparse routing, and malformed offsets whose running maximum carries from the first chunk into the later ones."""
    routings = _many_expert_routings(E, E)
    for offsets, m in routings:
        active = _has_rows(offsets, m)
        assert any(active[:64]) and any(active[64:]) and not all(active[64:])
    bad = routings[1][0]
    assert bad[3] > max(bad[4:70]) and not any(_has_rows(bad, routings[1][1])[3:70])          # the early offset shadows a chunk boundary
    _check_builder(E, 32, 256, [(None, 0)] + routings, 11 + E)


@pytest.mark.gpu
def test_builder_skip_when_waves_carry_state_over_items(pk):
    """More items than the launch has waves (E = 256 experts of 39 items each: 9984 items, where the grid is capped at 8 workgroups of 4 waves
    per CU), so a wave runs several items of different experts and carries its running maximum from one to the next, over more than one
    64-offset chunk: a sparse routing and the malformed one (a decreasing offset early, empty experts late)."""
    E, n, k = 256, 96, 3328
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert E * (n // 32) * (k // 256) > cus * 8 * 4
    _check_builder(E, n, k, _many_expert_routings(E, 7), 5)


_EXPERTS = {}


def _experts(pk, E, n, k):
    """(Experts, resident images, bias [E, n] per dtype), built once per shape and left unchanged."""
    key = (E, n, k)
    if key not in _EXPERTS:
        ex = Experts(pk, "nv", E, n, k, 500 + k, gs_scale=0.05)
        g = torch.Generator(device=DEV).manual_seed(k)
        bias = torch.randn(E, n, device=DEV, generator=g) * 0.5
        _EXPERTS[key] = (ex, pk.nvfp4_native_images(ex.b, ex.sp, E, n, k), bias)
    return _EXPERTS[key]


def _routings(m, E):
    even = [m // E + (1 if e < m % E else 0) for e in range(E)]                                   # every expert active (as far as m rows go)
    half = [0] * E
    for i in range(m):
        half[1 + 2 * (i % (E // 2))] += 1                                                         # the even experts empty
    one = [0] * E
    one[E - 3] = m
    out = [even, half, one]
    if m == 300:
        out.append([0, 1, 129, 0, 130, 40, 0, 0])                                                 # ragged: counts that straddle 128-row tiles
    return out


def _both(pk, ex, images, a, off, m, n, k, E, sid, **kw):
    got = pk.mul_nvfp4_native_moe_transient(a, ex.b, ex.sp, ex.gsd, off, m, n, k, E, solution_id=sid, **kw)
    want = pk.mul_nvfp4_native_moe(a, images, ex.gsd, off, m, n, k, E, solution_id=sid, **kw)
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp6", "mxfp4"])
@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("m", [1, 33, 300])
@pytest.mark.parametrize("k", [512, 2048])
def test_transient_equals_resident(pk, k, m, is_bf16, fmt):
    """Bit for bit mul_nvfp4_native_moe on nvfp4_native_images of the same tensors: every epilogue (plain, bias, SiLU-mul and SwiGLU-OAI with and
    without the quantised output), 16-bit a through a_row_index with indices out of range, pre-quantised a, the C scatter."""
    E, n = 8, 512
    ex, images, bias32 = _experts(pk, E, n, k)
    dt = torch.bfloat16 if is_bf16 else torch.float16
    bias = bias32.to(dt)
    sid = SENTINEL[fmt]
    g = torch.Generator(device=DEV).manual_seed(m + k)
    a_rows = m + 7
    src = torch.randn(a_rows, k, device=DEV, generator=g).to(dt)
    a_idx = torch.randint(0, a_rows, (m,), device=DEV, generator=g, dtype=torch.int32)
    a_idx[0] = a_rows + 5                                                                         # out of range: a zero row
    if m > 2:
        a_idx[m // 2] = -1
    a = src[:m].contiguous()
    qa = pk.quantize_activations(a, fmt)
    perm = torch.randperm(m, device=DEV, generator=g).to(torch.int32)
    forms = [
        ("plain", a, {}),
        ("bias, gathered a", src, dict(bias=bias, a_row_index=a_idx)),
        ("quantised a, scattered c", qa, dict(c_row_index=perm, c_rows=m)),
        ("silu_mul", a, dict(activation="silu_mul")),
        ("silu_mul, quantised a and out", qa, dict(activation="silu_mul", out_quantized=fmt)),
        ("swiglu_oai, bias", a, dict(activation="swiglu_oai", bias=bias)),
        ("swiglu_oai, gathered a, quantised out", src, dict(activation="swiglu_oai", a_row_index=a_idx, out_quantized=fmt)),
    ]
    for counts in _routings(m, E):
        off = _offsets_dev(counts)
        for name, a_in, kw in forms:
            got, want = _both(pk, ex, images, a_in, off, m, n, k, E, sid, **kw)
            assert torch.equal(_bits(got), _bits(want)), f"{name}, counts {counts}"


@pytest.mark.gpu
@pytest.mark.parametrize("k", [512, 768, 2048])       # span sizes 4 / 2 / 8: each has its own MoE forms
def test_transient_every_explicit_native_id(pk, k):
    """Every explicit native id of the NVFP4 family that native_moe_resolve_solution accepts for the problem runs transient as on the images."""
    E, n, m = 8, 512, 300
    ex, images, _ = _experts(pk, E, n, k)
    h = _hints(pk, "nv", True)
    pk.ops.enable_native_fp4(True)
    try:
        listed = [sid for sid in pk.ops.get_fp4_solutions(h, m, n, k) if (sid >> 48) & 0xF == 13]
    finally:
        pk.ops.enable_native_fp4(False)
    accepted = [sid for sid in listed if pk.native_moe_resolve_solution(h, E, m, n, k, sid) == sid]
    assert len(accepted) >= 3, [hex(x) for x in listed]                                           # one per activation format at least
    a = torch.randn(m, k, device=DEV, generator=torch.Generator(device=DEV).manual_seed(k)).bfloat16()
    off = _offsets_dev([0, 1, 129, 0, 130, 40, 0, 0])
    for sid in accepted:
        got, want = _both(pk, ex, images, a, off, m, n, k, E, sid)
        assert torch.equal(_bits(got), _bits(want)), hex(sid)
        got, want = _both(pk, ex, images, a, off, m, n, k, E, sid, activation="silu_mul")
        assert torch.equal(_bits(got), _bits(want)), hex(sid)


def _raw_transient(_lib, ex, c, a, off, m, n, k, E, ws, ws_bytes):
    h = _nv_hints(_lib)
    return _lib.lib.petit_gemm_native_moe_transient(c.data_ptr(), a.data_ptr(), ex.b.data_ptr(), ex.sp.data_ptr(), ex.gsd.data_ptr(), off.data_ptr(), E, m,
                                                    n, k, None, m, None, m, C.byref(h), C.c_uint64(_lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP8), None, None,
                                                    ws.data_ptr(), C.c_uint64(ws_bytes), _stream())


@pytest.mark.gpu
def test_workspace_contents_exact_size_and_sharing(pk):
    """After a call the image part of the workspace holds the images of the experts with rows and nothing else; a workspace of exactly the
    queried size runs, one byte less is refused with C and the workspace untouched; two layers' calls share one buffer."""
    _lib = _L()
    E, n, k, m = 8, 512, 2048, 300
    ex, images, _ = _experts(pk, E, n, k)
    per = images.numel() // E
    counts = [0, 1, 129, 0, 130, 40, 0, 0]
    off = _offsets_dev(counts)
    a = torch.randn(m, k, device=DEV).bfloat16()
    need = pk.nvfp4_native_moe_transient_workspace_bytes(E, m, n, k)
    assert need == E * per + m * (k + k // 32)
    ws = torch.full((need,), POISON, dtype=torch.uint8, device=DEV)
    c = torch.zeros(m, n, dtype=torch.bfloat16, device=DEV)
    assert _raw_transient(_lib, ex, c, a, off, m, n, k, E, ws, need) == 0
    want = pk.mul_nvfp4_native_moe(a, images, ex.gsd, off, m, n, k, E)
    assert torch.equal(c.view(torch.int16), want.view(torch.int16))
    for e in range(E):
        region = ws[e * per:(e + 1) * per]
        if counts[e]:
            assert torch.equal(region, images[e * per:(e + 1) * per]), f"expert {e}"
        else:
            assert (region == POISON).all(), f"expert {e} has no rows and its image region was written"
    # one byte less: refused before the first launch
    ws2 = torch.full((need,), POISON, dtype=torch.uint8, device=DEV)
    c2 = torch.zeros_like(c)
    assert _raw_transient(_lib, ex, c2, a, off, m, n, k, E, ws2, need - 1) == _lib.PETIT_ERROR_KERNEL_SHAPE
    torch.cuda.synchronize()
    assert torch.count_nonzero(c2) == 0 and (ws2 == POISON).all()
    # a second layer (other weights, every expert active) on the same buffer, then the first again: each its own result
    ex_b = Experts(pk, "nv", E, n, k, 777, gs_scale=0.05)
    images_b = pk.nvfp4_native_images(ex_b.b, ex_b.sp, E, n, k)
    off_b = _offsets_dev(_routings(m, E)[0])
    c_b, c_a = torch.zeros_like(c), torch.zeros_like(c)
    assert _raw_transient(_lib, ex_b, c_b, a, off_b, m, n, k, E, ws, need) == 0
    assert _raw_transient(_lib, ex, c_a, a, off, m, n, k, E, ws, need) == 0
    assert torch.equal(c_b.view(torch.int16), pk.mul_nvfp4_native_moe(a, images_b, ex_b.gsd, off_b, m, n, k, E).view(torch.int16))
    assert torch.equal(c_a.view(torch.int16), want.view(torch.int16))
    # the operator layers take the caller's workspace too: both write their images into it, and refuse one below the query
    for layer in (pk.ops, pk.compiled):
        ws3 = torch.full((need + 256,), POISON, dtype=torch.uint8, device=DEV)
        got = layer.mul_nvfp4_native_moe_transient(a, ex.b, ex.sp, ex.gsd, off, m, n, k, E, workspace=ws3)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), layer.__name__
        assert torch.equal(ws3[2 * per:3 * per], images[2 * per:3 * per]) and (ws3[:per] == POISON).all() and (ws3[need:] == POISON).all()
        with pytest.raises(RuntimeError, match="workspace"):
            layer.mul_nvfp4_native_moe_transient(a, ex.b, ex.sp, ex.gsd, off, m, n, k, E, workspace=ws3[:need - 256])


@pytest.mark.gpu
def test_graph_replay_follows_routing_and_weights(pk):
    """A captured transient call reads expert_offsets, b and scales at every replay: a formerly empty expert that gets rows gets its image,
    and overwritten weights are the ones computed with."""
    E, n, k, m = 8, 512, 512, 64
    ex1 = Experts(pk, "nv", E, n, k, 901, gs_scale=0.05)
    ex2 = Experts(pk, "nv", E, n, k, 902, gs_scale=0.05)
    b, sp = ex1.b.clone(), ex1.sp.clone()
    a = torch.randn(m, k, device=DEV).bfloat16()
    off1 = _offsets_dev([0, 30, 0, 0, 34, 0, 0, 0])
    off2 = _offsets_dev([10, 0, 20, 5, 0, 9, 0, 20])
    off = off1.clone()

    def fresh(ex, o):
        return pk.mul_nvfp4_native_moe(a, pk.nvfp4_native_images(ex.b, ex.sp, E, n, k), ex1.gsd, o, m, n, k, E, activation="silu_mul")

    def call():
        return pk.mul_nvfp4_native_moe_transient(a, b, sp, ex1.gsd, off, m, n, k, E, activation="silu_mul")

    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        call()                                                        # warm-up outside the capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            out = call()
        g.replay()
        st.synchronize()
        assert torch.equal(_bits(out), _bits(fresh(ex1, off1)))
        off.copy_(off2)
        g.replay()
        st.synchronize()
        assert torch.equal(_bits(out), _bits(fresh(ex1, off2)))
        b.copy_(ex2.b)
        sp.copy_(ex2.sp)
        g.replay()
        st.synchronize()
        assert torch.equal(_bits(out), _bits(fresh(ex2, off2)))
        assert not torch.equal(_bits(fresh(ex1, off2)), _bits(fresh(ex2, off2)))
    torch.cuda.current_stream().wait_stream(st)


@pytest.mark.gpu
@pytest.mark.parametrize("inter", [256, 512])
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4"])
def test_layers_equal_the_resident_image_layers(pk, fmt, inter):
    """fp4_moe_native(transient=True) on the packed tensors equals the resident-image layer on nvfp4_native_images of them, with unrouted (-1)
    ids; fp4_moe_routed(transient=True) likewise, through an expert map that sends some experts away and with a shared expert."""
    E, hid, T, topk = 8, 512, 33, 2
    w13, w2 = _make_layer(pk, "nv", E, hid, inter, 300 + inter)
    i13, i2 = pk.nvfp4_native_images(w13.b, w13.sp, E, w13.n, w13.k), pk.nvfp4_native_images(w2.b, w2.sp, E, w2.n, w2.k)
    x = torch.randn(T, hid, device=DEV).bfloat16()
    tw, ids = _routing(T, E, topk, 5)
    ids[::4, 1] = -1
    ids[ids == 6] = 2                                                                             # expert 6 gets no rows
    tw, ids = tw.to(DEV), ids.to(DEV)
    got = pk.fp4_moe_native(x, w13.b, w13.sp, w13.gsd, w2.b, w2.sp, w2.gsd, tw, ids, kind="nvfp4", activations=fmt, transient=True)
    want = pk.fp4_moe_native(x, i13, None, w13.gsd, i2, None, w2.gsd, tw, ids, kind="nvfp4", activations=fmt)
    assert got.shape == (T, hid) and torch.equal(got.view(torch.int16), want.view(torch.int16))
    # the layer's two launches run on ONE scratch: what a call allocates at its peak stays below two scratches plus the resident layer's own
    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before
    p_res = peak(lambda: pk.fp4_moe_native(x, i13, None, w13.gsd, i2, None, w2.gsd, tw, ids, kind="nvfp4", activations=fmt))
    p_tr = peak(lambda: pk.fp4_moe_native(x, w13.b, w13.sp, w13.gsd, w2.b, w2.sp, w2.gsd, tw, ids, kind="nvfp4", activations=fmt, transient=True))
    m = T * topk
    one = max(pk.nvfp4_native_moe_transient_workspace_bytes(E, m, 2 * inter, hid, SENTINEL[fmt], a_format=fmt, activation="silu_mul", out_quantized=fmt),
              pk.nvfp4_native_moe_transient_workspace_bytes(E, m, hid, inter, SENTINEL[fmt], a_format=fmt))
    assert one >= max(i13.numel(), i2.numel())
    assert p_tr <= p_res + one + (1 << 20), (p_tr, p_res, one)                                    # (allocator rounding: 512-byte blocks)
    # routed: 10 global experts, 7 of them local (3 sent away: -1 ids), then one shared expert -- 8 stacked experts
    emap = torch.tensor([0, -1, 1, 2, -1, 3, 4, 5, -1, 6], dtype=torch.int32, device=DEV)
    logits = torch.randn(T, 10, device=DEV)
    kw = dict(path="native", activations=fmt, expert_map=emap, num_local_experts=7, num_shared=1)
    got = pk.fp4_moe_routed(x, logits, w13.b, w13.sp, w13.gsd, w2.b, w2.sp, w2.gsd, topk, "nvfp4", transient=True, **kw)
    want = pk.fp4_moe_routed(x, logits, i13, None, w13.gsd, i2, None, w2.gsd, topk, "nvfp4", **kw)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))

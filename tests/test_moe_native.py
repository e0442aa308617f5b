"""The native-class MoE launch: petit_gemm_native_moe / mul_*_native_moe (routed experts on the block-scaled MFMA, activations quantised
to MXFP8 / MXFP6 / MXFP4), the gathering quantiser (petit_quantize_activations_rows / quantize_activation_rows) and fp4_moe_native.

Unmarked tests run without a GPU (argument checks and queries of the C ABI, Meta shapes of the torch ops); the @pytest.mark.gpu ones check
bit-identity per expert with the dense native call of the same id, the gathering quantiser against quantize_activations of torch-gathered
rows, the quantising epilogue's row limit, the C scatter, one oracle call per activation format, and the whole layer (stages, graph replay,
a loose comparison with the exact fused layer).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gpu_parity import native_exact_bound, native_p99_guard, quantize_act_mxfp4, quantize_act_mxfp6, quantize_act_mxfp8
from test_moe import Experts, _hints, _make_layer, _routing

DEV = "cuda"
FMTS = {"mxfp8": 8, "mxfp6": 6, "mxfp4": 4}
SENTINEL = {"mxfp8": -2, "mxfp4": -3, "mxfp6": -4}


def _aligned(buf, align=256):
    return C.c_void_p((C.addressof(buf) + align - 1) & ~(align - 1))


def _ws_bytes(fmt, m, k):
    return m * (k // 8 * FMTS[fmt]) + m * (k // 32)


# --- without a GPU ----------------------------------------------------------------------------------------------------------------

def test_native_moe_abi_argument_checks_without_a_gpu():
    from petit_kernel import _lib
    L = _lib.lib
    buf = (C.c_uint8 * 8192)()
    p = _aligned(buf)
    shape, kern, bad, ok = _lib.PETIT_ERROR_PROBLEM_SHAPE, _lib.PETIT_ERROR_KERNEL_SHAPE, _lib.PETIT_ERROR_BAD_ARGUMENT, _lib.PETIT_OK
    s8 = _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP8
    h = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_MXFP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
    silu = _lib.Epilogue(None, 1, 0)

    def na(a_fmt=0, out_fmt=0):
        return C.byref(_lib.NativeArgs(C.sizeof(_lib.NativeArgs), a_fmt, out_fmt, 0))

    # every call below is refused before anything is launched (or is empty): the pointers are host scratch
    def run(E=8, m=256, n=512, k=256, c=p, a=p, b=p, s=p, gs=p, off=p, a_idx=None, a_rows=256, c_idx=None, c_rows=256, sid=s8, epi=None,
            native=None, ws=p, ws_bytes=0, hints=h):
        return L.petit_gemm_native_moe(c, a, b, s, gs, off, E, m, n, k, a_idx, a_rows, c_idx, c_rows, C.byref(hints), C.c_uint64(sid), epi, native,
                                       ws, C.c_uint64(ws_bytes), None)

    assert run(c=None) == shape and run(a=None) == shape and run(b=None) == shape and run(s=None) == shape
    assert run(gs=None) == shape and run(off=None) == shape
    assert run(E=0) == shape and run(E=_lib.PETIT_MOE_MAX_EXPERTS + 1) == shape
    assert run(n=24) == shape and run(k=384) == shape
    # never another accuracy class: PETIT_SOLUTION_AUTO and exact-class ids are refused
    exact_id = L.petit_gemm_moe_resolve_solution(C.byref(h), 8, 256, 512, 256, C.c_uint64(_lib.PETIT_SOLUTION_AUTO), None)
    assert exact_id != 0
    assert run(sid=_lib.PETIT_SOLUTION_AUTO) == kern and run(sid=exact_id) == kern
    # option combinations
    assert run(a_idx=p, native=na(8)) == bad                                             # quantised rows are grouped already
    assert run(c_idx=p, epi=C.byref(silu), native=na(0, 8)) == bad                       # the quantised output is identity-only
    assert run(native=na(0, 8)) == bad                                                   # ... and the SiLU-mul epilogue's
    assert run(n=256, epi=C.byref(silu), native=na(0, 8)) == shape                       # n % 512
    assert run(native=C.byref(_lib.NativeArgs(C.sizeof(_lib.NativeArgs), 5, 0, 0))) == bad
    assert run(a_rows=255) == shape and run(c_rows=255) == shape                         # a null index is the identity
    # the workspace: the query is the quantised rows of the class's format; below it, refused as the dense native entry points refuse it
    for fmt, sid in SENTINEL.items():
        need = L.petit_gemm_native_moe_workspace_bytes(C.byref(h), 8, 256, 512, 256, C.c_uint64(_sid(_lib, sid)), None, None)
        assert need == _ws_bytes(fmt, 256, 256), fmt
        assert L.petit_gemm_native_moe_workspace_bytes(C.byref(h), 8, 256, 512, 256, C.c_uint64(_sid(_lib, sid)), None, na(FMTS[fmt])) == 0
        assert run(sid=_sid(_lib, sid), ws_bytes=need - 1) == kern
        assert run(sid=_sid(_lib, sid), ws=None, ws_bytes=0) == kern
    assert run(native=na(4)) == kern                                                     # MXFP4 rows, MXFP8 class
    assert run(ws=C.c_void_p(p.value + 16), ws_bytes=1 << 20) == bad                     # 256-byte aligned scratch
    assert run(m=0) == ok and run(m=0, ws=None) == ok
    # NVFP4: b is the images (256-byte aligned), scales are not read
    hn = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
    assert run(hints=hn, m=0, s=None) == ok
    assert run(hints=hn, b=C.c_void_p(p.value + 16), s=None, ws_bytes=1 << 20) == bad

    q = L.petit_quantize_activations_rows
    assert q(p, p, None, 4, 0, 256, _lib.CXX_DTYPE_BF16, 8, None) == ok
    assert q(None, p, None, 4, 4, 256, _lib.CXX_DTYPE_BF16, 8, None) == bad
    assert q(p, p, None, 4, 4, 384, _lib.CXX_DTYPE_BF16, 8, None) == shape
    assert q(p, p, None, 3, 4, 256, _lib.CXX_DTYPE_BF16, 8, None) == shape               # identity needs a_rows >= m
    assert q(p, p, p, 1, 1 << 22, 1 << 10, _lib.CXX_DTYPE_BF16, 8, None) == shape        # 2^32 bytes of output: 32-bit offsets


def _sid(_lib, py_sid):
    return {-2: _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP8, -3: _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP4, -4: _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP6}[py_sid]


@pytest.mark.parametrize("kind", ["mx", "nv"])
def test_native_moe_forms_resolve_without_a_gpu(kind):
    """Every activation format has a MoE form at every span size (k % 256 == 0), with and without the quantising epilogue; a resolved id
    resolves to itself as an explicit id, is a 32x32x64 native kernel of the named class, and refused problems resolve to 0."""
    import petit_kernel as pk
    h = _hints(pk, kind, True)
    mfma = {"mxfp8": 2, "mxfp6": 4, "mxfp4": 6}
    for k in (256, 512, 768, 1024, 1536, 2048, 7168):
        for fmt, sid in SENTINEL.items():
            for m, E in ((1, 8), (64, 128), (4096, 8), (131072, 256)):
                got = pk.native_moe_resolve_solution(h, E, m, 1024, k, sid)
                assert got != 0, (k, fmt, m, E)
                assert (got >> 48) & 0xF == 13 and (got >> 32) & 0x7 == mfma[fmt]
                assert pk.native_moe_resolve_solution(h, E, m, 1024, k, got) == got
                assert pk.native_moe_resolve_solution(h, E, m, 1024, k, sid, activation="silu_mul", out_quantized=fmt) == got
                assert pk.native_moe_resolve_solution(h, E, m, 1024, k, sid, a_format=fmt) == got
            assert pk.native_moe_resolve_solution(h, 8, 64, 1024, k, sid, a_format="mxfp8" if fmt != "mxfp8" else "mxfp4") == 0
    assert pk.native_moe_resolve_solution(h, 8, 64, 1024, 2048, -1) == 0
    assert pk.native_moe_resolve_solution(h, 0, 64, 1024, 2048, -2) == 0
    assert pk.native_moe_resolve_solution(h, 8, 0, 1024, 2048, -2) == 0
    assert pk.native_moe_resolve_solution(h, 8, 64, 1024, 384, -2) == 0


def test_native_moe_ops_meta_shapes():
    import petit_kernel  # noqa: F401
    from petit_kernel import compiled
    assert compiled.available(), compiled.why_unavailable()
    ops = torch.ops.petit_kernel
    E, n, k, m = 8, 1024, 512, 12
    a = torch.empty(5, k, dtype=torch.bfloat16, device="meta")
    b = torch.empty(E * n * k // 2, dtype=torch.uint8, device="meta")
    s = torch.empty(E * n * k // 32, dtype=torch.uint8, device="meta")
    gs = torch.empty(E, dtype=torch.float32, device="meta")
    off = torch.empty(E + 1, dtype=torch.int32, device="meta")
    idx = torch.empty(m, dtype=torch.int32, device="meta")
    c = ops.mul_mxfp4_native_moe(a, b, s, gs, off, m, n, k, E, idx, None, -1, -2, None, 1)
    assert c.shape == (m, n // 2) and c.dtype == torch.bfloat16 and c.device.type == "meta"
    c = ops.mul_mxfp4_native_moe(a.half(), b, s, gs, off, m, n, k, E, None, idx, 40, -3, None, 0)
    assert c.shape == (40, n) and c.dtype == torch.float16
    for fmt, f in FMTS.items():
        c = ops.mul_nvfp4_native_moe(a, b, None, gs, off, m, n, k, E, idx, None, -1, -2, None, 1, 0, 5, f)
        assert c.shape == (_ws_bytes(fmt, m, n // 2),) and c.dtype == torch.uint8
        qa = torch.empty(_ws_bytes(fmt, m, k), dtype=torch.uint8, device="meta")
        c = ops.mul_nvfp4_native_moe(qa, b, None, gs, off, m, n, k, E, None, idx, 30, -2, None, 0, f, 4, 0)
        assert c.shape == (30, n) and c.dtype == torch.float16


# --- on the GPU -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pk():
    import petit_kernel
    assert torch.cuda.is_available()
    assert torch.cuda.get_device_properties(0).gcnArchName.startswith("gfx950")
    return petit_kernel


def _u8(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy()


class NativeExperts:
    """Experts (test_moe) plus what the native calls read: NVFP4 weights as E native images back to back."""

    def __init__(self, pk, kind, E, n, k, seed):
        self.ex = Experts(pk, kind, E, n, k, seed, mx_band=(122, 127), gs_scale=0.05)
        self.kind, self.E, self.n, self.k = kind, E, n, k
        if kind == "nv":
            self.img = pk.nvfp4_native_images(self.ex.b, self.ex.sp, E, n, k)
            self.per = self.img.numel() // E

    def moe(self, pk, a, offsets, m, sid, **kw):
        if self.kind == "nv":
            return pk.mul_nvfp4_native_moe(a, self.img, self.ex.gsd, offsets, m, self.n, self.k, self.E, solution_id=sid, **kw)
        return pk.mul_mxfp4_native_moe(a, self.ex.b, self.ex.sp, self.ex.gsd, offsets, m, self.n, self.k, self.E, solution_id=sid, **kw)

    def dense(self, pk, a, e, sid, **kw):
        n, k, m = self.n, self.k, (a.m if hasattr(a, "m") else a.shape[0])
        if self.kind == "nv":
            return pk.mul_nvfp4_native(a, self.img[e * self.per:(e + 1) * self.per], self.ex.gsd[e:e + 1], m, n, k, sid, **kw)
        b = self.ex.b.view(-1)[e * n * k // 8:(e + 1) * n * k // 8].view(n // 16, 2 * k)
        s = self.ex.sp.view(-1)[e * n * k // 32:(e + 1) * n * k // 32].view(n // 32, k)
        return pk.mul_mxfp4_native(a, b, s, self.ex.gsd[e:e + 1], m, n, k, sid, **kw)


def _offsets_dev(counts):
    return torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(DEV)


def _rows_of(buf, m, K, f):
    """Quantised [m, K] bytes ("petit-qact/1", k-tile major) -> one row of bytes per activation row (a fixed re-layout)."""
    b = _u8(buf)
    kt = K // 128
    lo = 64 if f == 6 else 16 * f
    parts = [b[:kt * m * lo].reshape(kt, m, lo)]
    off = kt * m * lo
    if f == 6:
        parts.append(b[off:off + kt * m * 32].reshape(kt, m, 32))
        off += kt * m * 32
    parts.append(b[off:off + kt * m * 4].reshape(kt, m, 4))
    assert off + kt * m * 4 == b.size
    return np.concatenate([p.transpose(1, 0, 2).reshape(m, -1) for p in parts], axis=1)


# routings: empty experts, a one-row expert, counts not a multiple of 128, then every row on one expert
ROUTINGS = [[0, 1, 130, 0, 257, 40], [0, 0, 300, 0, 0, 0]]


@pytest.mark.gpu
@pytest.mark.parametrize("k,epi", [(2048, "plain"), (768, "silu_bias"), (512, "bias")])
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp6", "mxfp4"])
@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("kind", ["mx", "nv"])
def test_bit_identical_to_dense_native_per_expert(pk, kind, is_bf16, fmt, k, epi):
    """Each expert's rows equal, bit for bit, the dense native call with the same explicit id on that expert's rows (gathered in torch).
    k = 2048 / 512 / 768: span sizes 8 / 4 / 2 (768: Qwen3's down)."""
    E, n = 6, 512
    ne = NativeExperts(pk, kind, E, n, k, 7 + k)
    dt = torch.bfloat16 if is_bf16 else torch.float16
    act = "silu_mul" if epi.startswith("silu") else None
    bias = (torch.randn(E, n, device=DEV) * 0.5).to(dt) if "bias" in epi else None
    h = _hints(pk, kind, is_bf16)
    for counts in ROUTINGS:
        m = sum(counts)
        sid = pk.native_moe_resolve_solution(h, E, m, n, k, SENTINEL[fmt], activation=act)
        assert sid
        a = torch.randn(m, k, device=DEV).to(dt)
        off = _offsets_dev(counts)
        got = ne.moe(pk, a, off, m, sid, bias=bias, activation=act)
        assert torch.equal(got, ne.moe(pk, a, off, m, SENTINEL[fmt], bias=bias, activation=act))   # the sentinel picks the same id
        o = np.concatenate([[0], np.cumsum(counts)])
        for e in range(E):
            if counts[e] == 0:
                continue
            ref = ne.dense(pk, a[o[e]:o[e + 1]].contiguous(), e, sid, bias=bias[e].contiguous() if bias is not None else None, activation=act)
            assert torch.equal(got[o[e]:o[e + 1]].view(torch.int16), ref.view(torch.int16)), f"expert {e}, counts {counts}"


@pytest.mark.gpu
@pytest.mark.parametrize("is_bf16", [True, False])
def test_gathering_quantiser_equals_quantize_of_gathered_rows(pk, is_bf16):
    dt = torch.bfloat16 if is_bf16 else torch.float16
    a_rows, k = 200, 768
    a = (torch.randn(a_rows, k, device=DEV) * 3).to(dt)
    idx = torch.randint(0, a_rows, (333,), device=DEV, dtype=torch.int32)
    idx[[0, 17, 332]] = torch.tensor([-1, a_rows, 1 << 30], device=DEV, dtype=torch.int32)   # out of range: zero rows
    ok = (idx >= 0) & (idx < a_rows)
    gathered = torch.where(ok[:, None], a[idx.clamp(0, a_rows - 1).long()], torch.zeros((), dtype=dt, device=DEV)).contiguous()
    for fmt in FMTS:
        got = pk.quantize_activation_rows(a, fmt, idx)
        ref = pk.quantize_activations(gathered, fmt)
        assert got.m == 333 and got.k == k and np.array_equal(_u8(got.data), _u8(ref.data)), fmt
        zero = _rows_of(got.data, 333, k, FMTS[fmt])[0]
        assert (zero[-(k // 32):] == 127).all() and (zero[:-(k // 32)] == 0).all()
        assert np.array_equal(_u8(pk.quantize_activation_rows(a, fmt).data), _u8(pk.quantize_activations(a, fmt).data))


def _raw_native_moe(pk, ne, out, a, off, m, sid, c_idx=None, c_rows=None, act=0, out_fmt=0, a_fmt=0):
    """petit_gemm_native_moe into a caller's buffer (the sentinel tests): a is 16-bit rows (a_fmt 0) or quantised bytes."""
    from petit_kernel import _lib, ops
    dt = a.dtype if not a_fmt else torch.bfloat16
    at = _lib.CXX_DTYPE_BF16 if dt == torch.bfloat16 else _lib.CXX_DTYPE_FP16
    hints = _lib.SolutionHints(at, _lib.CXX_DTYPE_MXFP4_E2M1 if ne.kind == "mx" else _lib.CXX_DTYPE_FP4_E2M1, at, 0)
    epi = _lib.Epilogue(None, act, 0)
    na = _lib.NativeArgs(C.sizeof(_lib.NativeArgs), a_fmt, out_fmt, 0)
    sid = ops._c_solution_id(sid, native_ok=True)
    ws_bytes = _lib.lib.petit_gemm_native_moe_workspace_bytes(C.byref(hints), ne.E, m, ne.n, ne.k, C.c_uint64(sid), C.byref(epi) if act else None,
                                                              C.byref(na))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=DEV)
    b = ne.img if ne.kind == "nv" else ne.ex.b
    rc = _lib.lib.petit_gemm_native_moe(out.data_ptr(), a.data_ptr(), b.data_ptr(), ne.ex.sp.data_ptr() if ne.kind == "mx" else None,
                                        ne.ex.gsd.data_ptr(), off.data_ptr(), ne.E, m, ne.n, ne.k, None, m,
                                        c_idx.data_ptr() if c_idx is not None else None, c_rows if c_rows is not None else m, C.byref(hints),
                                        C.c_uint64(sid), C.byref(epi) if act else None, C.byref(na), ws.data_ptr(), C.c_uint64(ws_bytes),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.PETIT_OK, _lib.error_string(rc)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp6", "mxfp4"])
@pytest.mark.parametrize("kind", ["mx", "nv"])
def test_quantising_epilogue_per_expert_and_row_limit(pk, kind, fmt):
    """gate_up with out_quantized: each expert's grouped rows, re-laid out by row, equal the dense call's out_quantized bytes; rows past
    expert_offsets[E] (same tiles as the last expert's rows) keep a sentinel fill."""
    E, n, k = 6, 1024, 1024
    ne = NativeExperts(pk, kind, E, n, k, 31)
    counts = ROUTINGS[0]
    m = sum(counts)
    a = torch.randn(m, k, device=DEV).bfloat16()
    off = _offsets_dev(counts)
    sid = pk.native_moe_resolve_solution(_hints(pk, kind, True), E, m, n, k, SENTINEL[fmt], activation="silu_mul", out_quantized=fmt)
    assert sid
    got = ne.moe(pk, a, off, m, sid, activation="silu_mul", out_quantized=fmt)
    rows = _rows_of(got.data, m, n // 2, FMTS[fmt])
    o = np.concatenate([[0], np.cumsum(counts)])
    for e in range(E):
        if counts[e]:
            ref = ne.dense(pk, a[o[e]:o[e + 1]].contiguous(), e, sid, activation="silu_mul", out_quantized=fmt)
            assert np.array_equal(rows[o[e]:o[e + 1]], _rows_of(ref.data, counts[e], n // 2, FMTS[fmt])), f"expert {e}"
    # only the first 131 rows routed (expert 1: 1 row, expert 2: 130): rows 131.. share their tiles and must stay untouched
    part = torch.tensor([0, 0, 1, 131, 131, 131, 131], dtype=torch.int32, device=DEV)
    out = torch.full((got.data.numel(),), 0xA5, dtype=torch.uint8, device=DEV)
    _raw_native_moe(pk, ne, out, a, part, m, sid, act=1, out_fmt=FMTS[fmt])
    r2 = _rows_of(out, m, n // 2, FMTS[fmt])
    assert np.array_equal(r2[:131], rows[:131]) and (r2[131:] == 0xA5).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mx", "nv"])
def test_scattered_c_and_out_of_range_indices(pk, kind):
    E, n, k = 6, 512, 1024
    ne = NativeExperts(pk, kind, E, n, k, 41)
    counts = ROUTINGS[0]
    m = sum(counts)
    a = torch.randn(m, k, device=DEV).bfloat16()
    off = _offsets_dev(counts)
    plain = ne.moe(pk, a, off, m, -2)
    perm = torch.randperm(m, device=DEV).to(torch.int32)
    scat = ne.moe(pk, a, off, m, -2, c_row_index=perm, c_rows=m)
    assert torch.equal(scat[perm.long()].view(torch.int16), plain.view(torch.int16))
    silu_plain = ne.moe(pk, a, off, m, -2, activation="silu_mul")
    silu_scat = ne.moe(pk, a, off, m, -2, activation="silu_mul", c_row_index=perm, c_rows=m)
    assert torch.equal(silu_scat[perm.long()].view(torch.int16), silu_plain.view(torch.int16))
    # indices outside [0, c_rows) store nothing
    bad = perm.clone()
    bad[::7] = -1
    bad[3::11] = m + 5
    keep = (bad >= 0) & (bad < m)
    for act in (0, 1):
        out = torch.full((m, n // 2 if act else n), 1234.0, dtype=torch.bfloat16, device=DEV)
        _raw_native_moe(pk, ne, out, a, off, m, -2, c_idx=bad, c_rows=m, act=act)
        ref = silu_plain if act else plain
        assert torch.equal(out[bad[keep].long()].view(torch.int16), ref[keep].view(torch.int16))
        untouched = torch.ones(m, dtype=torch.bool, device=DEV)
        untouched[bad[keep].long()] = False
        assert (out[untouched] == 1234.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp6", "mxfp4"])
def test_native_moe_vs_oracle(pk, fmt):
    """One call per activation format against the f64 oracle on the CPU-quantised activations (MXFP4 weights): native_exact_bound per
    output, plus the p99 guard."""
    E, n, k = 4, 256, 1024
    ne = NativeExperts(pk, "mx", E, n, k, 51)
    counts = [100, 0, 1, 160]
    m = sum(counts)
    a = torch.randn(m, k, device=DEV).bfloat16()
    got = ne.moe(pk, a, _offsets_dev(counts), m, SENTINEL[fmt]).float().cpu().numpy().astype(np.float64)
    a_f32 = a.float().cpu().numpy()
    qfn = {"mxfp8": quantize_act_mxfp8, "mxfp6": quantize_act_mxfp6, "mxfp4": quantize_act_mxfp4}[fmt]
    o = np.concatenate([[0], np.cumsum(counts)])
    for e in range(E):
        if not counts[e]:
            continue
        a_q = qfn(a_f32[o[e]:o[e + 1]])
        dq, gs = ne.ex.dq(e), float(ne.ex.gs[e])
        _, exact = O.gemm_ref(O.f32_to_bf16_bits(a_q), True, dq, gs)
        err = np.abs(got[o[e]:o[e + 1]] - exact)
        assert (err <= np.maximum(np.maximum(1e-2, 1e-2 * np.abs(exact)), native_exact_bound(a_q, dq, gs, fmt))).all(), f"expert {e}"
        native_p99_guard(err, exact, (np.abs(a_q) @ np.abs(dq).T) * gs, f"{fmt} expert {e}")


def _native_layer(pk, kind, E, hid, inter, seed):
    w13, w2 = _make_layer(pk, kind, E, hid, inter, seed)
    if kind == "nv":
        return w13, w2, pk.nvfp4_native_images(w13.b, w13.sp, E, w13.n, w13.k), None, pk.nvfp4_native_images(w2.b, w2.sp, E, w2.n, w2.k), None
    return w13, w2, w13.b, w13.sp, w2.b, w2.sp


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp6", "mxfp4"])
@pytest.mark.parametrize("kind", ["mx", "nv"])
def test_fp4_moe_native_equals_its_stages_and_the_exact_layer(pk, kind, fmt):
    E, hid, inter, T, topk = 8, 1024, 512, 200, 2
    w13, w2, b13, s13, b2, s2 = _native_layer(pk, kind, E, hid, inter, 61)
    tw, ids = _routing(T, E, topk, 3)
    tw, ids = tw.to(DEV), ids.to(DEV)
    x = torch.randn(T, hid, device=DEV).bfloat16()
    out = pk.fp4_moe_native(x, b13, s13, w13.gsd, b2, s2, w2.gsd, tw, ids, kind=kind + "fp4", activations=fmt)
    # the same stages, one by one
    sp, off, ti = pk.moe_align_device(ids, E)
    m = T * topk
    qa = pk.quantize_activation_rows(x, fmt, ti)
    sid = SENTINEL[fmt]
    if kind == "nv":
        h = pk.mul_nvfp4_native_moe(qa, b13, w13.gsd, off, m, 2 * inter, hid, E, solution_id=sid, activation="silu_mul", out_quantized=fmt)
        y = pk.mul_nvfp4_native_moe(h, b2, w2.gsd, off, m, hid, inter, E, solution_id=sid, c_row_index=sp, c_rows=m)
    else:
        h = pk.mul_mxfp4_native_moe(qa, b13, s13, w13.gsd, off, m, 2 * inter, hid, E, solution_id=sid, activation="silu_mul", out_quantized=fmt)
        y = pk.mul_mxfp4_native_moe(h, b2, s2, w2.gsd, off, m, hid, inter, E, solution_id=sid, c_row_index=sp, c_rows=m)
    assert torch.equal(out.view(torch.int16), pk.moe_combine(y, tw, ids, E).view(torch.int16))
    # a loose sanity check against the exact fused layer on the same weights (guards against gross errors; not an accuracy claim)
    ref = pk.fp4_moe_fused(x, w13.b, w13.sp, w13.gsd, w2.b, w2.sp, w2.gsd, tw, ids, kind=kind + "fp4").float()
    rel = ((out.float() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    assert rel < (0.4 if fmt == "mxfp4" else 0.1), rel


@pytest.mark.gpu
def test_fp4_moe_native_graph_replay_with_changing_routing(pk):
    E, hid, inter, T, topk = 8, 1024, 512, 64, 2
    w13, w2, b13, s13, b2, s2 = _native_layer(pk, "mx", E, hid, inter, 71)
    x = torch.randn(T, hid, device=DEV).bfloat16()
    tw = torch.empty(T, topk, device=DEV)
    ids = torch.empty(T, topk, dtype=torch.int32, device=DEV)

    def layer():
        return pk.fp4_moe_native(x, b13, s13, w13.gsd, b2, s2, w2.gsd, tw, ids, kind="mxfp4", activations="mxfp8")

    w0, i0 = _routing(T, E, topk, 0)
    tw.copy_(w0)
    ids.copy_(i0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        layer()                                         # warm-up outside the capture (library state, allocator)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = layer()
    for seed in (1, 2, 3):
        w1, i1 = _routing(T, E, topk, seed)
        if seed == 3:
            i1[::5, 1] = -1                             # unrouted entries (expert parallelism)
        tw.copy_(w1)
        ids.copy_(i1)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), layer().view(torch.int16)), seed

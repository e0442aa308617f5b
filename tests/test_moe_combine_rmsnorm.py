"""petit_moe_combine_rmsnorm / moe_combine_rmsnorm: the MoE top-k combine, the residual add, the RMSNorm and (optionally) the activation
quantiser in one launch (include/petit_amd.h "Top-k combine into the norm"), its host twin petit_moe_combine_rmsnorm_host /
offline.moe_combine_rmsnorm_cpu, and the fused end of the layers (fp4_moe_fused / fp4_moe_native / fp4_moe_routed(..., norm_weight=...)).

Unmarked tests run without a GPU, through the C ABI's host twin: the twin against the chain stated independently (the combine in numpy f32, then
offline.rmsnorm_quantize_cpu), the 16-bit-only form at K = 2880 and K = 8, unrouted slots with poisoned rows, every refusal, the Python layer
and the Meta op.  The @pytest.mark.gpu ones check the device against the twin byte for byte (every ILP form, one and several groups of slots),
fused == the two launches, aliasing, the layers eagerly and from a replayed graph, and consumption by the native GEMM.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_gpu_parity import _mx_problem_on_device
from test_rmsnorm_quantize import bits, from_bits, round16

DEV = "cuda"
FMTS = {"mxfp8": 8, "mxfp6": 6, "mxfp4": 4}
E = 8   # experts of the synthetic routings: ids 0 .. 7 are routed, -1 and 8, 9 are not


def to_f32(b: np.ndarray, is_bf16: bool) -> np.ndarray:
    if is_bf16:
        return (b.astype(np.uint32) << 16).view(np.float32)
    return b.view(np.float16).astype(np.float32)


def make_case(T, k, topk, is_bf16, seed, all_unrouted_token=None):
    """slot rows, f32 weights, ids in [-1, E + 2) (about one in four unrouted), residual and norm weight, as bit patterns / numpy arrays."""
    rng = np.random.default_rng(seed)
    scale = np.array([0.05, 1.0, 20.0])[np.arange(T * topk) % 3][:, None]
    slot = round16((rng.standard_normal((T * topk, k)) * scale).astype(np.float32), is_bf16)
    tw = rng.random((T, topk), dtype=np.float32) + np.float32(0.01)
    ids = rng.integers(0, E, (T, topk)).astype(np.int32)
    drop = rng.random((T, topk)) < 0.25
    ids[drop] = rng.choice(np.array([-1, E, E + 1], dtype=np.int32), int(drop.sum()))
    if all_unrouted_token is not None:
        ids[all_unrouted_token] = -1
    res = round16(rng.standard_normal((T, k)).astype(np.float32), is_bf16)
    w = round16((1.0 + 0.1 * rng.standard_normal(k)).astype(np.float32), is_bf16)
    return slot, tw, ids, res, w


def combine_np(slot, tw, ids, is_bf16):
    """petit_moe_combine stated in numpy f32: acc = acc + x * w per routed slot in order (numpy rounds the product and the sum each), one round16."""
    T, topk = ids.shape
    x = to_f32(slot, is_bf16).reshape(T, topk, -1)
    acc = np.zeros((T, x.shape[2]), dtype=np.float32)
    for t in range(T):
        for j in range(topk):
            if 0 <= ids[t, j] < E:
                acc[t] = acc[t] + x[t, j] * tw[t, j]
    return round16(acc, is_bf16)


def twin(slot, tw, ids, res, w, is_bf16, fmt, eps=1e-6, woff=0.0, ids64=False):
    """offline.moe_combine_rmsnorm_cpu on bit patterns -> (qa bytes or None, y16 bits, h bits)."""
    from petit_kernel import offline
    out = offline.moe_combine_rmsnorm_cpu(from_bits(slot, is_bf16), torch.from_numpy(tw), torch.from_numpy(ids.astype(np.int64) if ids64 else ids), E,
                                          from_bits(w, is_bf16), eps, fmt, residual=None if res is None else from_bits(res, is_bf16),
                                          weight_offset=woff, return_normed=True, return_hidden=True)
    if fmt is None:
        return None, bits(out[1]), bits(out[0])
    return out[0].data.numpy(), bits(out[2]), bits(out[1])


@functools.lru_cache(maxsize=None)
def twin_case(T, k, topk, is_bf16, fmt, with_res, woff):
    """One host-twin reference per case, shared by the tests that need it."""
    slot, tw, ids, res, w = make_case(T, k, topk, is_bf16, 2000 + T + k + topk)
    res = res if with_res else None
    return (slot, tw, ids, res, w) + twin(slot, tw, ids, res, w, is_bf16, fmt, woff=woff)


# --- without a GPU --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ids64", [False, True])
@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp6", "mxfp4"])
def test_host_twin_equals_the_chain_stated_independently(fmt, is_bf16, ids64):
    """qa bytes, y16 and residual_out of the twin == the numpy combine -> offline.rmsnorm_quantize_cpu(residual=...), bit for bit; without a
    residual the twin's h is the combined row itself."""
    from petit_kernel import offline
    for (T, k, topk), with_res, woff in (((5, 768, 4), True, 0.0), ((3, 2048, 9), True, 1.0), ((4, 256, 2), False, 0.0), ((2, 4096, 3), False, 1.0),
                                        ((2, 256, 70), True, 0.0)):
        slot, tw, ids, res, w = make_case(T, k, topk, is_bf16, 10 * T + k + topk)
        c = combine_np(slot, tw, ids, is_bf16)
        want = offline.rmsnorm_quantize_cpu(from_bits(c, is_bf16), from_bits(w, is_bf16), 1e-6, fmt, residual=from_bits(res, is_bf16) if with_res else None,
                                            weight_offset=woff, return_normed=True)
        qa, y, h = twin(slot, tw, ids, res if with_res else None, w, is_bf16, fmt, woff=woff, ids64=ids64)
        tag = f"T={T} k={k} topk={topk} res={with_res} woff={woff}"
        assert np.array_equal(qa, want[0].data.numpy()), tag
        assert np.array_equal(y, bits(want[-1])), tag
        assert np.array_equal(h, bits(want[1]) if with_res else c), tag


@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("T,k,topk", [(4, 2880, 4), (3, 8, 2)])
def test_format_0_writes_the_16_bit_outputs_for_any_k(T, k, topk, is_bf16):
    """fmt None: h = round16(c + residual) (or c), y16 = round16((h inv) (w + offset)) in numpy f32 with inv = petit_rmsnorm_inv_host on h."""
    from petit_kernel import _lib
    eps = 1e-5
    slot, tw, ids, res, w = make_case(T, k, topk, is_bf16, 31 + k)
    c = combine_np(slot, tw, ids, is_bf16)
    for with_res, woff in ((True, 0.0), (False, 1.0)):
        qa, y, h = twin(slot, tw, ids, res if with_res else None, w, is_bf16, None, eps, woff)
        assert qa is None
        want_h = round16(to_f32(c, is_bf16) + to_f32(res, is_bf16), is_bf16) if with_res else c
        assert np.array_equal(h, want_h)
        inv = np.empty(T, dtype=np.float32)
        ht = from_bits(want_h, is_bf16)
        rc = _lib.lib.petit_rmsnorm_inv_host(inv.ctypes.data, ht.data_ptr(), None, eps, T, k, _lib.CXX_DTYPE_BF16 if is_bf16 else _lib.CXX_DTYPE_FP16)
        assert rc == _lib.PETIT_OK
        hf = to_f32(want_h, is_bf16)
        ms = (hf.astype(np.float64) ** 2).mean(axis=1)
        assert np.allclose(inv, 1.0 / np.sqrt(ms + eps), rtol=32 * 2.0 ** -24, atol=0)        # (the bound of test_rmsnorm_quantize: the stated order)
        want_y = round16((hf * inv[:, None]) * (to_f32(w, is_bf16) + np.float32(woff))[None, :], is_bf16)
        assert np.array_equal(y, want_y), f"res={with_res}: {int((y != want_y).sum())} y16 elements differ"


@pytest.mark.parametrize("is_bf16", [True, False])
def test_unrouted_slots_are_skipped_and_never_read(is_bf16):
    """Ids -1 and >= E contribute nothing; a token with every slot unrouted has h = residual, or without a residual a zero row with scale bytes 127;
    NaN patterns in the unrouted slot rows change no output byte."""
    T, k, topk = 5, 512, 4
    slot, tw, ids, res, w = make_case(T, k, topk, is_bf16, 77, all_unrouted_token=2)
    assert (ids == -1).any() and (ids >= E).any() and ((ids >= 0) & (ids < E)).any()
    unrouted = ~((ids >= 0) & (ids < E)).reshape(-1)
    poisoned = slot.copy()
    poisoned[unrouted] = np.where(np.arange(k) % 2, 0x7FC1, 0xFFFF).astype(np.uint16) if is_bf16 else np.where(np.arange(k) % 2, 0x7E01, 0xFFFF).astype(np.uint16)
    c = combine_np(slot, tw, ids, is_bf16)
    for fmt in (None, "mxfp8", "mxfp6", "mxfp4"):
        for r in (res, None):
            clean, dirty = twin(slot, tw, ids, r, w, is_bf16, fmt), twin(poisoned, tw, ids, r, w, is_bf16, fmt)
            for a, b in zip(clean, dirty):
                assert (a is None and b is None) or np.array_equal(a, b), (fmt, r is None)
            qa, y, h = dirty
            assert np.array_equal(h, round16(to_f32(c, is_bf16) + to_f32(r, is_bf16), is_bf16) if r is not None else c)
            assert np.array_equal(h[2], r[2]) if r is not None else not h[2].any()
            if r is None:
                assert not y[2].any()
                if fmt is not None:
                    scales = qa[T * k // 8 * FMTS[fmt]:].reshape(k // 128, T, 4)
                    assert (scales[:, 2] == 127).all()


def test_every_refusal_and_its_code():
    """Each refusal of the contract with its code, from the host twin and (refused before any launch) from the device entry point."""
    from petit_kernel import _lib
    L = _lib.lib
    buf = (C.c_uint8 * (1 << 17))()
    base = (C.addressof(buf) + 255) & ~255
    p = [C.c_void_p(base + 8192 * i) for i in range(8)]   # qa, y16, residual_out, slot_out, topk_weights, topk_ids, residual, weight: aligned, zeroed
    shape, kern, bad, ok = _lib.PETIT_ERROR_PROBLEM_SHAPE, _lib.PETIT_ERROR_KERNEL_SHAPE, _lib.PETIT_ERROR_BAD_ARGUMENT, _lib.PETIT_OK
    bf16 = _lib.CXX_DTYPE_BF16

    def both(qa=p[0], y16=p[1], res_out=p[2], slot=p[3], tw=p[4], ids=p[5], i64=0, res=p[6], w=p[7], eps=1e-6, woff=0.0, T=2, topk=2, k=256, ne=4,
             a_type=bf16, fmt=8):
        host = L.petit_moe_combine_rmsnorm_host(qa, y16, res_out, slot, tw, ids, i64, res, w, eps, woff, T, topk, k, ne, a_type, fmt)
        if host != ok or T == 0 or k == 0:                           # (an accepted call would launch: only the twin runs those)
            assert L.petit_moe_combine_rmsnorm(qa, y16, res_out, slot, tw, ids, i64, res, w, eps, woff, T, topk, k, ne, a_type, fmt, None) == host
        return host

    assert both() == ok and both(y16=None, res_out=None, res=None) == ok and both(a_type=_lib.CXX_DTYPE_FP16, fmt=6, i64=1) == ok
    assert both(res=None) == ok                                      # residual_out without a residual: the combined row
    assert both(fmt=0, qa=None, k=8) == ok and both(fmt=0, qa=None, k=2880, T=1, topk=1) == ok
    assert both(k=260) == shape and both(fmt=0, qa=None, k=12) == shape          # k % 8
    assert both(k=384) == shape and both(k=128) == shape and both(k=2880) == shape  # k % 256 with a format
    assert both(topk=0) == shape
    assert both(ne=0) == shape and both(ne=_lib.PETIT_MOE_MAX_EXPERTS + 1) == shape and both(ne=_lib.PETIT_MOE_MAX_EXPERTS) == ok
    assert both(T=1 << 20, topk=1 << 11) == shape                   # num_tokens * topk = 2^31
    assert both(T=(1 << 20) + 1, topk=1) == shape
    assert both(k=16384 + 256) == kern and both(fmt=0, qa=None, k=16384 + 8) == kern
    assert both(a_type=_lib.PETIT_DTYPE_FP32) == kern and both(a_type=_lib.CXX_DTYPE_FP4_E2M1) == kern
    for eps in (0.0, -1e-6, float("inf"), float("nan")):
        assert both(eps=eps) == bad
    for woff in (float("inf"), float("-inf"), float("nan")):
        assert both(woff=woff) == bad
    for name in ("slot", "tw", "ids", "w"):
        assert both(**{name: None}) == bad, name
    for name in ("qa", "y16", "res_out", "slot", "res", "w"):
        assert both(**{name: C.c_void_p(base + 8)}) == bad, name   # 16-byte alignment, every pointer of the 16-bit / qa set
    for fmt in (1, 5, 7, 16, -1):
        assert both(fmt=fmt) == bad
    assert both(fmt=0) == bad and both(fmt=0, qa=None, y16=None) == bad          # format 0 with a qa / without a y16
    assert both(qa=None) == bad and both(qa=None, fmt=4) == bad                  # a format without a qa
    assert both(T=0) == ok and both(k=0) == ok and both(T=0, qa=None, slot=None, tw=None, ids=None, w=None) == ok


def test_rmsnorm_inv_host_takes_any_k_multiple_of_8_and_keeps_its_other_refusals():
    """The test aid petit_rmsnorm_inv_host: k % 8 == 0 is enough (the 16-bit-only rows are checked through it); every other refusal it had stays."""
    from petit_kernel import _lib
    L = _lib.lib
    buf = (C.c_uint8 * (1 << 17))()
    base = (C.addressof(buf) + 255) & ~255
    inv, x, res = (C.c_void_p(base + 40960 * i) for i in range(3))
    shape, kern, bad, ok = _lib.PETIT_ERROR_PROBLEM_SHAPE, _lib.PETIT_ERROR_KERNEL_SHAPE, _lib.PETIT_ERROR_BAD_ARGUMENT, _lib.PETIT_OK

    def call(inv=inv, x=x, res=res, eps=1e-6, m=1, k=256, a_type=_lib.CXX_DTYPE_BF16):
        return L.petit_rmsnorm_inv_host(inv, x, res, eps, m, k, a_type)

    assert call() == ok and call(res=None) == ok and call(a_type=_lib.CXX_DTYPE_FP16) == ok
    assert call(k=8) == ok and call(k=2880) == ok and call(k=384) == ok and call(k=16384) == ok
    assert call(k=4) == shape and call(k=260) == shape and call(m=(1 << 20) + 1) == shape
    assert call(k=16384 + 8) == kern and call(a_type=_lib.PETIT_DTYPE_FP32) == kern
    for eps in (0.0, -1e-6, float("inf"), float("nan")):
        assert call(eps=eps) == bad
    assert call(x=None) == bad and call(inv=None) == bad
    assert call(x=C.c_void_p(base + 8)) == bad and call(res=C.c_void_p(base + 8)) == bad
    assert call(m=0) == ok and call(k=0) == ok
    out = (C.c_float * 1)()
    assert call(inv=C.cast(out, C.c_void_p), res=None, k=8, eps=0.25) == ok and out[0] == 2.0     # a zero row: 1 / sqrt(eps)


def test_python_layer_checks_exports_and_meta_op():
    import petit_kernel as pk
    from petit_kernel import compiled
    assert "moe_combine_rmsnorm" in pk.__all__ and callable(pk.moe_combine_rmsnorm) and callable(pk.offline.moe_combine_rmsnorm_cpu)
    T, topk, k = 3, 2, 256
    slot = torch.zeros(T * topk, k, dtype=torch.bfloat16)
    tw = torch.ones(T, topk)
    ids = torch.zeros(T, topk, dtype=torch.int32)
    w = torch.ones(k, dtype=torch.bfloat16)
    r = torch.zeros(T, k, dtype=torch.bfloat16)
    cpu = pk.offline.moe_combine_rmsnorm_cpu
    y = cpu(slot, tw, ids, E, w)                                                  # fmt None, no residual: the 16-bit y alone
    assert isinstance(y, torch.Tensor) and y.shape == (T, k) and y.dtype == torch.bfloat16
    h, y = cpu(slot, tw, ids, E, w, residual=r)
    assert h is not r and h.shape == y.shape == (T, k)
    h, y = cpu(slot, tw, ids, E, w, return_hidden=True)                           # the combined layer output
    q = cpu(slot, tw, ids, E, w, 1e-6, "mxfp8")
    assert isinstance(q, pk.QuantizedActivations) and (q.m, q.k, q.fmt, q.dtype) == (T, k, "mxfp8", torch.bfloat16)
    q, h = cpu(slot, tw, ids, E, w, 1e-6, "mxfp4", residual=r, inplace_residual=True)
    assert h is r and isinstance(q, pk.QuantizedActivations)
    q, h, y = cpu(slot, tw.clone(), ids.long(), E, w, 1e-6, "mxfp6", residual=r, return_normed=True)
    assert h.shape == y.shape == (T, k)
    q, y = cpu(slot, tw, ids, E, w, 1e-6, "mxfp8", residual=r, return_hidden=False, return_normed=True)
    assert isinstance(q, pk.QuantizedActivations) and y.shape == (T, k)
    for bad in (dict(fmt="fp8"), dict(eps=0.0), dict(weight_offset=float("nan")), dict(inplace_residual=True), dict(residual=r[:1]), dict(return_normed=False),
                dict(residual=r, inplace_residual=True, return_hidden=False)):
        with pytest.raises(RuntimeError):
            cpu(slot, tw, ids, E, w, **bad)
    for args in ((slot, tw, ids, 0, w), (slot, tw, ids, E, w.float()), (slot[:-1], tw, ids, E, w), (slot, tw.double(), ids, E, w),
                 (slot, tw, ids.to(torch.int16), E, w), (slot.float(), tw, ids, E, w)):
        with pytest.raises(RuntimeError):
            cpu(*args)
    with pytest.raises(RuntimeError):                                             # a format needs k % 256 == 0
        cpu(torch.zeros(T * topk, 2880, dtype=torch.bfloat16), tw, ids, E, torch.ones(2880, dtype=torch.bfloat16), 1e-6, "mxfp8")
    with pytest.raises(RuntimeError):
        pk.moe_combine_rmsnorm(slot, tw, ids, E, w)                               # CPU tensors: the device form wants GPU tensors
    with pytest.raises(RuntimeError):
        pk.moe.fp4_moe_fused(None, None, None, torch.ones(4), None, None, None, tw, ids, "nvfp4", norm_residual=r)   # a fused-end argument without norm_weight

    assert compiled.available(), compiled.why_unavailable()
    op = torch.ops.petit_kernel.moe_combine_rmsnorm
    m = lambda t: t.to("meta")
    for dtype in (torch.bfloat16, torch.float16):
        s16, w16, r16 = m(slot).to(dtype), m(w).to(dtype), m(r).to(dtype)
        for fmt, normed, hidden, inplace in ((0, True, False, False), (0, True, True, False), (8, False, False, False), (6, True, True, False),
                                             (4, False, True, True)):
            qa, h, y = op(s16, m(tw), m(ids), E, w16, 1e-6, fmt, r16, 0.0, normed, hidden, inplace)
            nbytes = pk._lib.lib.petit_quantized_activation_bytes(T, k, fmt) if fmt else 0
            assert qa.shape == (nbytes,) and qa.dtype == torch.uint8 and qa.device.type == "meta"
            assert tuple(h.shape) == ((T, k) if hidden and not inplace else (0,)) and h.dtype == dtype
            assert tuple(y.shape) == ((T, k) if normed else (0,)) and y.dtype == dtype


# --- on the GPU -----------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pk():
    import petit_kernel
    assert torch.cuda.is_available()
    name = torch.cuda.get_device_properties(0).gcnArchName
    assert name.startswith("gfx950"), f"these kernels are gfx950 code objects, device is {name}"
    return petit_kernel


def device_run(pk, slot, tw, ids, res, w, is_bf16, fmt, eps=1e-6, woff=0.0, ids64=False):
    """moe_combine_rmsnorm on bit patterns -> (qa bytes or None, y16 bits, h bits)."""
    idt = torch.from_numpy(ids.astype(np.int64) if ids64 else ids).to(DEV)
    out = pk.moe_combine_rmsnorm(from_bits(slot, is_bf16).to(DEV), torch.from_numpy(tw).to(DEV), idt, E, from_bits(w, is_bf16).to(DEV), eps, fmt,
                                 residual=None if res is None else from_bits(res, is_bf16).to(DEV), weight_offset=woff, return_normed=True,
                                 return_hidden=True)
    if fmt is None:
        return None, bits(out[1]), bits(out[0])
    return out[0].data.cpu().numpy(), bits(out[2]), bits(out[1])


# every ILP form (K <= 2048, 4096, 8192, 16384), the smallest K, a K that leaves waves partly idle; topk below, at and above a group of slots
# (8 / 4 / 2 / 2 slots per group for the four forms)
# (70 slots: the ids and weights are read 64 slots at a time)
SHAPES = [(1, 256, 1), (5, 768, 4), (2, 512, 11), (33, 3072, 9), (3, 8192, 8), (2, 16384, 2), (2, 16384, 3), (2, 256, 70)]


@pytest.mark.gpu
@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp6", "mxfp4"])
def test_device_equals_host_twin(pk, fmt, is_bf16, with_res):
    """qa, y16 and h byte for byte, over every shape; weight offset 1 and int64 ids on every other shape."""
    for i, (T, k, topk) in enumerate(SHAPES):
        woff = float(i % 2)
        slot, tw, ids, res, w, qa_h, y_h, h_h = twin_case(T, k, topk, is_bf16, fmt, with_res, woff)
        qa_d, y_d, h_d = device_run(pk, slot, tw, ids, res, w, is_bf16, fmt, woff=woff, ids64=bool(i % 2))
        tag = f"T={T} k={k} topk={topk} woff={woff}"
        assert np.array_equal(h_d, h_h), f"{tag}: {int((h_d != h_h).sum())} h elements differ"
        assert np.array_equal(y_d, y_h), f"{tag}: {int((y_d != y_h).sum())} y16 elements differ"
        assert np.array_equal(qa_d, qa_h), f"{tag}: {int((qa_d != qa_h).sum())} qa bytes differ"


@pytest.mark.gpu
@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("T,k,topk", [(4, 2880, 4), (3, 8, 2)])
def test_device_equals_host_twin_format_0(pk, T, k, topk, is_bf16):
    for with_res in (True, False):
        slot, tw, ids, res, w, _, y_h, h_h = twin_case(T, k, topk, is_bf16, None, with_res, 0.0)
        _, y_d, h_d = device_run(pk, slot, tw, ids, res, w, is_bf16, None)
        assert np.array_equal(h_d, h_h) and np.array_equal(y_d, y_h), (with_res, int((y_d != y_h).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp6", "mxfp4"])
def test_fused_equals_the_two_launches(pk, fmt):
    """moe_combine -> rmsnorm_quantize(residual=...) on the device gives the fused launch's bytes; the routing has -1 ids and the unrouted rows are
    NaN patterns."""
    for (T, k, topk), is_bf16 in (((33, 768, 4), True), ((7, 4096, 9), False)):
        slot, tw, ids, res, w = make_case(T, k, topk, is_bf16, 5 + T, all_unrouted_token=1)
        assert (ids == -1).any()
        slot[~((ids >= 0) & (ids < E)).reshape(-1)] = 0x7FC1 if is_bf16 else 0x7E01
        sd, rd, wd = (from_bits(t, is_bf16).to(DEV) for t in (slot, res, w))
        twd, idd = torch.from_numpy(tw).to(DEV), torch.from_numpy(ids).to(DEV)
        q, h, y = pk.moe_combine_rmsnorm(sd, twd, idd, E, wd, 1e-5, fmt, residual=rd, return_normed=True)
        q2, h2, y2 = pk.rmsnorm_quantize(pk.moe_combine(sd, twd, idd, E), wd, 1e-5, fmt, residual=rd, return_normed=True)
        assert torch.equal(q.data, q2.data) and np.array_equal(bits(h), bits(h2)) and np.array_equal(bits(y), bits(y2)), (T, k)
        assert (q.m, q.k, q.fmt, q.dtype) == (q2.m, q2.k, q2.fmt, q2.dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["mxfp8", None])
def test_residual_out_may_alias_residual(pk, fmt):
    T, k, topk, is_bf16 = 33, 3072, 9, True
    slot, tw, ids, res, w, qa_h, y_h, h_h = twin_case(T, k, topk, is_bf16, fmt, True, 0.0)
    rd = from_bits(res, is_bf16).to(DEV)
    out = pk.moe_combine_rmsnorm(from_bits(slot, is_bf16).to(DEV), torch.from_numpy(tw).to(DEV), torch.from_numpy(ids).to(DEV), E,
                                 from_bits(w, is_bf16).to(DEV), 1e-6, fmt, residual=rd, inplace_residual=True, return_normed=True)
    assert out[-2] is rd and np.array_equal(bits(rd), h_h) and np.array_equal(bits(out[-1]), y_h)
    if fmt:
        assert np.array_equal(out[0].data.cpu().numpy(), qa_h)


def _tiny_layer(pk, kind="nv"):
    from test_moe import _make_layer
    ne, hid, inter, T, topk = 4, 256, 256, 5, 2
    w13, w2 = _make_layer(pk, kind, ne, hid, inter, 501)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(T, hid, generator=g).to(torch.bfloat16).to(DEV)
    r = torch.randn(T, hid, generator=g).to(torch.bfloat16).to(DEV)
    nw = (1.0 + 0.1 * torch.randn(hid, generator=g)).to(torch.bfloat16).to(DEV)
    logits = [torch.randn(T, ne, generator=g).to(DEV) for _ in range(2)]
    return (w13.b, w13.sp, w13.gsd, w2.b, w2.sp, w2.gsd), x, r, nw, logits, topk


def _graph_of(fn):
    """fn warmed up on a side stream, then captured once."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    torch.cuda.synchronize()
    return g, out


@pytest.mark.gpu
@pytest.mark.parametrize("norm_fmt", ["mxfp8", None])
@pytest.mark.parametrize("layer", ["fused", "routed", "native"])
def test_layers_with_the_fused_end(pk, layer, norm_fmt):
    """fp4_moe_fused / fp4_moe_routed / fp4_moe_native(..., norm_weight=...) == the un-fused layer followed by rmsnorm_quantize, or for norm_fmt
    None by the add and the twin's norm -- eagerly, and from one captured graph replayed with a second routing (which has a -1 id on the layers
    that take ids)."""
    weights, x, r, nw, logits, topk = _tiny_layer(pk, "mx" if layer == "native" else "nv")
    slog = logits[0].clone()
    stw, sid = (t.clone() for t in pk.moe_route(slog, topk))

    def run(**norm):
        if layer == "fused":
            return pk.fp4_moe_fused(x, *weights, stw, sid, "nvfp4", **norm)
        if layer == "native":
            return pk.fp4_moe_native(x, *weights, stw, sid, "mxfp4", "mxfp8", **norm)
        return pk.fp4_moe_routed(x, slog, *weights, topk, "nvfp4", **norm)

    def check(got):
        out = run()
        if norm_fmt:
            q, h, y = pk.rmsnorm_quantize(out, nw, 1e-5, norm_fmt, residual=r, return_normed=True)
            assert isinstance(got[0], pk.QuantizedActivations) and torch.equal(got[0].data, q.data)
            assert np.array_equal(bits(got[1]), bits(h))
        else:
            h = out + r
            y = pk.offline.rmsnorm_quantize_cpu(h.cpu(), nw.cpu(), 1e-5, "mxfp8", return_normed=True)[1]
            assert np.array_equal(bits(got[0]), bits(h)) and np.array_equal(bits(got[1]), bits(y))
        return bits(got[1] if norm_fmt else got[0])

    norm = dict(norm_weight=nw, norm_eps=1e-5, norm_residual=r, norm_fmt=norm_fmt)
    got = run(**norm)
    assert len(got) == 2
    first = check(got)
    g, out = _graph_of(lambda: run(**norm))
    slog.copy_(logits[1])
    tw2, id2 = pk.moe_route(logits[1], topk)
    id2[0, 1] = -1
    stw.copy_(tw2)
    sid.copy_(id2)
    g.replay()
    torch.cuda.synchronize()
    assert not np.array_equal(check(out), first)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4"])
def test_native_gemm_consumes_the_result(pk, fmt):
    """mul_mxfp4_native on the fused launch's QuantizedActivations == on the chain's, as bit patterns."""
    m, n, k, topk = 64, 256, 1024, 4
    _, _, _, _, _, b, sp, gsd = _mx_problem_on_device(pk, m, n, k, 9200)
    sid = {"mxfp8": pk.SOLUTION_AUTO_NATIVE_MXFP8, "mxfp4": pk.SOLUTION_AUTO_NATIVE_MXFP4}[fmt]
    slot, tw, ids, res, w = make_case(m, k, topk, True, 41)
    sd, rd, wd = (from_bits(t, True).to(DEV) for t in (slot, res, w))
    twd, idd = torch.from_numpy(tw).to(DEV), torch.from_numpy(ids).to(DEV)
    pk.ops.enable_native_fp4(True)
    try:
        q, _ = pk.moe_combine_rmsnorm(sd, twd, idd, E, wd, 1e-6, fmt, residual=rd)
        q2, _ = pk.rmsnorm_quantize(pk.moe_combine(sd, twd, idd, E), wd, 1e-6, fmt, residual=rd)
        got = pk.mul_mxfp4_native(q, b, sp, gsd, m, n, k, sid)
        want = pk.mul_mxfp4_native(q2, b, sp, gsd, m, n, k, sid)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    finally:
        pk.ops.enable_native_fp4(False)

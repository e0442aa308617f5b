"""petit_rmsnorm_quantize / rmsnorm_quantize: (residual add +) RMSNorm that writes the native class's quantised activations in one launch
(include/petit_amd.h "RMSNorm into quantised activations"), and its host twin petit_rmsnorm_quantize_host / offline.rmsnorm_quantize_cpu.

Unmarked tests run without a GPU, through the C ABI's host twin: the twin against an independent f64 statement of the norm, its bytes against
the numpy statement of the quantiser, every refusal.  The @pytest.mark.gpu ones check the device against the twin byte for byte (every ILP form,
idle lanes, both dtypes, residual or none, both weight offsets), fused == two-step, hostile rows, aliasing, and consumption by the native GEMM
eagerly and from a replayed graph.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_gpu_parity import _mx_problem_on_device, decode_qact, quantize_act_mxfp4, quantize_act_mxfp6, quantize_act_mxfp8

DEV = "cuda"
FMTS = {"mxfp8": 8, "mxfp6": 6, "mxfp4": 4}
QUANT = {"mxfp8": quantize_act_mxfp8, "mxfp6": quantize_act_mxfp6, "mxfp4": quantize_act_mxfp4}
DTYPES = {True: torch.bfloat16, False: torch.float16}


# --- 16-bit patterns <-> numbers, in numpy alone (independent of the library and of torch's converts) -------------------------------------------------

def bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def from_bits(b: np.ndarray, is_bf16: bool) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(b).view(np.int16).copy()).view(DTYPES[is_bf16])


def to_f64(b: np.ndarray, is_bf16: bool) -> np.ndarray:
    if is_bf16:
        return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return b.view(np.float16).astype(np.float64)


def round16(v: np.ndarray, is_bf16: bool) -> np.ndarray:
    """f32 or f64 values -> the 16-bit patterns, ONE round to nearest even (normal-range bf16; fp16 by numpy's own correctly rounded cast)."""
    if not is_bf16:
        with np.errstate(over="ignore"):
            return v.astype(np.float16).view(np.uint16)
    if v.dtype == np.float32:
        u = v.view(np.uint32).astype(np.uint64)
        return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    u = v.astype(np.float64).view(np.uint64)                       # keep 8 significant bits of the f64: drop 45 mantissa bits, ties to even
    r = ((u + ((1 << 44) - 1) + ((u >> 45) & 1)) >> 45) << 45
    return (r.view(np.float64).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def ordered(b: np.ndarray) -> np.ndarray:
    """16-bit sign-magnitude patterns -> integers whose difference counts units in the last place."""
    mag = (b & 0x7FFF).astype(np.int64)
    return np.where(b & 0x8000, -mag, mag)


def make_inputs(m, k, is_bf16, seed, scales=(0.05, 1.0, 20.0)):
    rng = np.random.default_rng(seed)
    row_scale = np.array([scales[i % len(scales)] for i in range(m)])[:, None]
    x = round16((rng.standard_normal((m, k)) * row_scale).astype(np.float32), is_bf16)
    r = round16((rng.standard_normal((m, k)) * row_scale).astype(np.float32), is_bf16)
    w = round16((1.0 + 0.1 * rng.standard_normal(k)).astype(np.float32), is_bf16)
    return x, r, w


def host_twin(x, r, w, is_bf16, fmt, eps=1e-6, woff=0.0):
    """offline.rmsnorm_quantize_cpu on bit patterns -> (qa bytes, y16 bits, residual_out bits or None)."""
    from petit_kernel import offline
    out = offline.rmsnorm_quantize_cpu(from_bits(x, is_bf16), from_bits(w, is_bf16), eps, fmt, residual=None if r is None else from_bits(r, is_bf16),
                                       weight_offset=woff, return_normed=True)
    if r is None:
        return out[0].data.numpy(), bits(out[1]), None
    return out[0].data.numpy(), bits(out[2]), bits(out[1])


@functools.lru_cache(maxsize=None)
def twin_case(m, k, is_bf16, fmt, with_res, woff):
    """One host-twin reference per case, shared by the tests that need it."""
    x, r, w = make_inputs(m, k, is_bf16, 1000 + m + k)
    return (x, r if with_res else None, w) + host_twin(x, r if with_res else None, w, is_bf16, fmt, woff=woff)


# --- without a GPU --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("k", [256, 3072, 16384])
def test_host_twin_against_f64_statement(k, is_bf16):
    """The twin against h, mean square and y stated in f64.  residual_out is round16(x + r) exactly.  inv (petit_rmsnorm_inv_host: y itself carries
    it only through a 16-bit rounding) within 32 x 2^-24 relative of the f64 value: at most 30 roundings on the longest path of the stated order
    (8 in a column chain, 7 column adds, 6 butterflies, 3 wave adds, with room) plus the three of step 3.  y16 within one unit in the last place of
    the rounded f64 value everywhere, and different from it in at most 1 element in 1000 -- a condition, not a tolerance: a numpy simulation of the
    f32 arithmetic on such inputs differs in <= 8e-5 of the elements."""
    from petit_kernel import _lib
    m, eps = 6, 1e-6
    x, r, w = make_inputs(m, k, is_bf16, 77 + k)
    for woff in (0.0, 1.0):
        _, y, res_out = host_twin(x, r, w, is_bf16, "mxfp8", eps, woff)
        h = round16((to_f64(x, is_bf16) + to_f64(r, is_bf16)).astype(np.float32), is_bf16)      # (the f64 sum of two 16-bit values is exact)
        assert np.array_equal(res_out, h)
        h64 = to_f64(h, is_bf16)
        inv64 = 1.0 / np.sqrt((h64 * h64).mean(axis=1) + np.float64(np.float32(eps)))
        inv = np.empty(m, dtype=np.float32)
        xt, rt = from_bits(x, is_bf16), from_bits(r, is_bf16)
        rc = _lib.lib.petit_rmsnorm_inv_host(inv.ctypes.data, xt.data_ptr(), rt.data_ptr(), eps, m, k,
                                             _lib.CXX_DTYPE_BF16 if is_bf16 else _lib.CXX_DTYPE_FP16)
        assert rc == _lib.PETIT_OK
        rel = np.abs(inv.astype(np.float64) - inv64) / inv64
        print(f"k={k} bf16={is_bf16} woff={woff}: inv rel err max {rel.max():.3e} (bound {32 * 2.0 ** -24:.3e})")
        assert (rel <= 32 * 2.0 ** -24).all()
        want = round16(h64 * inv64[:, None] * (to_f64(w, is_bf16) + woff)[None, :], is_bf16)
        ulps = np.abs(ordered(y) - ordered(want))
        print(f"   y16: {int((ulps != 0).sum())} of {ulps.size} differ, max {int(ulps.max())} ulp")
        assert ulps.max() <= 1
        assert (ulps != 0).sum() * 1000 <= ulps.size


@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp6", "mxfp4"])
def test_host_twin_bytes_are_the_quantiser_on_y16(fmt, is_bf16):
    """decode(qa) == the numpy statement of the quantiser applied to the twin's own y16, exactly; with and without a residual; K with idle lanes."""
    for (m, k), with_res in (((5, 768), True), ((3, 2048), False)):
        _, _, _, qa, y, _ = twin_case(m, k, is_bf16, fmt, with_res, 0.0)
        want = QUANT[fmt](to_f64(y, is_bf16).astype(np.float32))
        assert np.array_equal(decode_qact(qa, m, k, fmt), want)


def test_every_refusal_and_its_code():
    """Each refusal of the contract with its code, from the host twin and (refused before any launch) from the device entry point."""
    from petit_kernel import _lib
    L = _lib.lib
    buf = (C.c_uint8 * (1 << 16))()
    base = (C.addressof(buf) + 255) & ~255
    p = [C.c_void_p(base + 8192 * i) for i in range(6)]          # qa, y16, residual_out, x, residual, weight: aligned host scratch
    shape, kern, bad, ok = _lib.PETIT_ERROR_PROBLEM_SHAPE, _lib.PETIT_ERROR_KERNEL_SHAPE, _lib.PETIT_ERROR_BAD_ARGUMENT, _lib.PETIT_OK
    bf16 = _lib.CXX_DTYPE_BF16

    def both(qa=p[0], y16=p[1], res_out=p[2], x=p[3], res=p[4], w=p[5], eps=1e-6, woff=0.0, m=2, k=256, a_type=bf16, fmt=8):
        host = L.petit_rmsnorm_quantize_host(qa, y16, res_out, x, res, w, eps, woff, m, k, a_type, fmt)
        if host != ok or m == 0 or k == 0:                        # (an accepted call would launch: only the twin runs those)
            assert L.petit_rmsnorm_quantize(qa, y16, res_out, x, res, w, eps, woff, m, k, a_type, fmt, None) == host
        return host

    assert both() == ok and both(y16=None, res_out=None, res=None) == ok and both(a_type=_lib.CXX_DTYPE_FP16, fmt=6) == ok
    assert both(k=384) == shape and both(k=128) == shape
    assert both(k=16384 + 256) == kern
    assert both(a_type=_lib.PETIT_DTYPE_FP32) == kern and both(a_type=_lib.CXX_DTYPE_FP4_E2M1) == kern
    for eps in (0.0, -1e-6, float("inf"), float("nan")):
        assert both(eps=eps) == bad
    for woff in (float("inf"), float("-inf"), float("nan")):
        assert both(woff=woff) == bad
    assert both(qa=None) == bad and both(x=None) == bad and both(w=None) == bad
    for name in ("qa", "y16", "res_out", "x", "res", "w"):
        assert both(**{name: C.c_void_p(base + 8)}) == bad, name   # 16-byte alignment, every pointer
    assert both(res=None) == bad                                  # a residual_out without a residual
    assert both(res=None, res_out=None) == ok
    for fmt in (0, 5, 7, 16):
        assert both(fmt=fmt) == bad
    assert both(m=0) == ok and both(k=0) == ok and both(m=0, qa=None, x=None, w=None) == ok


def test_python_layer_checks_and_exports():
    import petit_kernel as pk
    assert "rmsnorm_quantize" in pk.__all__ and callable(pk.rmsnorm_quantize) and callable(pk.offline.rmsnorm_quantize_cpu)
    x = torch.zeros(2, 256, dtype=torch.bfloat16)
    w = torch.ones(256, dtype=torch.bfloat16)
    cpu = pk.offline.rmsnorm_quantize_cpu
    q = cpu(x, w)
    assert isinstance(q, pk.QuantizedActivations) and (q.m, q.k, q.fmt) == (2, 256, "mxfp8")
    r = torch.zeros_like(x)
    q, ro = cpu(x, w, residual=r)
    assert ro is not r
    q, ro, y = cpu(x, w, residual=r, return_normed=True, inplace_residual=True)
    assert ro is r and y.shape == x.shape and y.dtype == x.dtype
    for bad in (dict(fmt="fp8"), dict(eps=0.0), dict(weight_offset=float("nan")), dict(inplace_residual=True), dict(residual=r[:1])):
        with pytest.raises(RuntimeError):
            cpu(x, w, **bad)
    with pytest.raises(RuntimeError):
        cpu(x, w.float())
    with pytest.raises(RuntimeError):
        cpu(torch.zeros(2, 384, dtype=torch.bfloat16), torch.ones(384, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError):
        pk.rmsnorm_quantize(x, w)                                  # CPU tensors: the device form wants GPU tensors


# --- on the GPU -----------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pk():
    import petit_kernel
    assert torch.cuda.is_available()
    name = torch.cuda.get_device_properties(0).gcnArchName
    assert name.startswith("gfx950"), f"these kernels are gfx950 code objects, device is {name}"
    return petit_kernel


def device_run(pk, x, r, w, is_bf16, fmt, eps=1e-6, woff=0.0):
    """rmsnorm_quantize on bit patterns -> (qa bytes, y16 bits, residual_out bits or None)."""
    xd, wd = from_bits(x, is_bf16).to(DEV), from_bits(w, is_bf16).to(DEV)
    out = pk.rmsnorm_quantize(xd, wd, eps, fmt, residual=None if r is None else from_bits(r, is_bf16).to(DEV), weight_offset=woff, return_normed=True)
    if r is None:
        return out[0].data.cpu().numpy(), bits(out[1]), None
    return out[0].data.cpu().numpy(), bits(out[2]), bits(out[1])


SHAPES = [(1, 256), (5, 768), (33, 3072), (3, 8192), (2, 16384)]     # every ILP form, the smallest K, a K that leaves waves partly idle


@pytest.mark.gpu
@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp6", "mxfp4"])
def test_device_equals_host_twin(pk, fmt, is_bf16, with_res):
    """qa, y16 and residual_out byte for byte, over every shape and both weight offsets."""
    for m, k in SHAPES:
        for woff in (0.0, 1.0):
            x, r, w, qa_h, y_h, ro_h = twin_case(m, k, is_bf16, fmt, with_res, woff)
            qa_d, y_d, ro_d = device_run(pk, x, r, w, is_bf16, fmt, woff=woff)
            tag = f"m={m} k={k} woff={woff}"
            if with_res:
                assert np.array_equal(ro_d, ro_h), tag
            assert np.array_equal(y_d, y_h), f"{tag}: {int((y_d != y_h).sum())} y16 elements differ"
            assert np.array_equal(qa_d, qa_h), f"{tag}: {int((qa_d != qa_h).sum())} qa bytes differ"


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp6", "mxfp4"])
def test_fused_equals_two_step(pk, fmt):
    """quantize_activations on the fused launch's own y16 gives the fused launch's bytes."""
    for m, k in ((130, 2048), (33, 768)):
        x, r, w = make_inputs(m, k, True, 5 + m)
        xd, rd, wd = (from_bits(t, True).to(DEV) for t in (x, r, w))
        q, _, y = pk.rmsnorm_quantize(xd, wd, 1e-5, fmt, residual=rd, return_normed=True)
        two = pk.quantize_activations(y, fmt)
        assert torch.equal(q.data, two.data), (m, k)
        assert (q.m, q.k, q.fmt, q.dtype) == (two.m, two.k, two.fmt, two.dtype)


def hostile_rows(is_bf16):
    """(16, 2048): a zero row, a -0.0 row, 16-bit subnormals, one huge value among tiny ones, (bf16) magnitudes 2^70 whose squares overflow, and a row
    built so that inv is exactly 1/2 (sum of squares exactly 4 k, every partial sum exact in any order; eps = 2^-40 vanishes in the f32 sum) whose
    blocks have maxima just below / at / above the saturation points 6 (e2m1) and 7.5 (e2m3), at the top and the bottom of the binade, and their
    negatives -- so y = h / 2 exactly and the block maxima of y sit where the row puts them."""
    rng = np.random.default_rng(4242)
    m, k = 16, 2048
    a = (rng.standard_normal((m, k)) * 0.5).astype(np.float32)
    a[0] = 0.0
    a[1] = -0.0
    tiny = 2.0 ** -133 if is_bf16 else 2.0 ** -24
    a[2] = tiny * rng.integers(0, 8, k)
    a[3] = 1e-3
    a[3, 5::64] = 3.0e4 if is_bf16 else 3.0e3
    a[3, 777] = -(3.0e4 if is_bf16 else 3.0e3)
    if is_bf16:
        a[4] = 2.0 ** 70 * np.where(rng.integers(0, 2, k), 1.0, -1.0)
    maxima = [5.96875, 6.0, 6.03125, 7.46875, 7.5, 7.53125, 7.96875, 4.0, 3.96875]
    row = np.zeros(k)
    blk = 0
    for sign in (1.0, -1.0):
        for t in maxima:
            vals = rng.integers(-32, 33, 32) / 32.0                # multiples of 2^-5 in [-1, 1]
            vals[7] = t
            row[32 * blk: 32 * blk + 32] = sign * vals
            blk += 1
    rest = int(round((4.0 * k - (row * row).sum()) * 1024))         # what is left of 4 k, in units of 2^-10: filled with squares of n / 32, n <= 128
    pos = 32 * blk
    while rest:
        n = min(128, int(np.sqrt(rest)))
        row[pos] = n / 32.0
        rest -= n * n
        pos += 1
    assert pos <= k and (row * row).sum() == 4.0 * k
    a[5] = row
    x = round16(a, is_bf16)
    assert np.array_equal(to_f64(x[5], is_bf16), row)
    return x, round16(np.ones(k, dtype=np.float32), is_bf16)


@pytest.mark.gpu
@pytest.mark.parametrize("is_bf16", [True, False])
def test_hostile_rows(pk, is_bf16):
    """Device == host twin == the numpy statement of the quantiser on y16, on rows that hit every consequence the contract names."""
    x, w = hostile_rows(is_bf16)
    m, k = x.shape
    eps = 2.0 ** -40
    for fmt in FMTS:
        qa_h, y_h, _ = host_twin(x, None, w, is_bf16, fmt, eps)
        qa_d, y_d, _ = device_run(pk, x, None, w, is_bf16, fmt, eps)
        assert np.array_equal(y_d, y_h), f"{fmt}: rows {sorted(set(np.argwhere(y_d != y_h)[:, 0]))} of y16 differ"
        assert np.array_equal(qa_d, qa_h), f"{fmt}: {int((qa_d != qa_h).sum())} qa bytes differ"
        got = decode_qact(qa_d, m, k, fmt)
        assert np.array_equal(got, QUANT[fmt](to_f64(y_d, is_bf16).astype(np.float32))), fmt
        scales = qa_d[m * k // 8 * FMTS[fmt]:].reshape(k // 128, m, 4)
        assert (scales[:, 0] == 127).all() and (scales[:, 1] == 127).all() and (got[0] == 0).all() and (got[1] == 0).all()
    assert (y_d[0] == 0).all() and (y_d[1] == 0x8000).all()                          # inv = 1 / sqrt(eps); the sign of zero goes through
    assert np.array_equal(to_f64(y_d[5], is_bf16), to_f64(x[5], is_bf16) / 2)         # inv = 1/2 exactly: the maxima sit where the row put them
    if is_bf16:
        assert ((y_d[4] & 0x7FFF) == 0).all() and np.array_equal(y_d[4] & 0x8000, x[4] & 0x8000)   # S = inf, inv = 0, y = +-0


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp6"])
def test_aliasing_gives_the_same_bytes(pk, fmt):
    """residual_out is residual (inplace_residual) and y16 is x (the C ABI: the Python layer always allocates y16): the out-of-place bytes."""
    from petit_kernel import _lib
    m, k, is_bf16 = 33, 3072, True
    x, r, w, qa_h, y_h, ro_h = twin_case(m, k, is_bf16, fmt, True, 0.0)
    xd, rd, wd = (from_bits(t, is_bf16).to(DEV) for t in (x, r, w))
    q, ro = pk.rmsnorm_quantize(xd, wd, 1e-6, fmt, residual=rd, inplace_residual=True)
    assert ro is rd and np.array_equal(bits(rd), ro_h) and np.array_equal(q.data.cpu().numpy(), qa_h)
    rd = from_bits(r, is_bf16).to(DEV)
    qa = torch.empty_like(q.data)
    with torch.cuda.device(xd.device):
        rc = _lib.lib.petit_rmsnorm_quantize(qa.data_ptr(), xd.data_ptr(), rd.data_ptr(), xd.data_ptr(), rd.data_ptr(), wd.data_ptr(), 1e-6, 0.0, m, k,
                                             _lib.CXX_DTYPE_BF16, FMTS[fmt], C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.PETIT_OK
    assert np.array_equal(bits(xd), y_h) and np.array_equal(bits(rd), ro_h) and np.array_equal(qa.cpu().numpy(), qa_h)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4"])
def test_native_gemm_consumes_the_result_eagerly_and_from_a_graph(pk, fmt):
    """mul_mxfp4_native on rmsnorm_quantize's result == on quantize_activations(y16), as bit patterns; a captured graph of norm + GEMM, replayed
    twice with x changed in between, follows the new x."""
    m, n, k = 64, 256, 1024
    _, _, _, _, a, b, sp, gsd = _mx_problem_on_device(pk, m, n, k, 9100)
    sid = {"mxfp8": pk.SOLUTION_AUTO_NATIVE_MXFP8, "mxfp4": pk.SOLUTION_AUTO_NATIVE_MXFP4}[fmt]
    x1, r, w = make_inputs(m, k, True, 31)
    x2, _, _ = make_inputs(m, k, True, 32)
    xd, rd, wd = (from_bits(t, True).to(DEV) for t in (x1, r, w))
    pk.ops.enable_native_fp4(True)
    try:
        def fused():
            q, _ = pk.rmsnorm_quantize(xd, wd, 1e-6, fmt, residual=rd)
            return pk.mul_mxfp4_native(q, b, sp, gsd, m, n, k, sid)

        def two_step():
            _, _, y = pk.rmsnorm_quantize(xd, wd, 1e-6, fmt, residual=rd, return_normed=True)
            return pk.mul_mxfp4_native(pk.quantize_activations(y, fmt), b, sp, gsd, m, n, k, sid)

        want1 = two_step()
        assert torch.equal(fused().view(torch.int16), want1.view(torch.int16))
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            fused()
            stream.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                out = fused()
            g.replay()
            stream.synchronize()
            assert torch.equal(out.view(torch.int16), want1.view(torch.int16))
            xd.copy_(from_bits(x2, True))
            g.replay()
            stream.synchronize()
            got2 = out.clone()
        want2 = two_step()
        assert torch.equal(got2.view(torch.int16), want2.view(torch.int16)) and not torch.equal(want1.view(torch.int16), want2.view(torch.int16))
    finally:
        pk.ops.enable_native_fp4(False)

"""Block-Hadamard rotation "petit-had/1" in the native class's activation quantisers (include/petit_amd.h "Block-Hadamard rotation"):
petit_hadamard_rows, petit_quantize_activations_rot, petit_quantize_activations_rows_rot, petit_rmsnorm_quantize_rot, their host twins and the
Python layer (hadamard_rotate, the hadamard= keyword of the quantisers and of quantize_mxfp4 / quantize_nvfp4).

Unmarked tests run without a GPU through the host twins: the twins against an independent numpy statement of the definition (float32 butterflies
in the stated stage order, then the numpy statement of the quantiser), that the statement can see the stage order, the algebra on integers, the
weight convenience, the accuracy gain that is the reason for the feature, and every refusal.  The @pytest.mark.gpu ones check the four device
entries against the twins byte for byte, the gathered form, fused norm == chain, block 0 == the unrotated entries, that a non-finite element
spoils only its own rotation block, consumption by the native GEMMs (eagerly and from a graph), and the in-place rotation.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_gpu_parity import decode_qact, native_exact_bound, quantize_act_mxfp4, quantize_act_mxfp8

DEV = "cuda"
FMTS = {"mxfp8": 8, "mxfp4": 4}
QUANT = {"mxfp8": quantize_act_mxfp8, "mxfp4": quantize_act_mxfp4}
EMAX = {"mxfp8": 7, "mxfp4": 2}
DTYPES = {True: torch.bfloat16, False: torch.float16}
BLOCKS = (32, 128)


# --- 16-bit patterns <-> numbers and the definition, in numpy alone ------------------------------------------------------------------------------------

def bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def from_bits(b: np.ndarray, is_bf16: bool) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(b).view(np.int16).copy()).view(DTYPES[is_bf16])


def to_f32(b: np.ndarray, is_bf16: bool) -> np.ndarray:
    if is_bf16:
        return (b.astype(np.uint32) << 16).view(np.float32)
    return b.view(np.float16).astype(np.float32)


def round16(v: np.ndarray, is_bf16: bool) -> np.ndarray:
    """float32 -> the 16-bit patterns, ONE round to nearest even (bf16 by the integer rule, fp16 by numpy's correctly rounded cast)."""
    assert v.dtype == np.float32
    if not is_bf16:
        with np.errstate(over="ignore"):
            return v.astype(np.float16).view(np.uint16)
    u = np.ascontiguousarray(v).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def hadamard_np(z: np.ndarray, block: int, reverse: bool = False) -> np.ndarray:
    """The definition: float32 butterflies (z[i], z[i + d]) <- (z[i] + z[i + d], z[i] - z[i + d]) for d = 1, 2, ..., block / 2 in this order
    (reverse: the other order, which the contract does NOT mean) on every block of `block` consecutive elements of the last axis."""
    assert z.dtype == np.float32
    shape = z.shape
    z = z.reshape(-1, block).copy()
    strides = [1 << s for s in range(block.bit_length() - 1)]
    for d in (reversed(strides) if reverse else strides):
        v = z.reshape(-1, block // (2 * d), 2, d)
        a, b = v[:, :, 0, :].copy(), v[:, :, 1, :].copy()
        v[:, :, 0, :] = a + b                                      # float32 + float32: one rounding, nothing fused
        v[:, :, 1, :] = a - b
    return z.reshape(shape)


def sylvester(block: int) -> np.ndarray:
    h = np.array([[1.0]])
    while h.shape[0] < block:
        h = np.kron(np.array([[1.0, 1.0], [1.0, -1.0]]), h)         # natural order: entry (i, j) = (-1)^popcount(i & j)
    return h


def scale_bytes_np(z: np.ndarray, fmt: str) -> np.ndarray:
    """The scale byte of every 32-k block of z [m, k] (OCP floor rule, act_scale_byte) -> [m, k / 32]."""
    amax = np.abs(z.reshape(z.shape[0], -1, 32)).max(axis=2).astype(np.float32)
    ebits = ((amax.view(np.uint32) >> 23) & 0xFF).astype(np.int64)
    return np.where(amax == 0, 127, np.clip(ebits - EMAX[fmt], 1, 254)).astype(np.uint8)


def qact_scales(raw: np.ndarray, m: int, k: int, fmt: str) -> np.ndarray:
    """The scale bytes of 'petit-qact/1' bytes -> [m, k / 32]."""
    return raw[m * k // 8 * FMTS[fmt]:].reshape(k // 128, m, 4).transpose(1, 0, 2).reshape(m, k // 32)


def qact_tiles(raw: np.ndarray, m: int, k: int, fmt: str):
    """'petit-qact/1' bytes -> (element bytes [k / 128, m, .], scale bytes [k / 128, m, 4])."""
    split = m * k // 8 * FMTS[fmt]
    return raw[:split].reshape(k // 128, m, 16 * FMTS[fmt]), raw[split:].reshape(k // 128, m, 4)


@functools.lru_cache(maxsize=None)
def mixed_input(m: int, k: int, is_bf16: bool, seed: int = 0) -> np.ndarray:
    """[m, k] 16-bit patterns of N(0, 1) x a magnitude drawn per ELEMENT from 0.05 .. 20, so that the f32 sums of a block do round."""
    rng = np.random.default_rng(9000 + 7 * m + k + seed)
    mag = rng.choice(np.array([0.05, 0.3, 1.0, 4.0, 20.0]), size=(m, k))
    x = round16((rng.standard_normal((m, k)) * mag).astype(np.float32), is_bf16)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def twin_qact(m: int, k: int, is_bf16: bool, fmt: str, block: int) -> np.ndarray:
    """offline.quantize_activations_cpu on mixed_input: one host-twin reference per case, shared by the tests that need it."""
    from petit_kernel import offline
    raw = offline.quantize_activations_cpu(from_bits(mixed_input(m, k, is_bf16), is_bf16), fmt, hadamard=block).data.numpy()
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def twin_rotate(m: int, k: int, is_bf16: bool, block: int, log2_scale: int) -> np.ndarray:
    from petit_kernel import offline
    out = bits(offline.hadamard_rotate_cpu(from_bits(mixed_input(m, k, is_bf16), is_bf16), block, log2_scale))
    out.setflags(write=False)
    return out


# --- without a GPU --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("m,k", [(1, 256), (3, 2304)])
def test_twin_is_the_definition(m, k, block, is_bf16):
    """petit_hadamard_rows_host and petit_quantize_activations_rot_host against the numpy statement: the 16-bit rotation bit for bit, the
    quantiser's decoded elements and scale bytes exactly."""
    x = mixed_input(m, k, is_bf16)
    z = hadamard_np(to_f32(x, is_bf16), block)
    for log2_scale in (0, -(block.bit_length() - 1)):
        want = round16(z * np.float32(2.0 ** log2_scale), is_bf16)
        assert np.array_equal(twin_rotate(m, k, is_bf16, block, log2_scale), want), (block, log2_scale)
    for fmt in FMTS:
        raw = twin_qact(m, k, is_bf16, fmt, block)
        assert np.array_equal(qact_scales(raw, m, k, fmt), scale_bytes_np(z, fmt)), fmt
        assert np.array_equal(decode_qact(raw, m, k, fmt), QUANT[fmt](z)), fmt


def test_the_stage_order_is_what_is_pinned():
    """On such an input a butterfly in the reverse stage order differs from the definition in at least one bit -- and the twin follows the
    definition: the test above can see the order."""
    m, k, block = 3, 2304, 128
    x32 = to_f32(mixed_input(m, k, True), True)
    fwd, rev = hadamard_np(x32, block), hadamard_np(x32, block, reverse=True)
    assert not np.array_equal(fwd.view(np.uint32), rev.view(np.uint32))
    assert np.allclose(fwd, rev, rtol=1e-4, atol=1e-3)                # (the same matrix product: only the roundings differ)
    raw = twin_qact(m, k, True, "mxfp8", block)
    assert np.array_equal(decode_qact(raw, m, k, "mxfp8"), quantize_act_mxfp8(fwd))


@pytest.mark.parametrize("is_bf16", [True, False])
def test_algebra_on_integers(is_bf16):
    """x in {-1, 0, 1}, B = 128: x . H holds integers of magnitude <= 128, exact in both 16-bit types -- the integer matrix product; rotating
    that again with log2_scale = -7 returns x exactly (H . H = 128 I)."""
    from petit_kernel import offline
    rng = np.random.default_rng(5)
    xi = rng.integers(-1, 2, (4, 512))
    x = from_bits(round16(xi.astype(np.float32), is_bf16), is_bf16)
    r = offline.hadamard_rotate_cpu(x, 128, 0)
    want = (xi.reshape(4, 4, 128) @ sylvester(128).astype(np.int64)).reshape(4, 512)
    assert np.abs(want).max() <= 128
    assert np.array_equal(to_f32(bits(r), is_bf16).astype(np.int64), want)
    back = offline.hadamard_rotate_cpu(r, 128, -7)
    assert np.array_equal(bits(back), bits(x))
    r32 = offline.hadamard_rotate_cpu(x, 32, 0)
    assert np.array_equal(to_f32(bits(r32), is_bf16).astype(np.int64), (xi.reshape(4, 16, 32) @ sylvester(32).astype(np.int64)).reshape(4, 512))


@pytest.mark.parametrize("block", BLOCKS)
def test_weight_convenience_is_rotate_then_quantise(block):
    """quantize_*_cpu(w, hadamard=B) == quantize_*_cpu(hadamard_rotate_cpu(w, B, -log2 B)), byte for byte, on stacked experts whose row count is
    no multiple of the rotation block.  [3, 48, 512] for NVFP4; MXFP4's own rule (num_experts * size_n % 32 == 0) refuses that tensor with
    or without a rotation, so MXFP4 runs [2, 48, 512] (96 rows)."""
    from petit_kernel import offline
    rng = np.random.default_rng(11)
    lg = block.bit_length() - 1
    w = torch.from_numpy((0.05 * rng.standard_normal((3, 48, 512))).astype(np.float32)).bfloat16()
    got, want = offline.quantize_nvfp4_cpu(w, hadamard=block), offline.quantize_nvfp4_cpu(offline.hadamard_rotate_cpu(w, block, -lg))
    assert all(torch.equal(g.view(torch.uint8), t.view(torch.uint8)) for g, t in zip(got, want))
    assert not torch.equal(got[0], offline.quantize_nvfp4_cpu(w)[0])
    gs = torch.full((3,), 0.001, dtype=torch.float32)
    got, want = offline.quantize_nvfp4_cpu(w, gs, hadamard=block), offline.quantize_nvfp4_cpu(offline.hadamard_rotate_cpu(w, block, -lg), gs)
    assert all(torch.equal(g.view(torch.uint8), t.view(torch.uint8)) for g, t in zip(got, want))
    for hadamard in (0, block):
        with pytest.raises(RuntimeError, match="MX scale tile"):
            offline.quantize_mxfp4_cpu(w, hadamard=hadamard)
    w2 = w[:2].contiguous().half()
    got, want = offline.quantize_mxfp4_cpu(w2, hadamard=block), offline.quantize_mxfp4_cpu(offline.hadamard_rotate_cpu(w2, block, -lg))
    assert all(torch.equal(g.view(torch.uint8), t.view(torch.uint8)) for g, t in zip(got, want))
    assert not torch.equal(got[0], offline.quantize_mxfp4_cpu(w2)[0])


@pytest.mark.parametrize("block", BLOCKS)
def test_rotation_cuts_the_mxfp4_activation_error(block):
    """The reason for the feature.  m = 32, k = 1024, n = 64; x = N(0, 1) with every channel c % 32 == 5 multiplied by 20, rounded to bf16;
    W = 0.02 N(0, 1) exact in float64, so only the activations are quantised.  rms(x_q . W'^T - x . W^T) with the twin's rotated MXFP4 bytes and
    W' = W . H_B / B must be at most 0.75 of the unrotated quantiser's error on the same input.  (A numpy simulation over 12 seeds gave a worst
    ratio of 0.62 for both B, mean 0.60; the margin covers the seed and the bf16 rounding of x.)"""
    from petit_kernel import offline
    m, k, n = 32, 1024, 64
    rng = np.random.default_rng(2024)
    x = rng.standard_normal((m, k))
    x[:, 5::32] *= 20.0
    xb = round16(x.astype(np.float32), True)
    x64 = to_f32(xb, True).astype(np.float64)
    w = 0.02 * rng.standard_normal((n, k))
    exact = x64 @ w.T
    xt = from_bits(xb, True)
    plain = decode_qact(offline.quantize_activations_cpu(xt, "mxfp4").data.numpy(), m, k, "mxfp4").astype(np.float64)
    err_plain = np.sqrt(np.mean((plain @ w.T - exact) ** 2))
    rot = decode_qact(offline.quantize_activations_cpu(xt, "mxfp4", hadamard=block).data.numpy(), m, k, "mxfp4").astype(np.float64)
    w_rot = (w.reshape(n, k // block, block) @ sylvester(block)).reshape(n, k) / block
    err_rot = np.sqrt(np.mean((rot @ w_rot.T - exact) ** 2))
    print(f"B={block}: rms error rotated {err_rot:.4e}, unrotated {err_plain:.4e}, ratio {err_rot / err_plain:.3f} (bound 0.75)")
    assert err_rot <= 0.75 * err_plain


def test_every_refusal_and_its_code():
    """Each refusal with its code, from the host twins and (refused before any launch) from the device entries; block 0 is the unrotated twin."""
    from petit_kernel import _lib
    L = _lib.lib
    buf = (C.c_uint8 * (1 << 17))()
    base = (C.addressof(buf) + 255) & ~255
    p = [C.c_void_p(base + 16384 * i) for i in range(6)]         # qa, y16, residual_out, x, residual, weight: aligned host scratch (zeros)
    off = C.c_void_p(base + 8)
    shape, kern, bad, ok = _lib.PETIT_ERROR_PROBLEM_SHAPE, _lib.PETIT_ERROR_KERNEL_SHAPE, _lib.PETIT_ERROR_BAD_ARGUMENT, _lib.PETIT_OK
    bf16, f16 = _lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP16

    def pair(host_fn, dev_fn, args, m_or_k_zero=False):
        host = host_fn(*args)
        if host != ok or m_or_k_zero:                             # (an accepted call would launch: only the twin runs those)
            assert dev_fn(*args, None) == host, (dev_fn.__name__, host)
        return host

    def rows(out=p[0], inp=p[3], r=2, k=256, a_type=bf16, block=32, ls=0):
        return pair(L.petit_hadamard_rows_host, L.petit_hadamard_rows, (out, inp, r, k, a_type, block, ls), r == 0 or k == 0)

    assert rows() == ok and rows(block=128, ls=-7, a_type=f16) == ok and rows(out=p[3]) == ok and rows(ls=126) == ok and rows(ls=-126) == ok
    for block in (0, 1, 16, 64, 256):
        assert rows(block=block) == bad
    assert rows(ls=127) == bad and rows(ls=-127) == bad
    assert rows(k=128) == shape and rows(k=384) == shape
    assert rows(a_type=_lib.PETIT_DTYPE_FP32) == kern
    assert rows(out=None) == bad and rows(inp=None) == bad and rows(out=off) == bad and rows(inp=off) == bad
    assert rows(r=0) == ok and rows(k=0) == ok

    def quant(qa=p[0], a=p[3], m=2, k=256, a_type=bf16, fmt=4, block=32):
        return pair(L.petit_quantize_activations_rot_host, L.petit_quantize_activations_rot, (qa, a, m, k, a_type, fmt, block), m == 0 or k == 0)

    assert quant() == ok and quant(fmt=8, block=128, a_type=f16) == ok
    for block in (1, 16, 64, 256):
        assert quant(block=block) == bad
    assert quant(fmt=6) == kern
    assert quant(k=128) == shape and quant(k=384) == shape
    assert quant(a_type=_lib.PETIT_DTYPE_FP32) == kern
    assert quant(qa=None) == bad and quant(a=None) == bad and quant(qa=off) == bad and quant(a=off) == bad
    assert quant(m=0) == ok and quant(k=0) == ok

    # the gathered form has no host twin: refusals straight from the device entry
    def gather(qa=p[0], a=p[3], idx=None, a_rows=2, m=2, k=256, a_type=bf16, fmt=4, block=32):
        return L.petit_quantize_activations_rows_rot(qa, a, idx, a_rows, m, k, a_type, fmt, block, None)

    for block in (1, 16, 64, 256):
        assert gather(block=block) == bad
    assert gather(fmt=6) == kern and gather(a_type=_lib.PETIT_DTYPE_FP32) == kern
    assert gather(k=384) == shape and gather(a_rows=1) == shape     # (a null index is the identity: its rows must exist)
    assert gather(qa=None) == bad and gather(a=None) == bad and gather(qa=off) == bad and gather(a=off) == bad
    assert gather(m=0) == ok and gather(k=0) == ok
    for block in (0, 32):                                          # block 0 hands the call on: the unrotated entry's own refusals
        assert gather(k=384, block=block) == L.petit_quantize_activations_rows(p[0], p[3], None, 2, 2, 384, bf16, 4, None) == shape

    def norm(qa=p[0], y16=p[1], res_out=p[2], x=p[3], res=p[4], w=p[5], eps=1e-6, woff=0.0, m=2, k=256, a_type=bf16, fmt=4, block=32):
        return pair(L.petit_rmsnorm_quantize_rot_host, L.petit_rmsnorm_quantize_rot, (qa, y16, res_out, x, res, w, eps, woff, m, k, a_type, fmt, block),
                    m == 0 or k == 0)

    assert norm() == ok and norm(y16=None, res_out=None, res=None, fmt=8, block=128, a_type=f16) == ok
    for block in (1, 16, 64, 256):
        assert norm(block=block) == bad
    assert norm(fmt=6) == kern and norm(fmt=6, block=0) == ok
    assert norm(k=384) == shape and norm(k=16384 + 256) == kern
    assert norm(a_type=_lib.PETIT_DTYPE_FP32) == kern
    assert norm(eps=0.0) == bad and norm(woff=float("nan")) == bad and norm(res=None) == bad and norm(fmt=5) == bad
    assert norm(qa=None) == bad and norm(x=None) == bad and norm(w=None) == bad
    for name in ("qa", "y16", "res_out", "x", "res", "w"):
        assert norm(**{name: off}) == bad, name
    assert norm(m=0) == ok and norm(k=0) == ok

    # block = 0 equals the unrotated twins' bytes
    m, k = 3, 512
    x = from_bits(mixed_input(m, k, True), True)
    w = torch.ones(k, dtype=torch.bfloat16)
    for fmt in (8, 6, 4):
        n = int(L.petit_quantized_activation_bytes(m, k, fmt))
        q0, q1 = torch.zeros(n, dtype=torch.uint8), torch.ones(n, dtype=torch.uint8)
        assert L.petit_quantize_activations_host(q0.data_ptr(), x.data_ptr(), m, k, bf16, fmt) == ok
        assert L.petit_quantize_activations_rot_host(q1.data_ptr(), x.data_ptr(), m, k, bf16, fmt, 0) == ok
        assert torch.equal(q0, q1)
        q1.fill_(1)
        assert L.petit_rmsnorm_quantize_host(q0.data_ptr(), None, None, x.data_ptr(), None, w.data_ptr(), 1e-6, 0.0, m, k, bf16, fmt) == ok
        assert L.petit_rmsnorm_quantize_rot_host(q1.data_ptr(), None, None, x.data_ptr(), None, w.data_ptr(), 1e-6, 0.0, m, k, bf16, fmt, 0) == ok
        assert torch.equal(q0, q1)


def test_python_layer_checks_and_exports():
    import petit_kernel as pk
    off = pk.offline
    assert "hadamard_rotate" in pk.__all__ and callable(pk.hadamard_rotate) and callable(off.hadamard_rotate_cpu) and callable(off.quantize_activations_cpu)
    assert callable(pk.ops.hadamard_rotate) and callable(pk.compiled.hadamard_rotate)
    x = torch.zeros(2, 256, dtype=torch.bfloat16)
    w = torch.ones(256, dtype=torch.bfloat16)
    q = off.quantize_activations_cpu(x, "mxfp4", hadamard=128)
    assert isinstance(q, pk.QuantizedActivations) and (q.m, q.k, q.fmt, q.hadamard) == (2, 256, "mxfp4", 128) and "hadamard=128" in repr(q)
    assert off.quantize_activations_cpu(x).hadamard == 0 and pk.QuantizedActivations(q.data, 2, 256, "mxfp4", x.dtype).hadamard == 0
    assert (qact_scales(q.data.numpy(), 2, 256, "mxfp4") == 127).all() and (q.data.numpy()[:2 * 256 // 2] == 0).all()   # a zero block stays zero
    assert off.rmsnorm_quantize_cpu(x, w, hadamard=32).hadamard == 32
    for bad in (dict(hadamard=64), dict(hadamard=-32), dict(hadamard=32.0), dict(fmt="mxfp6", hadamard=32)):
        with pytest.raises(RuntimeError, match="hadamard"):
            off.quantize_activations_cpu(x, **{"fmt": "mxfp4", **bad})
        with pytest.raises(RuntimeError, match="hadamard"):
            off.rmsnorm_quantize_cpu(x, w, **{"fmt": "mxfp4", **bad})
    with pytest.raises(RuntimeError, match="hadamard"):
        off.quantize_mxfp4_cpu(torch.zeros(32, 256, dtype=torch.bfloat16), hadamard=64)
    with pytest.raises(RuntimeError, match="block must be 32 or 128"):
        off.hadamard_rotate_cpu(x, 0)
    with pytest.raises(RuntimeError, match="log2_scale"):
        off.hadamard_rotate_cpu(x, 32, 127)
    with pytest.raises(RuntimeError, match="multiple of 256"):
        off.hadamard_rotate_cpu(torch.zeros(2, 384, dtype=torch.bfloat16), 32)
    with pytest.raises(RuntimeError):
        off.hadamard_rotate_cpu(x.float(), 32)
    with pytest.raises(RuntimeError, match="out must be"):
        off.hadamard_rotate_cpu(x, 32, out=torch.zeros(2, 256, dtype=torch.float16))
    out = torch.empty_like(x)
    assert off.hadamard_rotate_cpu(x, 32, out=out) is out
    assert off.hadamard_rotate_cpu(torch.zeros(2, 3, 256, dtype=torch.float16), 128, -7).shape == (2, 3, 256)
    for fn in (pk.ops.hadamard_rotate, pk.hadamard_rotate):
        with pytest.raises(RuntimeError):
            fn(x, 32)                                              # CPU tensors: the device form wants GPU tensors
    with pytest.raises(RuntimeError):
        pk.quantize_activations(x, "mxfp4", hadamard=32)


# --- on the GPU -----------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pk():
    import petit_kernel
    assert torch.cuda.is_available()
    name = torch.cuda.get_device_properties(0).gcnArchName
    assert name.startswith("gfx950"), f"these kernels are gfx950 code objects, device is {name}"
    return petit_kernel


MS, KS = (1, 33), (256, 2304, 8448)      # two k-tiles; a ragged share of a workgroup's columns; a second workgroup along k


@pytest.mark.gpu
@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("block", BLOCKS)
def test_device_rotation_equals_host_twin(pk, block, is_bf16):
    """hadamard_rotate (both Python layers) byte for byte, with scale 1 and with 2^-log2(B)."""
    for m in MS:
        for k in KS:
            xd = from_bits(mixed_input(m, k, is_bf16), is_bf16).to(DEV)
            for ls in (0, -(block.bit_length() - 1)):
                want = twin_rotate(m, k, is_bf16, block, ls)
                for layer in (pk.ops, pk.compiled):
                    got = bits(layer.hadamard_rotate(xd, block, ls))
                    assert np.array_equal(got, want), f"m={m} k={k} ls={ls}: {int((got != want).sum())} elements differ"


@pytest.mark.gpu
@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4"])
def test_device_quantisers_equal_host_twin(pk, fmt, block, is_bf16):
    """quantize_activations and quantize_activation_rows (identity rows) with a rotation, byte for byte."""
    for m in MS:
        for k in KS:
            xd = from_bits(mixed_input(m, k, is_bf16), is_bf16).to(DEV)
            want = twin_qact(m, k, is_bf16, fmt, block)
            q = pk.quantize_activations(xd, fmt, hadamard=block)
            got = q.data.cpu().numpy()
            assert q.hadamard == block and np.array_equal(got, want), f"dense m={m} k={k}: {int((got != want).sum())} bytes differ"
            got = pk.quantize_activation_rows(xd, fmt, hadamard=block).data.cpu().numpy()
            assert np.array_equal(got, want), f"rows m={m} k={k}: {int((got != want).sum())} bytes differ"


@pytest.mark.gpu
@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4"])
def test_device_norm_equals_host_twin(pk, fmt, block, is_bf16, with_res):
    """rmsnorm_quantize with a rotation against offline.rmsnorm_quantize_cpu: qa, y16 and residual_out byte for byte, every ILP form
    (k = 256 and 2304 | 4352 | 8448 | -- and 2304 leaves lanes idle)."""
    from petit_kernel import offline
    for m in MS:
        for k in KS + (4352,):
            x = from_bits(mixed_input(m, k, is_bf16), is_bf16)
            r = from_bits(mixed_input(m, k, is_bf16, seed=1), is_bf16) if with_res else None
            w = from_bits(round16((1.0 + 0.1 * np.random.default_rng(k).standard_normal(k)).astype(np.float32), is_bf16), is_bf16)
            want = offline.rmsnorm_quantize_cpu(x, w, 1e-6, fmt, residual=r, return_normed=True, hadamard=block)
            got = pk.rmsnorm_quantize(x.to(DEV), w.to(DEV), 1e-6, fmt, residual=None if r is None else r.to(DEV), return_normed=True, hadamard=block)
            assert got[0].hadamard == block
            assert torch.equal(got[0].data.cpu(), want[0].data), f"m={m} k={k}: qa differs"
            for g, t in zip(got[1:], want[1:]):
                assert np.array_equal(bits(g), bits(t)), f"m={m} k={k}: a 16-bit output differs"


@pytest.mark.gpu
@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4"])
def test_gathered_form(pk, fmt, block):
    """quantize_activation_rows(a, fmt, idx, hadamard=B) == quantize_activations(a[idx], fmt, hadamard=B): repeated, out-of-order and one
    out-of-range index, which gives a zero row with scale byte 127."""
    m, k = 5, 512
    a = from_bits(mixed_input(4, k, True), True).to(DEV)
    idx = torch.tensor([2, 0, 2, 7, 1], dtype=torch.int32, device=DEV)
    got = pk.quantize_activation_rows(a, fmt, idx, hadamard=block)
    gathered = a[idx.clamp(max=3).long()].contiguous()
    gathered[3] = 0
    want = pk.quantize_activations(gathered, fmt, hadamard=block)
    assert (got.m, got.k, got.hadamard) == (m, k, block) and torch.equal(got.data, want.data)
    raw = got.data.cpu().numpy()
    elems, scales = qact_tiles(raw, m, k, fmt)
    assert (scales[:, 3] == 127).all() and (elems[:, 3] == 0).all()
    assert np.array_equal(raw, pk.offline.quantize_activations_cpu(gathered.cpu(), fmt, hadamard=block).data.numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4"])
def test_fused_norm_equals_the_chain(pk, fmt, block):
    """rmsnorm_quantize(..., hadamard=B, return_normed=True): its bytes are quantize_activations(y16, hadamard=B); y16 and residual_out are
    those of the unrotated call."""
    for m, k in ((33, 768), (5, 4352)):
        xd = from_bits(mixed_input(m, k, True), True).to(DEV)
        rd = from_bits(mixed_input(m, k, True, seed=1), True).to(DEV)
        wd = torch.from_numpy(1.0 + 0.1 * np.random.default_rng(k).standard_normal(k)).to(torch.bfloat16).to(DEV)
        q, ro, y = pk.rmsnorm_quantize(xd, wd, 1e-5, fmt, residual=rd, return_normed=True, hadamard=block)
        _, ro0, y0 = pk.rmsnorm_quantize(xd, wd, 1e-5, fmt, residual=rd, return_normed=True)
        assert torch.equal(q.data, pk.quantize_activations(y, fmt, hadamard=block).data), (m, k)
        assert np.array_equal(bits(y), bits(y0)) and np.array_equal(bits(ro), bits(ro0))


@pytest.mark.gpu
def test_block_zero_and_defaults_are_the_existing_entries(pk):
    from petit_kernel import _lib
    L = _lib.lib
    m, k = 33, 2304
    xd = from_bits(mixed_input(m, k, True), True).to(DEV)
    rd = from_bits(mixed_input(m, k, True, seed=1), True).to(DEV)
    wd = torch.ones(k, dtype=torch.bfloat16, device=DEV)
    idx = torch.arange(m - 1, -1, -1, dtype=torch.int32, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for fmt, code in (("mxfp8", 8), ("mxfp6", 6), ("mxfp4", 4)):
        base = pk.quantize_activations(xd, fmt)
        assert base.hadamard == 0 and torch.equal(base.data, pk.quantize_activations(xd, fmt, hadamard=0).data)
        qa = torch.empty_like(base.data)
        assert L.petit_quantize_activations_rot(qa.data_ptr(), xd.data_ptr(), m, k, _lib.CXX_DTYPE_BF16, code, 0, stream) == _lib.PETIT_OK
        assert torch.equal(qa, base.data)
        rows = pk.quantize_activation_rows(xd, fmt, idx)
        assert torch.equal(rows.data, pk.quantize_activation_rows(xd, fmt, idx, hadamard=0).data)
        qa.zero_()
        assert L.petit_quantize_activations_rows_rot(qa.data_ptr(), xd.data_ptr(), idx.data_ptr(), m, m, k, _lib.CXX_DTYPE_BF16, code, 0,
                                                     stream) == _lib.PETIT_OK
        assert torch.equal(qa, rows.data)
        fused = pk.rmsnorm_quantize(xd, wd, 1e-6, fmt, residual=rd)
        fused0 = pk.rmsnorm_quantize(xd, wd, 1e-6, fmt, residual=rd, hadamard=0)
        assert torch.equal(fused[0].data, fused0[0].data) and torch.equal(fused[1], fused0[1])
        qa.zero_()
        assert L.petit_rmsnorm_quantize_rot(qa.data_ptr(), None, None, xd.data_ptr(), None, wd.data_ptr(), 1e-6, 0.0, m, k, _lib.CXX_DTYPE_BF16,
                                            code, 0, stream) == _lib.PETIT_OK
        assert torch.equal(qa, pk.rmsnorm_quantize(xd, wd, 1e-6, fmt).data)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4"])
def test_a_non_finite_element_spoils_only_its_rotation_block(pk, fmt):
    """One inf in block 3 of a row with k = 512, B = 128: every other k-tile's bytes equal those of the row with that element set to zero."""
    m, k, block = 2, 512, 128
    x = to_f32(mixed_input(m, k, True), True).copy()
    x[1, 3 * 128 + 17] = 0.0
    clean = from_bits(round16(x, True), True)
    dirty = clean.clone()
    dirty[1, 3 * 128 + 17] = float("inf")
    e0, s0 = qact_tiles(pk.quantize_activations(clean.to(DEV), fmt, hadamard=block).data.cpu().numpy(), m, k, fmt)
    e1, s1 = qact_tiles(pk.quantize_activations(dirty.to(DEV), fmt, hadamard=block).data.cpu().numpy(), m, k, fmt)
    assert np.array_equal(e0[:3], e1[:3]) and np.array_equal(s0[:3], s1[:3])
    assert np.array_equal(e0[3, 0], e1[3, 0]) and np.array_equal(s0[3, 0], s1[3, 0])      # (the other row of the same k-tile too)


@pytest.mark.gpu
def test_native_gemms_consume_rotated_activations(pk):
    """mul_mxfp4_native and mul_nvfp4_native, bf16, m = 33, n = 256, k = 512, on weights from quantize_*(w, hadamard=128): the device's rotated
    QuantizedActivations and the twin's bytes, uploaded, give bit-identical results; on the MXFP4 weights the result matches the float64
    product of the dequantised operands within the native class's derived bound; eagerly and from a captured graph."""
    m, n, k, block, fmt = 33, 256, 512, 128, "mxfp4"
    rng = np.random.default_rng(77)
    xd = from_bits(mixed_input(m, k, True), True).to(DEV)
    w = torch.from_numpy((0.05 * rng.standard_normal((n, k))).astype(np.float32)).bfloat16().to(DEV)
    twin = twin_qact(m, k, True, fmt, block)
    q_twin = pk.QuantizedActivations(torch.from_numpy(twin.copy()).to(DEV), m, k, fmt, torch.bfloat16, block)
    b, s, gs = pk.quantize_mxfp4(w, hadamard=block)
    bn, sn, gsn = pk.quantize_nvfp4(w, hadamard=block)
    image = pk.nvfp4_native_image(bn, sn, n, k)
    sid = pk.SOLUTION_AUTO_NATIVE_MXFP4
    pk.ops.enable_native_fp4(True)
    try:
        def run_mx(q=None):
            return pk.mul_mxfp4_native(pk.quantize_activations(xd, fmt, hadamard=block) if q is None else q, b, s, gs, m, n, k, sid)

        def run_nv(q=None):
            return pk.mul_nvfp4_native(pk.quantize_activations(xd, fmt, hadamard=block) if q is None else q, image, gsn, m, n, k, sid)

        c_mx, c_nv = run_mx(), run_nv()
        assert torch.equal(c_mx.view(torch.int16), run_mx(q_twin).view(torch.int16))
        assert torch.equal(c_nv.view(torch.int16), run_nv(q_twin).view(torch.int16))
        # the float64 product of the dequantised operands, and the bound tests/test_gpu_parity.py derives for the class
        a_q = decode_qact(twin, m, k, fmt)
        w_dq = pk.ops.dequant_packed(b, s, n, k, "mxfp4").cpu().numpy()
        g = float(gs.cpu()[0])
        exact = a_q.astype(np.float64) @ w_dq.astype(np.float64).T * g
        derived = native_exact_bound(a_q, w_dq, g, fmt)
        err = np.abs(c_mx.float().cpu().numpy().astype(np.float64) - exact)
        print(f"max |err| {err.max():.3e}, max of the bound {np.maximum(np.maximum(1e-2, 1e-2 * np.abs(exact)), derived).max():.3e}")
        assert (err <= np.maximum(np.maximum(1e-2, 1e-2 * np.abs(exact)), derived)).all()
        # ... and it is the unrotated layer's product up to the two quantisers: x . W^T from the 16-bit operands
        full = xd.double().cpu().numpy() @ w.double().cpu().numpy().T
        assert np.sqrt(np.mean((c_mx.double().cpu().numpy() - full) ** 2)) <= 0.5 * np.sqrt(np.mean(full ** 2))
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            run_mx(), run_nv()
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                g_mx, g_nv = run_mx(), run_nv()
            graph.replay()
            stream.synchronize()
        assert torch.equal(g_mx.view(torch.int16), c_mx.view(torch.int16)) and torch.equal(g_nv.view(torch.int16), c_nv.view(torch.int16))
    finally:
        pk.ops.enable_native_fp4(False)


@pytest.mark.gpu
@pytest.mark.parametrize("is_bf16", [True, False])
def test_in_place_rotation(pk, is_bf16):
    m, k = 33, 2304
    for block in BLOCKS:
        xd = from_bits(mixed_input(m, k, is_bf16), is_bf16).to(DEV)
        want = twin_rotate(m, k, is_bf16, block, 0)
        assert pk.hadamard_rotate(xd, block, 0, out=xd) is xd and np.array_equal(bits(xd), want)
        xd = from_bits(mixed_input(m, k, is_bf16), is_bf16).to(DEV)
        assert pk.ops.hadamard_rotate(xd, block, 0, out=xd) is xd and np.array_equal(bits(xd), want)

"""MXFP6 weights on the native class (include/petit_amd.h; csrc/mxfp6_weights.hip): the host twins against a plain float64 statement of the rule,
the device kernel against the twins bit for bit (every byte of the image written), the OCP ingest, the image as a GEMM operand, the refusals.
Every value involved is an f32 number, so every comparison is exact equality.  fp16 cannot hold 2^+-40: its "far" blocks sit at the ends of its
normal range (2^12 and 2^-14: scale bytes 139 and 113, still outside the 115 .. 136 an NVFP4-derived image can contain)."""
import ctypes as C
import sys

import numpy as np
import pytest
import torch

from petit_kernel import _lib, offline
from test_gpu_parity import ROOT, pk  # noqa: F401  (the module's GPU fixture)
from test_native_invariant_abi import BAD, BF16, FP16, OK, PTR, SHAPE, dt, host_quantize, to16
from test_nvfp4_native_invariant_abi import exact_activations, twin

sys.path.insert(0, str(ROOT / "tools"))
import quantize_weights as QW  # noqa: E402

L = _lib.lib
gpu = pytest.mark.gpu
CASES = [(E, n, k, bf) for E in (1, 3) for n in (32, 80) for k in (256, 512, 1024) for bf in (True, False)]   # span_tiles_for_k: 2, 4, 8
IDS = ["E%d-n%d-k%d-%s" % (E, n, k, "bf16" if bf else "fp16") for E, n, k, bf in CASES]
FAR = {True: (40, -40), False: (12, -14)}


def reference(w: np.ndarray) -> np.ndarray:
    """The rule in float64: per 32 k, E = floor(log2 amax) - 2 (byte clamped into [1, 254]; a zero block: byte 127), round to nearest even on the
    e2m3 grid of w / 2^E (steps 1/8 below 2, 1/4 below 4, 1/2 above), saturating at 7.5, times 2^E."""
    b = w.reshape(-1, 32)
    amax = np.abs(b).max(axis=1, keepdims=True)
    E = np.where(amax > 0, np.clip(np.frexp(amax)[1] - 3, -126, 127), 0).astype(np.float64)
    a = np.abs(b) / np.exp2(E)
    step = np.exp2(np.clip(np.frexp(a)[1] - 1, 0, 2) - 3.0)
    return (np.copysign(np.minimum(np.rint(a / step) * step, 7.5), b) * np.exp2(E)).reshape(w.shape)


def weights(E, n, k, is_bf16):
    """[E, n, k] 16-bit tensor: the checkpoint-like draw, and in block 0 of rows 0 .. 4 of every expert an all-zero block, exact ties of the
    grid, a maximum that rounds up across the power of two (saturation), and the two far blocks."""
    rng = np.random.default_rng([E, n, k])
    w = QW.synthetic_weights(E * n, k, seed=n + k).astype(np.float64).reshape(E, n, k)
    ties = np.array([6.0, 1.0625, -1.1875, 2.125, -2.375, 4.25, -4.75, 7.25, 0.0625, -0.1875, 0.9375, -0.0, 7.5, -6.75, 3.625, 1.9375])
    far = rng.integers(16, 121, (2, 32)) / 16.0 * rng.choice([-1.0, 1.0], (2, 32))
    w[:, 0, :32] = 0.0
    w[:, 1, :32] = np.tile(ties, 2) * 0.25
    w[:, 2, :32] = np.tile([7.75, -7.875, 7.5, -7.625, 1.0, 0.5, -3.0, 7.9375], 4) * 8.0
    w[:, 3, :32], w[:, 4, :32] = far[0] * 2.0 ** FAR[is_bf16][0], far[1] * 2.0 ** FAR[is_bf16][1]
    t = torch.from_numpy(w).to(dt(is_bf16))
    assert np.array_equal(t[:, :5, :32].double().numpy(), w[:, :5, :32])                # (both types hold the special blocks exactly)
    return t


def dequant(images: torch.Tensor, E, n, k) -> np.ndarray:
    """-> float64 [E, n32, k]: every row of every image, the padding rows of the last 32-row block included"""
    n32 = (n + 31) // 32 * 32
    return np.stack([offline.nvfp4_native_image_dequant_cpu(img, n32, k).double().numpy() for img in images.cpu().view(E, -1)])


def ocp_tensor(E, n, k):
    """random 6-bit codes and scale bytes in [1, 254] -> (elems uint8 [E, n, 3 k / 4], scales uint8 [E, n, k / 32], the values as f32 numbers:
    4 x 2^126 and above is +-inf there, as in the image's own f32 expansion)"""
    rng = np.random.default_rng([7, E, n, k])
    code, sb = rng.integers(0, 64, (E, n, k)), rng.integers(1, 255, (E, n, k // 32)).astype(np.uint8)
    bits = ((code[..., None] >> np.arange(6)) & 1).astype(np.uint8).reshape(E, n, 6 * k)
    mag = np.where(code & 24, (8 + (code & 7)) / 8.0 * np.exp2(((code >> 3) & 3) - 1.0), (code & 7) / 8.0)
    val = np.where(code & 32, -mag, mag) * np.repeat(np.exp2(sb.astype(np.float64) - 127), 32, axis=2)
    with np.errstate(over="ignore"):
        val = val.astype(np.float32).astype(np.float64)
    return torch.from_numpy(np.packbits(bits, axis=2, bitorder="little")), torch.from_numpy(sb), val


@pytest.mark.parametrize("E,n,k,is_bf16", CASES, ids=IDS)
def test_host_twin_equals_the_reference(E, n, k, is_bf16):
    w = weights(E, n, k, is_bf16)
    got = dequant(offline.quantize_mxfp6_cpu(w if E > 1 else w[0]), E, n, k)
    assert np.array_equal(got[:, :n], reference(w.double().numpy())) and not got[:, n:].any()


@gpu
@pytest.mark.parametrize("E,n,k,is_bf16", CASES, ids=IDS)
def test_device_image_is_the_twins(pk, E, n, k, is_bf16):
    w = weights(E, n, k, is_bf16)
    want, wd = offline.quantize_mxfp6_cpu(w), w.cuda()
    buf = torch.full((want.numel() + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    assert L.petit_quantize_weights_mxfp6(wd.data_ptr(), BF16 if is_bf16 else FP16, E, n, k, buf.data_ptr(), None) == OK
    torch.cuda.synchronize()
    assert torch.equal(buf[:want.numel()].cpu(), want) and bool((buf[want.numel():] == 0xFF).all())
    assert torch.equal(pk.quantize_mxfp6(wd).cpu(), want) and torch.equal(pk.ops.quantize_mxfp6(wd).cpu(), want)


@pytest.mark.parametrize("E,n,k", [c[:3] for c in CASES[::2]], ids=[i[:-5] for i in IDS[::2]])
def test_ingest_host_is_exact(E, n, k):
    elems, scales, val = ocp_tensor(E, n, k)
    got = dequant(offline.mxfp6_native_image_cpu(elems, scales, n, k), E, n, k)
    assert np.array_equal(got[:, :n], val) and not got[:, n:].any()


@gpu
@pytest.mark.parametrize("E,n,k", [c[:3] for c in CASES[::2]], ids=[i[:-5] for i in IDS[::2]])
def test_ingest_device_is_the_twins(pk, E, n, k):
    elems, scales, _ = ocp_tensor(E, n, k)
    want, ed, sd = offline.mxfp6_native_image_cpu(elems, scales, n, k), elems.cuda(), scales.cuda()
    buf = torch.full((want.numel() + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    assert L.petit_mxfp6_native_images(buf.data_ptr(), ed.data_ptr(), sd.data_ptr(), E, n, k, None) == OK
    torch.cuda.synchronize()
    assert torch.equal(buf[:want.numel()].cpu(), want) and bool((buf[want.numel():] == 0xFF).all())
    assert torch.equal(pk.mxfp6_native_image(ed, sd, n, k).cpu(), want) and torch.equal(pk.ops.mxfp6_native_image(ed, sd, n, k).cpu(), want)


@gpu
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4"])
@pytest.mark.parametrize("k", [256, 1024])
def test_image_is_a_gemm_operand(pk, k, fmt):
    """mul_nvfp4_native_invariant / _moe_invariant on quantize_mxfp6 images, global scale 1.0: bit for bit the host twins on the same image and
    the same quantised activations.  The twins state the device's bits where every partial sum is exact, so the weights are eighths up to 7.5
    times 2^-1 .. 2^1 per block (the image then holds sixteenths) and the activations exact_activations' halves; rows 3 and 4 of every expert
    are that times 2^40 and 2^-40 -- scale bytes no NVFP4-derived image holds; bf16, so every result is finite."""
    E, n = 3, 64
    rng = np.random.default_rng([k, 4])
    w = rng.integers(-60, 61, (E, n, k // 32, 32)) / 8.0 * np.exp2(rng.integers(-1, 2, (E, n, k // 32, 1)))
    w = w.reshape(E, n, k)
    w[:, 3], w[:, 4] = w[:, 3] * 2.0 ** 40, w[:, 4] * 2.0 ** -40
    wt = torch.from_numpy(w).bfloat16()
    images_h, images = offline.quantize_mxfp6_cpu(wt), pk.quantize_mxfp6(wt.cuda())
    assert torch.equal(images.cpu(), images_h)
    per, ones = images_h.numel() // E, torch.ones(E, dtype=torch.float32, device="cuda")
    a64, wi = exact_activations(33, k, 3), dequant(images_h, E, n, k)
    wi[:, 3], wi[:, 4] = wi[:, 3] * 2.0 ** -40, wi[:, 4] * 2.0 ** 40
    assert (np.abs(a64) @ np.abs(wi.reshape(E * n, k)).T).max() < 2 ** 19                          # units of 2^-5: every partial sum is exact
    a, bits = torch.from_numpy(a64).bfloat16(), to16(a64, True)
    for m in (1, 33):
        got = pk.mul_nvfp4_native_invariant(a[:m].cuda(), images[:per], ones[:1], m, n, k, fmt).cpu()
        want = twin(host_quantize(bits[:m], True, fmt), images_h[:per], 1.0, None, m, n, k, True, fmt)
        assert np.isfinite(got.float().numpy()).all() and np.array_equal(got.view(torch.int16).numpy().view(np.uint16), want)
    m, off = 9, torch.tensor([0, 5, 5, 9], dtype=torch.int32)                                       # expert 1 has no rows
    got = pk.mul_nvfp4_native_moe_invariant(a[:m].cuda(), images, ones, off.cuda(), m, n, k, E, fmt=fmt).cpu()
    want, qa, gs = np.zeros((m, n), dtype=np.uint16), host_quantize(bits[:m], True, fmt), np.ones(E, dtype=np.float32)
    assert L.petit_gemm_nvfp4_native_moe_invariant_host(want.ctypes.data, qa.ctypes.data, images_h.data_ptr(), gs.ctypes.data, None,
                                                        off.data_ptr(), E, m, n, k, None, m, BF16, int(fmt[-1])) == OK
    assert np.array_equal(got.view(torch.int16).numpy().view(np.uint16), want)


@pytest.mark.parametrize("args,code", [((1, 32, 384), SHAPE), ((0, 32, 256), SHAPE), ((1, 32, 256), BAD)], ids=["k%256", "no experts", "misaligned"])
def test_refusals(args, code):
    """k % 256 and num_experts == 0 on good pointers; then a good shape with the image 16 bytes off its 256-byte alignment"""
    img = PTR if code == SHAPE else C.c_void_p(PTR.value + 16)
    assert L.petit_quantize_weights_mxfp6(PTR, BF16, *args, img, None) == code and L.petit_mxfp6_native_images(img, PTR, PTR, *args, None) == code
    if code == SHAPE:
        assert L.petit_quantize_weights_mxfp6_host(PTR, BF16, *args, PTR) == code and L.petit_mxfp6_native_images_host(PTR, PTR, PTR, *args) == code
    else:
        assert L.petit_quantize_weights_mxfp6(C.c_void_p(PTR.value + 8), BF16, *args, PTR, None) == BAD           # w off its 16-byte alignment

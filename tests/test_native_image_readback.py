"""Reading a native image back (include/petit_amd.h; csrc/native_image_readback.hip): the host twins of the export and of the dequantiser against
the OCP tensor an image was made from, the device kernel against the twins byte for byte behind a guard, the refusals.  Every value is an f32
number and every expected result one rounding of it, so every comparison is equality of bits (the sign of a zero included)."""
import ctypes as C

import pytest
import torch

from petit_kernel import _lib, offline
from test_mxfp6_weights import BAD, OK, PTR, SHAPE, ocp_tensor, pk, reference, weights  # noqa: F401  (pk: the module's GPU fixture)

L = _lib.lib
gpu = pytest.mark.gpu
cases = pytest.mark.parametrize("E,n,k", [(E, n, k) for E in (1, 3) for n in (32, 80) for k in (256, 512, 1024)])   # span_tiles_for_k: 2, 4, 8
DTYPES = {torch.float32: _lib.PETIT_DTYPE_FP32, torch.bfloat16: _lib.CXX_DTYPE_BF16, torch.float16: _lib.CXX_DTYPE_FP16}
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
GS = torch.tensor([0.75, 3.0, 1 / 3], dtype=torch.float32)


def same_bits(got: torch.Tensor, want: torch.Tensor) -> bool:
    return got.dtype == want.dtype and torch.equal(got.cpu().reshape(want.shape).view(BITS[want.dtype]), want.view(BITS[want.dtype]))


def guarded(nbytes: int) -> torch.Tensor:
    return torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device="cuda")


def holds(buf: torch.Tensor, want: torch.Tensor) -> bool:
    """the bytes of want at the front of buf, and the 256-byte guard behind them intact"""
    nb = want.numel() * want.element_size()
    return torch.equal(buf[:nb].cpu(), want.reshape(-1).view(torch.uint8)) and bool((buf[nb:] == 0xFF).all())


@cases
def test_export_twin_inverts_the_ingest(E, n, k):
    elems, scales, _ = ocp_tensor(E, n, k)
    img = offline.mxfp6_native_image_cpu(elems, scales, n, k)
    got_e, got_s = offline.mxfp6_export_cpu(img, n, k)
    assert torch.equal(got_e.reshape(elems.shape), elems) and torch.equal(got_s.reshape(scales.shape), scales)
    assert torch.equal(offline.mxfp6_native_image_cpu(got_e, got_s, n, k), img)


@cases
def test_dequant_twin_is_the_tensors_values(E, n, k):
    elems, scales, val = ocp_tensor(E, n, k)
    img, v32 = offline.mxfp6_native_image_cpu(elems, scales, n, k), torch.from_numpy(val).float()
    assert same_bits(offline.dequant_native_image_cpu(img, n, k, torch.float32), v32)
    assert torch.equal(v32.bfloat16().float(), v32)                                     # (bf16 holds every value of an image)
    assert same_bits(offline.dequant_native_image_cpu(img, n, k, torch.bfloat16), v32.bfloat16())
    half = torch.from_numpy(val).half()
    mag = half.view(torch.int16) & 0x7FFF
    assert bool((mag == 0x7C00).any()) and bool(((mag > 0) & (mag < 0x400)).any()) and bool((mag == 0).any())   # +-inf, subnormals, zeros
    assert same_bits(offline.dequant_native_image_cpu(img, n, k, torch.float16), half)
    for dtype in DTYPES:
        assert same_bits(offline.dequant_native_image_cpu(img, n, k, dtype, GS[:E]), (v32 * GS[:E, None, None]).to(dtype))


@pytest.mark.parametrize("args,code", [((1, 32, 384), SHAPE), ((0, 32, 256), SHAPE), ((1, 32, 256), BAD)], ids=["k%256", "no experts", "misaligned"])
def test_refusals(args, code):
    """k % 256 and num_experts == 0 on good pointers, a bad out_type before either; then a good shape with the image 16 bytes off its 256-byte
    alignment, and with the output off its 16-byte alignment"""
    bf16, img = DTYPES[torch.bfloat16], PTR if code == SHAPE else C.c_void_p(PTR.value + 16)
    assert L.petit_native_images_dequant(PTR, bf16, img, None, *args, None) == code and L.petit_mxfp6_export_images(PTR, PTR, img, *args, None) == code
    if code == SHAPE:
        assert L.petit_native_images_dequant_host(PTR, bf16, PTR, None, *args) == code and L.petit_mxfp6_export_images_host(PTR, PTR, PTR, *args) == code
        assert L.petit_native_images_dequant(PTR, 7, PTR, None, *args, None) == BAD and L.petit_native_images_dequant_host(PTR, 7, PTR, None, *args) == BAD
    else:
        off = C.c_void_p(PTR.value + 8)
        assert L.petit_native_images_dequant(off, bf16, PTR, None, *args, None) == BAD and L.petit_mxfp6_export_images(off, PTR, PTR, *args, None) == BAD


@gpu
@cases
def test_device_dequant_is_the_twins(pk, E, n, k):
    elems, scales, _ = ocp_tensor(E, n, k)
    img = offline.mxfp6_native_image_cpu(elems, scales, n, k)
    imgd, gsd = img.cuda(), GS[:E].cuda()
    for dtype, code in DTYPES.items():
        for gs, gd in ((None, None), (GS[:E], gsd)):
            want = offline.dequant_native_image_cpu(img, n, k, dtype, gs)
            buf = guarded(want.numel() * want.element_size())
            assert L.petit_native_images_dequant(buf.data_ptr(), code, imgd.data_ptr(), None if gd is None else gd.data_ptr(), E, n, k, None) == OK
            torch.cuda.synchronize()
            assert holds(buf, want)
            for f in (pk.dequant_native_image, pk.ops.dequant_native_image, torch.ops.petit_kernel.dequant_native_image):
                assert same_bits(f(imgd, n, k, dtype, gd), want)


@gpu
@cases
def test_device_export_is_the_twins(pk, E, n, k):
    elems, scales, _ = ocp_tensor(E, n, k)
    imgd = offline.mxfp6_native_image_cpu(elems, scales, n, k).cuda()
    be, bs = guarded(elems.numel()), guarded(scales.numel())
    assert L.petit_mxfp6_export_images(be.data_ptr(), bs.data_ptr(), imgd.data_ptr(), E, n, k, None) == OK
    torch.cuda.synchronize()
    assert holds(be, elems) and holds(bs, scales)
    for f in (pk.mxfp6_export, pk.ops.mxfp6_export, torch.ops.petit_kernel.mxfp6_export):
        got_e, got_s = f(imgd, n, k)
        assert torch.equal(got_e.cpu().reshape(elems.shape), elems) and torch.equal(got_s.cpu().reshape(scales.shape), scales)


@gpu
@cases
def test_the_loop_closes_on_real_weights(pk, E, n, k):
    """quantise -> export -> image again gives the same image; quantise -> dequantise gives the rule's values (test_mxfp6_weights.reference)"""
    w = weights(E, n, k, True)
    img = pk.quantize_mxfp6(w.cuda())
    assert torch.equal(pk.mxfp6_native_image(*pk.mxfp6_export(img, n, k), n, k), img)
    got = pk.dequant_native_image(img, n, k, torch.float32).cpu().reshape(E, n, k)
    assert torch.equal(got.double(), torch.from_numpy(reference(w.double().numpy())))

"""moe_combine_rmsnorm(..., hadamard=B): byte for byte moe_combine -> rmsnorm_quantize(..., residual=..., hadamard=B); twin == device."""
import pytest
import torch

from test_moe_combine_rmsnorm import E, combine_np, make_case
from test_rmsnorm_quantize import from_bits

DEV = "cuda"
CASES = [(5, 512, 2), (70, 512, 2)]


def _case(T, k, topk):
    slot, tw, ids, res, w = make_case(T, k, topk, True, 3000 + T)
    ids[0, 1] = -1
    return slot, tw, ids, res, w


def _same(a, b):
    return all(torch.equal(x.cpu().view(torch.uint8), y.cpu().view(torch.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("T,k,topk", CASES)
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4"])
@pytest.mark.parametrize("B", [32, 128])
def test_host_twin_equals_the_chain(B, fmt, T, k, topk):
    from petit_kernel import offline
    slot, tw, ids, res, w = _case(T, k, topk)
    args = (torch.from_numpy(tw), torch.from_numpy(ids), E, from_bits(w, True), 1e-5, fmt)
    q, h, y = offline.moe_combine_rmsnorm_cpu(from_bits(slot, True), *args, residual=from_bits(res, True), return_normed=True, hadamard=B)
    q2, h2, y2 = offline.rmsnorm_quantize_cpu(from_bits(combine_np(slot, tw, ids, True), True), from_bits(w, True), 1e-5, fmt,
                                              residual=from_bits(res, True), return_normed=True, hadamard=B)
    assert q.hadamard == B and _same((q.data, h, y), (q2.data, h2, y2))
    for bad_fmt, bad_block in (("mxfp6", B), (None, B), (fmt, 64)):
        with pytest.raises(RuntimeError):
            offline.moe_combine_rmsnorm_cpu(from_bits(slot, True), *args[:5], bad_fmt, hadamard=bad_block)


@pytest.mark.gpu
@pytest.mark.parametrize("T,k,topk", CASES)
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4"])
@pytest.mark.parametrize("B", [32, 128])
def test_device_equals_the_chain_and_the_twin(B, fmt, T, k, topk):
    import petit_kernel as pk
    from petit_kernel import offline
    slot, tw, ids, res, w = _case(T, k, topk)
    cpu = (from_bits(slot, True), torch.from_numpy(tw), torch.from_numpy(ids), from_bits(res, True), from_bits(w, True))
    sd, twd, idd, rd, wd = (t.to(DEV) for t in cpu)
    q, h, y = pk.moe_combine_rmsnorm(sd, twd, idd, E, wd, 1e-5, fmt, residual=rd, return_normed=True, hadamard=B)
    q2, h2, y2 = pk.rmsnorm_quantize(pk.moe_combine(sd, twd, idd, E), wd, 1e-5, fmt, residual=rd, return_normed=True, hadamard=B)
    assert q.hadamard == B and _same((q.data, h, y), (q2.data, h2, y2))
    qt, ht, yt = offline.moe_combine_rmsnorm_cpu(cpu[0], cpu[1], cpu[2], E, cpu[4], 1e-5, fmt, residual=cpu[3], return_normed=True, hadamard=B)
    assert _same((q.data, h, y), (qt.data, ht, yt))

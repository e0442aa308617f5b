#!/usr/bin/env python3
"""examples/mxfp6_linear.py -- MXFP6 weights on the native class (include/petit_amd.h "MXFP6 weights on the native class"): a bf16 linear
quantised on the device by quantize_mxfp6, run as RMSNorm -> MXFP8 activations -> the batch-invariant native-class GEMM (up to 32 rows: the
decode GEMM on the image, mul_nvfp4_native_decode), and a layer of
stacked experts through the batch-invariant MoE launch.  Needs an MI355X.

    python examples/mxfp6_linear.py

quantize_mxfp6 writes the MFMA-native image the NVFP4 path already runs on (FP6 e2m3 elements, one E8M0 scale per 32 k) straight from the
16-bit weights: 6.25 bits per weight, 4 significant bits per element where the FP4 formats keep 2, and the same GEMM kernels at the same rate.
The image goes to mul_nvfp4_native / mul_nvfp4_native_invariant / mul_nvfp4_native_moe / mul_nvfp4_native_moe_invariant with a global scale
of 1.0.  An MXFP6 checkpoint (OCP e2m3 bit stream + e8m0 scales) takes mxfp6_native_image instead: a copy into the same image, no rounding;
mxfp6_export is the way back (image -> OCP tensor, to save what quantize_mxfp6 produced) and dequant_native_image expands an image to 16 bit.
"""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "petit-kernel_amd"))
import petit_kernel  # noqa: E402


class Mxfp6Linear(torch.nn.Module):
    """y = RMSNorm(x) @ dequant(W)^T; W [n, k] (or experts [E, n, k] routed by expert_offsets over grouped rows) in MXFP6 on its native image."""

    def __init__(self, weight: torch.Tensor, norm_weight: torch.Tensor, fmt: str = "mxfp8", eps: float = 1e-6):
        super().__init__()
        self.fmt, self.eps = fmt, eps
        self.experts = weight.shape[0] if weight.dim() == 3 else 0
        self.size_n, self.size_k = weight.shape[-2:]
        self.register_buffer("norm_weight", norm_weight)
        self.register_buffer("image", petit_kernel.quantize_mxfp6(weight))          # one launch; E images back to back for a stacked tensor
        self.register_buffer("ones", torch.ones(max(self.experts, 1), dtype=torch.float32, device=weight.device))

    def forward(self, x: torch.Tensor, expert_offsets: torch.Tensor = None) -> torch.Tensor:
        q = petit_kernel.rmsnorm_quantize(x, self.norm_weight, self.eps, self.fmt)    # norm + quantiser: one launch
        if not self.experts and q.m <= 32:   # a decode step: the image as a weight stream (no global scale; its accumulation order moves with the shape)
            return petit_kernel.mul_nvfp4_native_decode(q, self.image, None, q.m, self.size_n, self.size_k, self.fmt)
        if not self.experts:
            return petit_kernel.mul_nvfp4_native_invariant(q, self.image, self.ones, q.m, self.size_n, self.size_k, self.fmt)
        return petit_kernel.mul_nvfp4_native_moe_invariant(q, self.image, self.ones, expert_offsets, q.m, self.size_n, self.size_k, self.experts,
                                                           fmt=self.fmt)


def main() -> None:
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    m, n, k, E = 64, 4096, 4096, 4
    norm_w = torch.ones(k, dtype=torch.bfloat16, device=dev)
    x = torch.randn(m, k, generator=g).bfloat16().to(dev)
    xn = torch.nn.functional.rms_norm(x.float(), (k,), norm_w.float(), 1e-6)

    def err(y, ref):
        return 100 * float((y.float() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())

    w = (torch.randn(n, k, generator=g) * 0.02).bfloat16().to(dev)
    ref = xn @ w.float().T
    layer = Mxfp6Linear(w, norm_w)
    print(f"MXFP6 weights, MXFP8 activations: rms error {err(layer(x), ref):4.1f} % of the bf16 layer's output rms")
    print(f"the same layer on 4 rows (mul_nvfp4_native_decode): rms error {err(layer(x[:4]), ref[:4]):4.1f} %")
    # save / reload: the image is instruction-shaped; mxfp6_export turns it into the OCP MXFP6 tensor any loader reads, and back without rounding
    elems, scales = petit_kernel.mxfp6_export(layer.image, n, k)
    state = {"weight.elems": elems.cpu(), "weight.scales": scales.cpu()}              # what a checkpoint would hold: 6.25 bits per weight
    reloaded = petit_kernel.mxfp6_native_image(state["weight.elems"].to(dev), state["weight.scales"].to(dev), n, k)
    w6 = petit_kernel.dequant_native_image(reloaded, n, k)                            # the weights the image holds, in bf16 (exact)
    print(f"export -> checkpoint -> image: same bytes: {torch.equal(reloaded, layer.image)}; "
          f"weight error {err(w6, w.float()):4.1f} % of the weight's rms")
    b, s, gs = petit_kernel.quantize_nvfp4(w)
    q = petit_kernel.rmsnorm_quantize(x, norm_w, 1e-6, "mxfp8")
    y4 = petit_kernel.mul_nvfp4_native_invariant(q, petit_kernel.nvfp4_native_image(b, s, n, k), gs, m, n, k, "mxfp8")
    print(f"NVFP4 image,   MXFP8 activations: rms error {err(y4, ref):4.1f} %")

    we = (torch.randn(E, 1024, k, generator=g) * 0.02).bfloat16().to(dev)
    offsets = torch.tensor([0, 20, 20, 48, m], dtype=torch.int32, device=dev)        # grouped rows per expert; expert 1 has none
    y = Mxfp6Linear(we, norm_w)(x, offsets)
    owner = torch.bucketize(torch.arange(m, device=dev), offsets[1:].long(), right=True)
    ref = torch.einsum("mk,mnk->mn", xn, we.float()[owner])
    print(f"{E} stacked MXFP6 experts, one MoE launch: rms error {err(y, ref):4.1f} %")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""examples/hadamard_mxfp4_linear.py -- MXFP4 activations with a block-Hadamard rotation (include/petit_amd.h "Block-Hadamard rotation"):
a dense layer as RMSNorm -> rotated MXFP4 activations -> the FP4 x FP4 block-scaled MFMA, on MXFP4 weights and on an NVFP4 image.
Needs an MI355X.

    python examples/hadamard_mxfp4_linear.py

Activations and weights are multiplied along K by the same +-1 Hadamard block, so x . W^T is unchanged while a block's outlier channels are
spread over all of its coefficients before the 4-bit rounding.  The weights are rotated ONCE at load time (quantize_*(w, hadamard=B) =
quantize_*(hadamard_rotate(w, B, -log2 B))); the activations are rotated inside the launch that quantises them (rmsnorm_quantize(...,
hadamard=B), or quantize_activations(x, "mxfp4", hadamard=B) for an input that does not come out of a norm): no extra launch, no 16-bit round
trip.  The GEMM is the unchanged native-class GEMM: it reads the quantised bytes and cannot tell that they were rotated.
A checkpoint whose weights were rotated offline with the orthonormal H / sqrt(B) runs the same way with global_scale / sqrt(B).
"""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "petit-kernel_amd"))
import petit_kernel  # noqa: E402


class HadamardFp4Linear(torch.nn.Module):
    """y = RMSNorm(x) @ dequant(W)^T * global_scale with MXFP4 activations; W [n, k] quantised to MXFP4 (kind "mx") or NVFP4 on its native
    image (kind "nv"), rotated with the block `hadamard` (0: the unrotated layer)."""

    def __init__(self, weight: torch.Tensor, norm_weight: torch.Tensor, kind: str = "mx", hadamard: int = 128, eps: float = 1e-6):
        super().__init__()
        self.kind, self.hadamard, self.eps = kind, hadamard, eps
        self.size_n, self.size_k = weight.shape
        self.register_buffer("norm_weight", norm_weight)
        if kind == "mx":
            b, s, gs = petit_kernel.quantize_mxfp4(weight, hadamard=hadamard)
            self.register_buffer("b", b)
            self.register_buffer("s", s)
        else:
            b, s, gs = petit_kernel.quantize_nvfp4(weight, hadamard=hadamard)
            self.register_buffer("image", petit_kernel.nvfp4_native_image(b, s, self.size_n, self.size_k))
        self.register_buffer("global_scale", gs)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x2 = x.reshape(-1, self.size_k).contiguous()
        q = petit_kernel.rmsnorm_quantize(x2, self.norm_weight, self.eps, "mxfp4", hadamard=self.hadamard)     # norm + rotation + quantiser: one launch
        sid = petit_kernel.SOLUTION_AUTO_NATIVE_MXFP4
        if self.kind == "mx":
            y = petit_kernel.mul_mxfp4_native(q, self.b, self.s, self.global_scale, q.m, self.size_n, self.size_k, sid)
        else:
            y = petit_kernel.mul_nvfp4_native(q, self.image, self.global_scale, q.m, self.size_n, self.size_k, sid)
        return y.reshape(*x.shape[:-1], self.size_n)


def main() -> None:
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    m, n, k = 64, 4096, 4096
    w = (torch.randn(n, k, generator=g) * 0.02).bfloat16().to(dev)
    norm_w = torch.ones(k, dtype=torch.bfloat16, device=dev)
    x = torch.randn(m, k, generator=g)
    x[:, 5::32] *= 20.0                                             # outlier channels, the shape LLM activations have
    x = x.bfloat16().to(dev)
    ref = torch.nn.functional.rms_norm(x.float(), (k,), norm_w.float(), 1e-6) @ w.float().T
    rms = ref.pow(2).mean().sqrt()
    for kind in ("mx", "nv"):
        for hadamard in (0, 32, 128):
            layer = HadamardFp4Linear(w, norm_w, kind, hadamard)
            err = (layer(x).float() - ref).pow(2).mean().sqrt() / rms
            name = "MXFP4 weights" if kind == "mx" else "NVFP4 image "
            print(f"{name}, MXFP4 activations, {'no rotation' if not hadamard else f'B = {hadamard:3d}   '}: rms error {100 * float(err):5.1f} % of the bf16 layer's output rms")


if __name__ == "__main__":
    main()

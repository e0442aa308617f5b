#!/usr/bin/env python3
"""examples/quantize_linear.py -- loading a bf16 checkpoint: quantise the 16-bit weights to packed NVFP4 / MXFP4 on the device and run them.
Needs an MI355X.

    python examples/quantize_linear.py

quantize_nvfp4 / quantize_mxfp4 return (b, s, global_scale) in the layout mul_*_a16 and the MoE layers read: there is no row-major FP4
tensor and no repack call in between.  A stack that receives fresh bf16 weights while it serves (an RL rollout engine) calls the same
function again: it makes no host sync and can be captured in a graph.
"""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "petit-kernel_amd"))
import petit_kernel  # noqa: E402


class QuantizedLinear(torch.nn.Module):
    """y = x @ W^T with W quantised at load time from its 16-bit form (fmt 'nvfp4' or 'mxfp4')."""

    def __init__(self, weight: torch.Tensor, fmt: str = "nvfp4"):
        super().__init__()
        self.size_n, self.size_k = weight.shape
        quantize = petit_kernel.quantize_nvfp4 if fmt == "nvfp4" else petit_kernel.quantize_mxfp4
        self.mul = petit_kernel.mul_nvfp4_a16 if fmt == "nvfp4" else petit_kernel.mul_mxfp4_a16
        b, s, gs = quantize(weight.contiguous())
        self.register_buffer("b", b)
        self.register_buffer("s", s)
        self.register_buffer("global_scale", gs)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x2 = x.reshape(-1, self.size_k)
        return self.mul(x2, self.b, self.s, self.global_scale, x2.shape[0], self.size_n, self.size_k, -1).reshape(*x.shape[:-1], self.size_n)


def main() -> None:
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    # a bf16 linear layer
    n, k = 4096, 4096
    weight = (torch.randn((n, k), generator=g) / k ** 0.5).bfloat16().to(dev)
    x = torch.randn((7, k), generator=g).bfloat16().to(dev)
    ref = x.float() @ weight.float().T
    for fmt in ("nvfp4", "mxfp4"):
        y = QuantizedLinear(weight, fmt)(x).float()
        err = ((y - ref).norm() / ref.norm()).item()
        print(f"{fmt} linear {n} x {k}: output error {err:.3f} of the bf16 layer's output rms (FP4 weights: about 0.1)")
        assert err < 0.2

    # a stacked-expert layer: [E, 2 I, H] gate_up and [E, H, I] down, every expert quantised on its own (one global scale each)
    E, H, I, T, topk = 8, 1024, 512, 16, 2
    w13 = (torch.randn((E, 2 * I, H), generator=g) / H ** 0.5).bfloat16().to(dev)
    w2 = (torch.randn((E, H, I), generator=g) / I ** 0.5).bfloat16().to(dev)
    hidden = torch.randn((T, H), generator=g).bfloat16().to(dev)
    topk_weights, topk_ids = torch.softmax(torch.randn((T, E), generator=g), -1).topk(topk)
    out = petit_kernel.fp4_moe_fused(hidden, *petit_kernel.quantize_nvfp4(w13), *petit_kernel.quantize_nvfp4(w2),
                                     topk_weights.to(dev), topk_ids.to(dev), "nvfp4")
    ref = torch.zeros((T, H))
    for t in range(T):
        for j in range(topk):
            e = int(topk_ids[t, j])
            y = hidden[t].float().cpu() @ w13[e].float().cpu().T
            ref[t] += topk_weights[t, j] * ((torch.nn.functional.silu(y[:I]) * y[I:]) @ w2[e].float().cpu().T)
    err = ((out.float().cpu() - ref).norm() / ref.norm()).item()
    print(f"nvfp4 MoE layer E = {E}, H = {H}, I = {I}: output error {err:.3f} of the bf16 layer's output rms")
    assert err < 0.3


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""examples/nvfp4_native_invariant.py -- NVFP4 weights on the native class with batch invariance (include/petit_amd.h "Batch-invariant
native-class GEMM and MoE launch on NVFP4 images"): a dense linear, and a routed-expert (MoE) layer composed from its launches, whose every
token gets the same bits alone, inside a batch, and at any position of it.  Needs an MI355X.

    python examples/nvfp4_native_invariant.py

The weights are re-encoded ONCE into their MFMA-native image (nvfp4_native_image / nvfp4_native_images: FP6 e2m3 elements, one E8M0 scale per
32 k); the activations are quantised per row (and per 32-k block), and the GEMM's K order is a function of the shape alone: nothing in either
chain looks at the batch.  The native defaults (mul_nvfp4_native, fp4_moe_native) are faster and pick their kernels by the batch size, so
the same token MAY come out with different bits alone and in a batch.  The price is in profiles/nvfp4_native_invariant.md.
"""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "petit-kernel_amd"))
import petit_kernel  # noqa: E402


class NvFp4InvariantLinear(torch.nn.Module):
    """y = x @ dequant(W)^T * global_scale (+ bias); W [n, k] quantised to NVFP4 and kept as its native image."""

    def __init__(self, weight: torch.Tensor, bias=None, fmt="mxfp8"):
        super().__init__()
        self.fmt, self.bias = fmt, bias
        self.size_n, self.size_k = weight.shape
        b, s, gs = petit_kernel.quantize_nvfp4(weight)
        self.register_buffer("image", petit_kernel.nvfp4_native_image(b, s, self.size_n, self.size_k))
        self.register_buffer("global_scale", gs)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x2 = x.reshape(-1, self.size_k).contiguous()
        y = petit_kernel.mul_nvfp4_native_invariant(x2, self.image, self.global_scale, x2.shape[0], self.size_n, self.size_k, self.fmt,
                                                    bias=self.bias)
        return y.reshape(*x.shape[:-1], self.size_n)


class NvFp4InvariantMoE(torch.nn.Module):
    """A routed-expert layer (SiLU-gated MLP per expert) on NVFP4 experts: align, the gathering quantiser, the two batch-invariant launches on
    the experts' images (gate_up on the quantised grouped rows, down scattered into slot order), the top-k combine -- what
    fp4_moe_native(invariant=True) composes for MXFP4 experts."""

    def __init__(self, w13: torch.Tensor, w2: torch.Tensor, fmt="mxfp8"):
        super().__init__()
        self.fmt = fmt
        self.E, n13, self.H = w13.shape
        self.I = n13 // 2
        for name, w, n, k in (("13", w13, n13, self.H), ("2", w2, self.H, self.I)):
            b, s, gs = petit_kernel.quantize_nvfp4(w)
            self.register_buffer("images" + name, petit_kernel.nvfp4_native_images(b, s, self.E, n, k))
            self.register_buffer("gs" + name, gs)

    def forward(self, hidden: torch.Tensor, topk_weights: torch.Tensor, topk_ids: torch.Tensor) -> torch.Tensor:
        m = hidden.shape[0] * topk_ids.shape[1]
        sorted_pos, offsets, token_index = petit_kernel.moe_align_device(topk_ids, self.E)
        qa = petit_kernel.quantize_activation_rows(hidden, self.fmt, token_index)             # the m grouped rows
        h = petit_kernel.mul_nvfp4_native_moe_invariant(qa, self.images13, self.gs13, offsets, m, 2 * self.I, self.H, self.E, fmt=self.fmt,
                                                        activation="silu_mul")               # [m, I]
        y = petit_kernel.mul_nvfp4_native_moe_invariant(h, self.images2, self.gs2, offsets, m, self.H, self.I, self.E, c_row_index=sorted_pos,
                                                        c_rows=m, fmt=self.fmt)              # [m, H], (token, slot) order
        return petit_kernel.moe_combine(y, topk_weights, topk_ids, self.E)


def main() -> None:
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    n, k = 4096, 4096
    dense = NvFp4InvariantLinear((torch.randn(n, k, generator=g) * 0.05).bfloat16().to(dev), torch.randn(n, generator=g).bfloat16().to(dev))
    print(f"S, L = {petit_kernel.invariant_geometry(n, k, torch.bfloat16, 'nvfp4')} for n = {n}, k = {k}")
    for rows in (8, 64, 512):
        batch = torch.randn((rows, k), generator=g).bfloat16().to(dev)
        full = dense(batch).view(torch.int16)
        equal = sum(torch.equal(dense(batch[r:r + 1]).view(torch.int16)[0], full[r]) for r in range(rows))
        form = "split" if petit_kernel.native_invariant_workspace_bytes(rows, n, k, torch.bfloat16, dense.fmt, True) else "whole"
        print(f"dense, batch of {rows:3d} ({form} form): {equal} of {rows} rows equal, bit for bit, the row projected alone")

    E, H, I, topk = 8, 1024, 512, 2
    moe = NvFp4InvariantMoE((torch.randn(E, 2 * I, H, generator=g) * 0.05).bfloat16().to(dev),
                            (torch.randn(E, H, I, generator=g) * 0.05).bfloat16().to(dev))
    for tokens in (4, 64, 300):
        hidden = torch.randn((tokens, H), generator=g).bfloat16().to(dev)
        w, ids = torch.topk(torch.softmax(torch.randn(tokens, E, generator=g), dim=1), topk, dim=1)
        w, ids = w.contiguous().to(dev), ids.to(torch.int32).contiguous().to(dev)
        full = moe(hidden, w, ids).view(torch.int16)
        equal = sum(torch.equal(moe(hidden[t:t + 1], w[t:t + 1], ids[t:t + 1]).view(torch.int16)[0], full[t]) for t in range(tokens))
        form = "split" if petit_kernel.native_moe_invariant_form(tokens * topk, E) else "whole"
        print(f"routed, batch of {tokens:3d} tokens ({form} form): {equal} of {tokens} tokens equal, bit for bit, the token routed alone")


if __name__ == "__main__":
    main()

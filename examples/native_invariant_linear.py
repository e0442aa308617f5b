#!/usr/bin/env python3
"""examples/native_invariant_linear.py -- RMSNorm -> MXFP4 linear on the native class with batch invariance: rmsnorm_quantize writes the
quantised activations ("petit-qact/1") and mul_mxfp4_native_invariant consumes them (include/petit_amd.h "Batch-invariant GEMM on the native
class"), so a token gets the same bits normed and projected alone, inside a prefill batch, and at any position of it.  Needs an MI355X.

    python examples/native_invariant_linear.py

The norm and the quantiser work per row (and per 32-k block), the GEMM's K order is a function of the shape alone: nothing in the chain looks
at the batch.  The native default (mul_mxfp4_native with a sentinel) is faster and picks its kernel, its K split and a bulk / tail row split by
the batch size, so the same row MAY come out with different bits alone and in a batch.  The price is in profiles/native_invariant.md.
"""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "petit-kernel_amd"))
import petit_kernel  # noqa: E402


class NormedMxFp4Linear(torch.nn.Module):
    """y = RMSNorm(x) @ dequant(W)^T (+ bias); W in MXFP4, the normed activations quantised to `fmt` by the norm's own launch."""

    def __init__(self, qweight: torch.Tensor, weight_scale: torch.Tensor, norm_weight: torch.Tensor, bias=None, fmt="mxfp8", eps=1e-6):
        super().__init__()
        self.fmt, self.eps, self.bias = fmt, eps, bias
        self.size_n, self.size_k = qweight.shape[0], qweight.shape[1] * 2
        self.register_buffer("b", petit_kernel.repack_mxfp4(qweight.view(torch.int32), size_n=self.size_n, size_k=self.size_k))
        self.register_buffer("s", petit_kernel.process_mxfp4_scales(scales=weight_scale, size_n=self.size_n, size_k=self.size_k))
        self.register_buffer("norm_weight", norm_weight)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x2 = x.reshape(-1, self.size_k)
        qa = petit_kernel.rmsnorm_quantize(x2, self.norm_weight, self.eps, self.fmt)
        y = petit_kernel.mul_mxfp4_native_invariant(qa, self.b, self.s, None, x2.shape[0], self.size_n, self.size_k, self.fmt, bias=self.bias)
        return y.reshape(*x.shape[:-1], self.size_n)


def main() -> None:
    dev = torch.device("cuda")
    n, k = 4096, 4096
    g = torch.Generator().manual_seed(0)
    q = torch.randint(0, 256, (n, k // 2), generator=g, dtype=torch.uint8).to(dev)
    ws = torch.randint(119, 136, (n, k // 32), generator=g, dtype=torch.uint8).to(dev)
    norm_w, bias = (1.0 + 0.1 * torch.randn(k, generator=g)).bfloat16().to(dev), torch.randn(n, generator=g).bfloat16().to(dev)
    print(f"S, L = {petit_kernel.invariant_geometry(n, k, torch.bfloat16, 'mxfp4')} for n = {n}, k = {k}")
    for fmt in ("mxfp8", "mxfp6", "mxfp4"):
        layer = NormedMxFp4Linear(q, ws, norm_w, bias, fmt)
        for rows in (8, 64, 512):
            batch = torch.randn((rows, k), generator=g).bfloat16().to(dev)
            full = layer(batch).view(torch.int16)
            equal = sum(torch.equal(layer(batch[r:r + 1]).view(torch.int16)[0], full[r]) for r in range(rows))
            form = "split" if petit_kernel.native_invariant_workspace_bytes(rows, n, k, torch.bfloat16, fmt, True) else "whole"
            print(f"{fmt}, batch of {rows:3d} ({form} form): {equal} of {rows} rows equal, bit for bit, the row normed and projected alone")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""examples/batch_invariant_linear.py -- an NVFP4 linear layer with the batch-invariance switch on: every output row is a pure function of
its own input row (include/petit_amd.h "Batch-invariant GEMM"), so a token gets the same bits decoded alone, inside a prefill batch, and at
any position of it -- what reproducible inference and RL rollouts that must match training forwards ask for.  Needs an MI355X.

    python examples/batch_invariant_linear.py

The default path (mul_nvfp4_a16, solution_id = -1) is pinned bit for bit within one call only: the kernel it picks moves with the batch size,
so the same row MAY come out with different bits alone and in a batch.  The invariant path costs speed (profiles/gemm_invariant.md).
"""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "petit-kernel_amd"))
import petit_kernel  # noqa: E402


class PetitNvFp4Linear(torch.nn.Module):
    """y = x @ dequant(W)^T * weight_scale_2 (+ bias); W in NVFP4.  batch_invariant=True: a row's result does not depend on its batch."""

    def __init__(self, qweight: torch.Tensor, weight_scale: torch.Tensor, weight_scale_2: torch.Tensor, bias=None, batch_invariant=False):
        super().__init__()
        self.batch_invariant = batch_invariant
        self.size_n, self.size_k = qweight.shape[0], qweight.shape[1] * 2
        self.register_buffer("b", petit_kernel.repack_nvfp4(qweight.view(torch.int32), size_n=self.size_n, size_k=self.size_k))
        self.register_buffer("s", petit_kernel.process_nvfp4_scales(scales=weight_scale, size_n=self.size_n, size_k=self.size_k))
        self.register_buffer("global_scale", weight_scale_2.reshape(1).float())
        self.bias = bias

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x2 = x.reshape(-1, self.size_k)
        if self.batch_invariant:
            y = petit_kernel.mul_nvfp4_a16_invariant(x2, self.b, self.s, self.global_scale, x2.shape[0], self.size_n, self.size_k, bias=self.bias)
        else:
            y = petit_kernel.mul_nvfp4_a16(x2, self.b, self.s, self.global_scale, x2.shape[0], self.size_n, self.size_k, -1, bias=self.bias)
        return y.reshape(*x.shape[:-1], self.size_n)


def differing_rows(layer, batch: torch.Tensor) -> int:
    """Rows of layer(batch) whose bits differ from the same row run alone."""
    full = layer(batch).view(torch.int16)
    return sum(not torch.equal(layer(batch[r:r + 1]).view(torch.int16)[0], full[r]) for r in range(batch.shape[0]))


def main() -> None:
    dev = torch.device("cuda")
    n, k = 4096, 4096
    g = torch.Generator().manual_seed(0)
    q = torch.randint(0, 256, (n, k // 2), generator=g, dtype=torch.uint8).to(dev)
    ws = (torch.rand((n, k // 16), generator=g) * 3.5 + 0.25).to(torch.float8_e4m3fn).to(dev)
    ws2, bias = torch.tensor(0.01).to(dev), torch.randn(n, generator=g).bfloat16().to(dev)
    invariant = PetitNvFp4Linear(q, ws, ws2, bias, batch_invariant=True)
    default = PetitNvFp4Linear(q, ws, ws2, bias)
    print(f"S, L = {petit_kernel.invariant_geometry(n, k)} for n = {n}, k = {k}")
    for rows in (8, 64, 512):
        batch = torch.randn((rows, k), generator=g).bfloat16().to(dev)
        bad = differing_rows(invariant, batch)
        print(f"batch of {rows:3d}, batch-invariant path: {rows - bad} of {rows} rows agree bit for bit with the row run alone")
        assert bad == 0
        shuffled = batch.flip(0)
        assert torch.equal(invariant(shuffled).flip(0).view(torch.int16), invariant(batch).view(torch.int16))
        bad = differing_rows(default, batch)
        print(f"batch of {rows:3d}, default path:         {rows - bad} of {rows} rows agree (it does not have to: the pick moves with the batch)")
        close = (invariant(batch).float() - default(batch).float()).abs().max().item()
        print(f"               the two paths differ by at most {close:.3g} (rounding order only)")


if __name__ == "__main__":
    main()

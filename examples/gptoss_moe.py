#!/usr/bin/env python3
"""examples/gptoss_moe.py -- the routed experts of a gpt-oss MoE block on the MoE layers.

A synthetic checkpoint in gpt-oss's own layout (MXFP4 blocks uint8 [E, rows, K/32, 16] + E8M0 scales, gate / up rows interleaved in
gate_up_proj, a bias on gate_up and on down, hidden = intermediate = 2880), then

    experts = petit_kernel.prepare_gptoss_experts(...)      # load time: de-interleave, pad 2880 -> 3072, repack
    out = experts.forward(x, topk_weights, topk_ids, path="fused" | "native")
    out = experts.forward(x, topk_weights, topk_ids, path="native", invariant=True)   # batch-invariant: the same bits for a token in any batch

and the maximum error of both paths against a float64 statement of the block (dequantised weights, clamped SwiGLU, router weights on
down + bias).  The router (top-k, then softmax over the k) is plain torch for the reference; `experts.forward_routed(x, logits)` does it on
the device, in the align's launch.

    python examples/gptoss_moe.py [--experts 8] [--tokens 16] [--hidden 2880]
"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "petit-kernel_amd"))

import petit_kernel  # noqa: E402

E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0], dtype=torch.float64)


def dequant(blocks, scales):
    """uint8 [rows, K/32, 16] + E8M0 uint8 [rows, K/32] -> float64 [rows, K]; the lower-k element is the low nibble"""
    lo, hi = E2M1[(blocks & 15).long()], E2M1[(blocks >> 4).long()]
    vals = torch.stack([lo, hi], dim=-1).reshape(blocks.shape[0], blocks.shape[1], 32)
    return (vals * torch.exp2(scales.double() - 127)[..., None]).reshape(blocks.shape[0], -1)


def reference(ck, x, tw, ids):
    out = torch.zeros(x.shape[0], ck["down_blocks"].shape[1], dtype=torch.float64)
    xf = x.double()
    for e in ids.unique().tolist():
        tok, slot = (ids == e).nonzero(as_tuple=True)
        y1 = xf[tok] @ dequant(ck["gate_up_blocks"][e], ck["gate_up_scales"][e]).T + ck["gate_up_bias"][e].double()
        g, u = y1[:, 0::2].clamp(max=7.0), y1[:, 1::2].clamp(-7.0, 7.0)          # interleaved: gate = 0::2, up = 1::2
        h = g * torch.sigmoid(1.702 * g) * (u + 1)
        y2 = h @ dequant(ck["down_blocks"][e], ck["down_scales"][e]).T + ck["down_bias"][e].double()
        out.index_add_(0, tok, y2 * tw[tok, slot].double()[:, None])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--experts", type=int, default=8)
    ap.add_argument("--tokens", type=int, default=16)
    ap.add_argument("--hidden", type=int, default=2880)
    ap.add_argument("--topk", type=int, default=4)
    a = ap.parse_args()
    E, T, H, topk = a.experts, a.tokens, a.hidden, a.topk
    g = torch.Generator().manual_seed(0)
    u8 = lambda *shape, lo=0, hi=256: torch.randint(lo, hi, shape, dtype=torch.uint8, generator=g)  # noqa: E731
    ck = dict(gate_up_blocks=u8(E, 2 * H, H // 32, 16), gate_up_scales=u8(E, 2 * H, H // 32, lo=122, hi=128),
              gate_up_bias=(torch.randn(E, 2 * H, generator=g) * 0.5).bfloat16(),
              down_blocks=u8(E, H, H // 32, 16), down_scales=u8(E, H, H // 32, lo=122, hi=128),
              down_bias=(torch.randn(E, H, generator=g) * 0.5).bfloat16())
    experts = petit_kernel.prepare_gptoss_experts(**{k: v.cuda() for k, v in ck.items()})
    print(f"{E} experts, hidden = intermediate = {experts.hidden} -> padded to {experts.hidden_padded}; "
          f"w13 {tuple(experts.w13.shape)}, w2 {tuple(experts.w2.shape)}, bias13 {tuple(experts.bias13.shape)}")
    x = (torch.randn(T, H, generator=g) * (3.0 / (0.9 * H ** 0.5))).bfloat16()
    logits = torch.randn(T, E, generator=g)
    top, ids = torch.topk(logits, topk, dim=-1)
    tw = torch.softmax(top, dim=-1)                                                  # gpt-oss: softmax over the selected k
    ref = reference(ck, x, tw, ids)
    for path in ("fused", "native"):
        out = experts.forward(x.cuda(), tw.cuda(), ids.int().cuda(), path=path)
        torch.cuda.synchronize()
        err = (out.double().cpu() - ref).abs()
        print(f"{path:6s}: out {tuple(out.shape)} {out.dtype}, max |err| {err.max().item():.4g} (output rms {ref.pow(2).mean().sqrt().item():.4g}, "
              f"rms err / rms {(err.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item():.3e})")
        routed = experts.forward_routed(x.cuda(), logits.cuda(), topk=topk, path=path)   # from the logits: route + align in one launch
        print(f"{path:6s}: forward_routed max |difference to forward| {(routed.float() - out.float()).abs().max().item():.4g}")
        # from the hidden state: the router's linear (weight [E, hidden], float32 bias) as the library's router GEMM on the unpadded x
        router_w = (torch.randn(experts.num_experts, x.size(1)) / x.size(1) ** 0.5).bfloat16().cuda()
        router_b = torch.randn(experts.num_experts).cuda()
        hidden = experts.forward_hidden(x.cuda(), router_w, router_b, topk=topk, path=path)
        same = experts.forward_routed(x.cuda(), petit_kernel.moe_router_logits(x.cuda(), router_w, router_b), topk=topk, path=path)
        print(f"{path:6s}: forward_hidden equals forward_routed on moe_router_logits: {torch.equal(hidden.view(torch.int16), same.view(torch.int16))}")

        # batch-invariant: a token's output row has the same bits alone and inside the batch (fp4_moe_native / fp4_moe_fused, invariant=True)
        inv = experts.forward(x.cuda(), tw.cuda(), ids.int().cuda(), path=path, invariant=True)
        one = experts.forward(x[3:4].cuda(), tw[3:4].cuda(), ids[3:4].int().cuda(), path=path, invariant=True)
        err = (inv.double().cpu() - ref).abs()
        print(f"{path:6s}: forward(..., path={path!r}, invariant=True): token 3 alone == token 3 in the batch: "
              f"{torch.equal(one[0].view(torch.int16), inv[3].view(torch.int16))}, max |err| {err.max().item():.4g}")


if __name__ == "__main__":
    main()

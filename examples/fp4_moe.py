#!/usr/bin/env python3
"""examples/fp4_moe.py -- an NVFP4 mixture-of-experts layer (E = 8 experts, top-2) the way a serving stack runs it: the experts' weights
stacked and packed once at load time, then one `fp4_moe` call per forward (two MoE launches: gate_up with fused SiLU-mul, down).
Checks against the same layer in torch on the dequantised weights.  Needs an MI355X.

    python examples/fp4_moe.py
"""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "petit-kernel_amd"))
import petit_kernel  # noqa: E402


def random_nvfp4(rows, cols, g):
    q = torch.randint(0, 256, (rows, cols // 2), dtype=torch.uint8, generator=g)
    s = (torch.rand(rows, cols // 16, generator=g) * 3.5 + 0.25).to(torch.float8_e4m3fn)
    return q, s


def main():
    dev = "cuda"
    E, topk, H, I, T = 8, 2, 1024, 512, 32
    g = torch.Generator().manual_seed(0)
    q13, s13 = random_nvfp4(E * 2 * I, H, g)          # [gate; up] of every expert, stacked along N
    q2, s2 = random_nvfp4(E * H, I, g)
    gs13, gs2 = torch.full((E,), 0.05), torch.full((E,), 0.05)
    # load time: one repack of each stacked tensor
    w13 = petit_kernel.repack_nvfp4(q13.to(dev).view(torch.int32), E * 2 * I, H)
    p13 = petit_kernel.process_nvfp4_scales(s13.to(dev), E * 2 * I, H)
    w2 = petit_kernel.repack_nvfp4(q2.to(dev).view(torch.int32), E * H, I)
    p2 = petit_kernel.process_nvfp4_scales(s2.to(dev), E * H, I)
    # forward
    x = torch.randn(T, H, generator=g).to(torch.bfloat16)
    topk_w, topk_ids = torch.topk(torch.softmax(torch.randn(T, E, generator=g), -1), topk, dim=-1)
    out = petit_kernel.fp4_moe(x.to(dev), w13, p13, gs13.to(dev), w2, p2, gs2.to(dev), topk_w.to(dev), topk_ids.to(torch.int32).to(dev), "nvfp4")
    # the same layer in torch on the dequantised weights
    d13 = petit_kernel.ops.dequant_packed(w13, p13, E * 2 * I, H, "nvfp4").cpu().view(E, 2 * I, H) * 0.05
    d2 = petit_kernel.ops.dequant_packed(w2, p2, E * H, I, "nvfp4").cpu().view(E, H, I) * 0.05
    ref = torch.zeros(T, H, dtype=torch.float64)
    xf = x.double()
    for t in range(T):
        for j in range(topk):
            e = int(topk_ids[t, j])
            y = d13[e].double() @ xf[t]
            h = torch.nn.functional.silu(y[:I]) * y[I:]
            ref[t] += topk_w[t, j].double() * (d2[e].double() @ h)
    err = (out.double().cpu() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()
    print(f"fp4_moe: T={T} E={E} top-{topk} H={H} I={I}: rms error / rms = {err:.2e}")
    assert err < 1e-2
    # the fused layer: device align, gate_up on gathered rows, down scattered into slot order, top-k combine (4 launches)
    fused = petit_kernel.fp4_moe_fused(x.to(dev), w13, p13, gs13.to(dev), w2, p2, gs2.to(dev), topk_w.to(dev), topk_ids.to(dev), "nvfp4")
    err_f = (fused.double().cpu() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()
    print(f"fp4_moe_fused: rms error / rms = {err_f:.2e}")
    assert err_f < 1e-2
    # from the router's logits: the routing (softmax, top-k, renormalise; the lower index among equal logits) and the align in one launch
    logits = torch.randn(T, E, generator=g).to(torch.bfloat16).to(dev)
    rw, rids = petit_kernel.moe_route(logits, topk, scoring="softmax", renormalize=True)
    routed = petit_kernel.fp4_moe_routed(x.to(dev), logits, w13, p13, gs13.to(dev), w2, p2, gs2.to(dev), topk, "nvfp4", scoring="softmax",
                                         renormalize=True)
    same = petit_kernel.fp4_moe_fused(x.to(dev), w13, p13, gs13.to(dev), w2, p2, gs2.to(dev), rw, rids, "nvfp4")
    assert torch.equal(routed.view(torch.int16), same.view(torch.int16))
    print(f"fp4_moe_routed: equals fp4_moe_fused on moe_route's ids {tuple(rids.shape)} and weights bit for bit")
    # one step earlier, from the hidden state: the router's linear as the library's router GEMM (fp32 accumulation in an order the shape
    # alone fixes, so a token's experts do not depend on its batch), then route + align on its partial sums -- two launches
    router_w = (torch.randn(E, H, generator=g) / H ** 0.5).to(torch.bfloat16).to(dev)
    from_hidden = petit_kernel.fp4_moe_routed(x.to(dev), None, w13, p13, gs13.to(dev), w2, p2, gs2.to(dev), topk, "nvfp4", scoring="softmax",
                                              renormalize=True, router_weight=router_w)
    own_logits = petit_kernel.moe_router_logits(x.to(dev), router_w)
    from_logits = petit_kernel.fp4_moe_routed(x.to(dev), own_logits, w13, p13, gs13.to(dev), w2, p2, gs2.to(dev), topk, "nvfp4", scoring="softmax",
                                              renormalize=True)
    assert torch.equal(from_hidden.view(torch.int16), from_logits.view(torch.int16))
    print(f"fp4_moe_routed(router_weight=...): equals the layer on moe_router_logits {tuple(own_logits.shape)} bit for bit")
    # batch-invariant: with invariant=True gate_up and down run as the batch-invariant MoE launches, so from the hidden state a token's output
    # row is a pure function of its hidden row and the weights -- the same bits alone and inside the batch (opt-in: slower than the default
    # pick, profiles/moe_invariant.md).  The default layer makes no such promise: its kernels are picked by the batch's size.
    inv = dict(scoring="softmax", renormalize=True, router_weight=router_w)
    args = (w13, p13, gs13.to(dev), w2, p2, gs2.to(dev), topk, "nvfp4")
    batch_inv = petit_kernel.fp4_moe_routed(x.to(dev), None, *args, invariant=True, **inv)
    batch_def = petit_kernel.fp4_moe_routed(x.to(dev), None, *args, **inv)
    equal_inv = equal_def = True
    for t in (0, T // 2, T - 1):
        one = x[t:t + 1].to(dev)
        alone_inv = petit_kernel.fp4_moe_routed(one, None, *args, invariant=True, **inv)
        alone_def = petit_kernel.fp4_moe_routed(one, None, *args, **inv)
        equal_inv &= torch.equal(alone_inv[0].view(torch.int16), batch_inv[t].view(torch.int16))
        equal_def &= torch.equal(alone_def[0].view(torch.int16), batch_def[t].view(torch.int16))
    print(f"fp4_moe_routed(invariant=True): a token's row alone equals its row in the batch of {T}: {equal_inv} (default layer: {equal_def})")
    assert equal_inv
    # the fused end: the layer's last launch also adds the residual stream, applies the NEXT block's RMSNorm and quantises its input for a
    # native-class GEMM -- bit for bit the layer followed by rmsnorm_quantize, one launch and one [T, H] round trip less.  (For a layer whose
    # combine is complete on this rank: with tensor or expert parallelism the all-reduce comes between the combine and the residual add.)
    resid = torch.randn(T, H, generator=g).to(torch.bfloat16).to(dev)
    norm_w = (1.0 + 0.1 * torch.randn(H, generator=g)).to(torch.bfloat16).to(dev)
    q, h_next = petit_kernel.fp4_moe_routed(x.to(dev), logits, w13, p13, gs13.to(dev), w2, p2, gs2.to(dev), topk, "nvfp4", scoring="softmax",
                                            renormalize=True, norm_weight=norm_w, norm_eps=1e-6, norm_residual=resid, norm_fmt="mxfp8")
    q_ref, h_ref = petit_kernel.rmsnorm_quantize(routed, norm_w, 1e-6, "mxfp8", residual=resid)
    assert torch.equal(q.data, q_ref.data) and torch.equal(h_next.view(torch.int16), h_ref.view(torch.int16))
    print(f"fp4_moe_routed(norm_weight=...): {q} and the new residual stream, equal to the layer + rmsnorm_quantize bit for bit")
    # DeepSeek-style: sigmoid scoring with groups, and one always-on shared expert of the routed experts' size as expert E of the stacks
    # ("shared-experts fusion"): every token gets slot topk with id E and weight 1, written by the same route + align launch
    qs13, ss13 = random_nvfp4(2 * I, H, g)
    qs2, ss2 = random_nvfp4(H, I, g)
    EA = E + 1
    w13a = petit_kernel.repack_nvfp4(torch.cat([q13, qs13]).to(dev).view(torch.int32), EA * 2 * I, H)
    p13a = petit_kernel.process_nvfp4_scales(torch.cat([s13.view(torch.uint8), ss13.view(torch.uint8)]).view(torch.float8_e4m3fn).to(dev), EA * 2 * I, H)
    w2a = petit_kernel.repack_nvfp4(torch.cat([q2, qs2]).to(dev).view(torch.int32), EA * H, I)
    p2a = petit_kernel.process_nvfp4_scales(torch.cat([s2.view(torch.uint8), ss2.view(torch.uint8)]).view(torch.float8_e4m3fn).to(dev), EA * H, I)
    gsa = torch.full((EA,), 0.05, device=dev)
    deepseek = dict(scoring="sigmoid", renormalize=True, n_group=4, topk_group=2, routed_scaling_factor=2.5,
                    bias=torch.randn(E, generator=g).to(dev) * 0.1)
    with_shared = petit_kernel.fp4_moe_routed(x.to(dev), logits, w13a, p13a, gsa, w2a, p2a, gsa, topk, "nvfp4", num_shared=1, **deepseek)
    sw, sids = petit_kernel.moe_route(logits, topk, num_shared=1, **deepseek)
    assert sids.shape == (T, topk + 1) and (sids[:, topk] == E).all() and (sw[:, topk] == 1.0).all()
    # the same thing the long way: the routed layer on the E routed experts, the shared expert as two dense calls, an add
    routed_only = petit_kernel.fp4_moe_routed(x.to(dev), logits, w13, p13, gs13.to(dev), w2, p2, gs2.to(dev), topk, "nvfp4", **deepseek)
    ws13 = petit_kernel.repack_nvfp4(qs13.to(dev).view(torch.int32), 2 * I, H)
    ps13 = petit_kernel.process_nvfp4_scales(ss13.to(dev), 2 * I, H)
    ws2 = petit_kernel.repack_nvfp4(qs2.to(dev).view(torch.int32), H, I)
    ps2 = petit_kernel.process_nvfp4_scales(ss2.to(dev), H, I)
    hs = petit_kernel.mul_nvfp4_a16(x.to(dev), ws13, ps13, gsa[:1], T, 2 * I, H, -1, activation="silu_mul")
    long_way = routed_only.float() + petit_kernel.mul_nvfp4_a16(hs, ws2, ps2, gsa[:1], T, H, I, -1).float()
    err_s = (with_shared.float() - long_way).pow(2).mean().sqrt() / long_way.pow(2).mean().sqrt()
    print(f"fp4_moe_routed(num_shared=1): {topk + 1} slots per token, rms difference to routed layer + dense shared expert = {err_s:.2e}")
    assert err_s < 1e-2
    # the native class (block-scaled MFMA, activations quantised to MXFP8: another accuracy class, for prefill) on the same packed tensors,
    # without resident images: each launch builds the images of the experts this routing uses into its scratch.  Bit for bit the layer on
    # images built once at load time, which would hold 6.25 more bits per weight
    ids_dev = topk_ids.to(torch.int32).to(dev)
    transient = petit_kernel.fp4_moe_native(x.to(dev), w13, p13, gs13.to(dev), w2, p2, gs2.to(dev), topk_w.to(dev), ids_dev, kind="nvfp4",
                                            activations="mxfp8", transient=True)
    i13 = petit_kernel.nvfp4_native_images(w13, p13, E, 2 * I, H)
    i2 = petit_kernel.nvfp4_native_images(w2, p2, E, H, I)
    resident = petit_kernel.fp4_moe_native(x.to(dev), i13, None, gs13.to(dev), i2, None, gs2.to(dev), topk_w.to(dev), ids_dev, kind="nvfp4",
                                           activations="mxfp8")
    assert torch.equal(transient.view(torch.int16), resident.view(torch.int16))
    err_n = (transient.double().cpu() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()
    print(f"fp4_moe_native(transient=True): equals the resident-image layer bit for bit; rms error / rms = {err_n:.2e} (native class)")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""tools/moe_bench.py -- the routed-expert (MoE) launch against a host loop of dense calls, on real expert shapes.

    python tools/moe_bench.py [--cells decode|prefill|all] [--models deepseek,qwen3,mixtral] [--iters N] [--out FILE]
                              [--only-moe | --only-loop] [--single-expert] [--layer [--native mxfp8|mxfp6|mxfp4 | --from-logits | --shared]]
                              [--gptoss]

Per cell (model, projection, T tokens): E experts' NVFP4 weights (bf16 activations) stacked back to back, copied until the pool is >= 1 GB so
that rotating over copies and over routings (drawn from a seed, top-k of random router logits) keeps the 256 MB Infinity Cache from serving
the weights.  Timed with HIP events over `--iters` iterations (eager launches):
  moe_us   one petit_gemm_fp4_fp16_moe launch (solution_id = -1)
  loop_us  the per-active-expert loop of dense mul_nvfp4_a16 calls (solution_id = -1 for each expert's row count); the benchmark knows its own
           routing, so the loop needs no device -> host copy (a real caller's would)
  active_bytes  weight + scale bytes of the experts that have rows (+ activations and outputs), the bytes the MoE launch has to move
--single-expert: every row routed to one expert, the MoE launch against the dense call with the SAME id (the indirection cost), at M = 1, 16, 512.
--layer: the whole routed-expert layer (gate_up with SiLU-mul, down, top-k combine; DeepSeek-V3 / Qwen3-30B-A3B / Mixtral shapes), fp4_moe
against fp4_moe_fused, each captured once in a torch.cuda.graph (one capture stream, no parallel branches) and replayed; per cell also the
plain MoE GEMMs on pre-gathered rows against the indexed ones (gate_up gathering A, down scattering C), ten launches per captured graph.
--layer --native mxfp8|mxfp6|mxfp4: fp4_moe_native against fp4_moe_fused on the same weights (MXFP4 raw; NVFP4 through nvfp4_native_images), graph
replays, T = 1, 16, 64, 1024, 4096; plus one single-expert cell (M = 4096, every row on one expert, activations pre-quantised: the native MoE launch
against the dense native call with the same id).
--layer --from-logits: the layer from the router's logits, graph replays on one stream, two columns: (a) the model's torch routing chain
(softmax + top-k + renormalise; gpt-oss: top-k, softmax over the k; DeepSeek-V3: the grouped top-k chain written out in torch_routing) followed
by fp4_moe_fused, and (b) fp4_moe_routed.  Measured a, b, a, b in one process, both pairs reported; per cell also the number of kernels the
routing chain of (a) launches (torch.profiler's kernel events) and saving / (that count x 1.6 .. 1.9 us).
--layer --shared: DeepSeek-V3 with its one shared expert (of the routed experts' size), T = 1, 16, 64, 512, graph replays on one stream, measured
a, b, a, b: (a) fp4_moe_routed(..., num_shared=1) on the 257-expert stacks -- the shared expert is slot topk of every token, in the layer's own
launches; (b) what a caller does without it: fp4_moe_routed on the 256 routed experts, the shared expert as two dense mul_nvfp4_a16 calls
(gate_up with fused SiLU-mul, down) on the same weights, and a torch add.
--layer --from-hidden: the layer from the hidden state (see hidden_layer_cells): the caller's linear + .float() + fp4_moe_routed against
fp4_moe_routed(router_weight=...), each model with its real router (E, K), measured a, b, a, b.
--gptoss: the gpt-oss-20b / -120b expert block (bf16 x MXFP4, 2880 -> 3072, biases, activation="swiglu_oai"): see gptoss_cells.  The two
models are also in the model list of the default cells (--models gpt-oss-20b,gpt-oss-120b: MXFP4 pools).
Kernel times without launch gaps: run under `rocprofv3 --kernel-trace --stats -- python tools/moe_bench.py ...`.
Prints one JSON object (and writes it to --out).
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "petit-kernel_amd"))

MODELS = {  # (gate_up n x k, down n x k, E, top-k)
    "deepseek": ((4096, 7168), (7168, 2048), 256, 8),
    "qwen3": ((1536, 2048), (2048, 768), 128, 8),
    "mixtral": ((32768, 6144), (6144, 16384), 8, 2),
    # gpt-oss: H = I = 2880, padded to 3072 by petit_kernel.gptoss (gate_up [2 * 3072, 3072], down [2880, 3072]); bf16 x MXFP4
    "gpt-oss-20b": ((6144, 3072), (2880, 3072), 32, 4),
    "gpt-oss-120b": ((6144, 3072), (2880, 3072), 128, 4),
}
MODEL_KIND = {"gpt-oss-20b": "mx", "gpt-oss-120b": "mx"}   # weight format of a model's cells (default "nv": NVFP4)
DECODE_T, PREFILL_T = (1, 4, 16, 64), (1024, 4096)
POOL_BYTES = 1 << 30


class Pool:
    """copies of E experts' packed [n, k] NVFP4 (kind "nv") or MXFP4 ("mx") weights (random bytes: timing only)"""

    def __init__(self, pk, E, n, k, kind="nv"):
        self.E, self.n, self.k, self.kind = E, n, k, kind
        self.w_bytes, self.s_bytes = n * k // 2, n * k // (16 if kind == "nv" else 32)
        per_copy = E * (self.w_bytes + self.s_bytes)
        self.copies = max(1, -(-POOL_BYTES // per_copy))
        g = torch.Generator(device="cuda").manual_seed(n * 31 + k)
        self.b = [torch.randint(-2 ** 31, 2 ** 31 - 1, (E * n // 16, 2 * k), dtype=torch.int32, device="cuda", generator=g) for _ in range(self.copies)]
        # e4m3 scales in [0.25, 4): exponent field 5..8; e8m0 scales 2^-9 .. 2^-1
        if kind == "nv":
            self.s = [(torch.randint(0x28, 0x40, (E * n, k // 16), dtype=torch.uint8, device="cuda", generator=g)).view(torch.float8_e4m3fn)
                      for _ in range(self.copies)]
        else:
            self.s = [torch.randint(118, 127, (E * n // 32, k), dtype=torch.uint8, device="cuda", generator=g) for _ in range(self.copies)]
        self.gs = torch.rand(E, device="cuda") + 0.5

    def expert(self, c, e):
        n, k = self.n, self.k
        b = self.b[c].view(-1)[e * n * k // 8:(e + 1) * n * k // 8].view(n // 16, 2 * k)
        s = self.s[c].view(-1)[e * self.s_bytes:(e + 1) * self.s_bytes]
        return b, (s.view(n, k // 16) if self.kind == "nv" else s.view(n // 32, k)), self.gs[e:e + 1]


def routings(T, E, topk, count, seed):
    out = []
    g = torch.Generator().manual_seed(seed)
    for _ in range(count):
        ids = torch.topk(torch.randn(T, E, generator=g), topk, dim=-1).indices
        counts = torch.bincount(ids.reshape(-1), minlength=E)
        offs = torch.zeros(E + 1, dtype=torch.int32)
        offs[1:] = torch.cumsum(counts, 0)
        out.append((counts.tolist(), offs))
    return out


def time_us(fn, iters):
    for i in range(3):
        fn(i)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(iters):
        fn(i)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def cell(pk, pool, T, topk, iters, do_moe=True, do_loop=True, seed=0):
    E, n, k = pool.E, pool.n, pool.k
    m = T * topk
    routes = routings(T, E, topk, 16, seed)
    a = torch.randn(m, k, device="cuda").to(torch.bfloat16)
    offs_d = [o.to("cuda") for _, o in routes]
    res = {"T": T, "E": E, "topk": topk, "n": n, "k": k, "m": m}
    act = [sum(1 for c in cnt if c) for cnt, _ in routes]
    res["active_experts_mean"] = sum(act) / len(act)
    res["active_bytes_mean"] = sum(a_ * (pool.w_bytes + pool.s_bytes) for a_ in act) / len(act) + 2 * m * k + 2 * m * n
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = torch.bfloat16
    h.b_type = pk.DataType.float4_e2m1 if pool.kind == "nv" else pk.DataType.mxfloat4_e2m1
    res["moe_solution"] = pk.ops._lib.describe_solution(pk.moe_resolve_solution(h, E, m, n, k, -1))
    mul_moe, mul_dense = (pk.mul_nvfp4_a16_moe, pk.mul_nvfp4_a16) if pool.kind == "nv" else (pk.mul_mxfp4_a16_moe, pk.mul_mxfp4_a16)

    def moe(i):
        c = i % pool.copies
        mul_moe(a, pool.b[c], pool.s[c], pool.gs, offs_d[i % len(offs_d)], m, n, k, E)

    def loop(i):
        c = i % pool.copies
        cnt, offs = routes[i % len(routes)]
        for e in range(E):
            if cnt[e]:
                b, s, gs = pool.expert(c, e)
                lo = int(offs[e])
                mul_dense(a[lo:lo + cnt[e]], b, s, gs, cnt[e], n, k, -1)

    if do_moe:
        res["moe_us"] = time_us(moe, iters)
        res["moe_TBps_active"] = res["active_bytes_mean"] / res["moe_us"] / 1e6
    if do_loop:
        res["loop_us"] = time_us(loop, max(3, iters // 4))
        res["loop_TBps_active"] = res["active_bytes_mean"] / res["loop_us"] / 1e6
    if do_moe and do_loop:
        res["speedup_vs_loop"] = res["loop_us"] / res["moe_us"]
    return res


def single_expert(pk, iters):
    """every row on one expert: the MoE launch against the dense call with the same id (DeepSeek gate_up shape, E = 256)"""
    out = []
    pool = Pool(pk, 256, 4096, 7168)
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = torch.bfloat16
    h.b_type = pk.DataType.float4_e2m1
    for m in (1, 16, 512):
        E, n, k = pool.E, pool.n, pool.k
        a = torch.randn(m, k, device="cuda").to(torch.bfloat16)
        offs = []
        for e in range(16):
            o = torch.zeros(E + 1, dtype=torch.int32)
            o[e * 7 + 1:] = m
            offs.append((e * 7, o.to("cuda")))
        sid = pk.moe_resolve_solution(h, 1, m, n, k, -1)   # (the pick for m rows on one expert, which the dense call also runs)

        def moe(i):
            pk.mul_nvfp4_a16_moe(a, pool.b[0], pool.s[0], pool.gs, offs[i % 16][1], m, n, k, E, sid)

        def dense(i):
            b, s, gs = pool.expert(0, offs[i % 16][0])
            pk.mul_nvfp4_a16(a, b, s, gs, m, n, k, sid)

        mu, du = time_us(moe, iters), time_us(dense, iters)
        out.append({"m": m, "solution": pk.ops._lib.describe_solution(sid), "moe_us": mu, "dense_us": du, "moe_over_dense": mu / du})
    return out


LAYER_T = (1, 4, 16, 64, 1024, 4096)
NATIVE_LAYER_T = (1, 16, 64, 1024, 4096)


def graph_us(fn, iters, per_graph=1):
    """fn captured `per_graph` times in one graph (one stream), replayed `iters` times: microseconds per fn"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(per_graph):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        g.replay()
    t1.record()
    torch.cuda.synchronize()
    del g
    return t0.elapsed_time(t1) * 1e3 / (iters * per_graph)


def layer_cells(pk, models, ts, iters):
    from petit_kernel.moe import moe_align
    cells = []
    for name in models:
        (n13, hid), (_, inter), E, topk = MODELS[name]
        g = torch.Generator(device="cuda").manual_seed(7)
        w13 = torch.randint(-2 ** 31, 2 ** 31 - 1, (E * n13 // 16, 2 * hid), dtype=torch.int32, device="cuda", generator=g)
        s13 = torch.randint(0x28, 0x40, (E * n13, hid // 16), dtype=torch.uint8, device="cuda", generator=g).view(torch.float8_e4m3fn)
        w2 = torch.randint(-2 ** 31, 2 ** 31 - 1, (E * hid // 16, 2 * inter), dtype=torch.int32, device="cuda", generator=g)
        s2 = torch.randint(0x28, 0x40, (E * hid, inter // 16), dtype=torch.uint8, device="cuda", generator=g).view(torch.float8_e4m3fn)
        gs13, gs2 = torch.rand(E, device="cuda") * 0.01 + 0.01, torch.rand(E, device="cuda") * 0.01 + 0.01
        for T in ts:
            m = T * topk
            it = iters if T < 1024 else max(5, iters // 5)
            x = torch.randn(T, hid, device="cuda").to(torch.bfloat16)
            logits = torch.randn(T, E, device="cuda", generator=g)
            tw, tid = torch.topk(torch.softmax(logits, -1), topk, dim=-1)
            tw, tid = tw.float().contiguous(), tid.to(torch.int32).contiguous()
            args = (x, w13, s13, gs13, w2, s2, gs2, tw, tid)
            r = {"model": name, "T": T, "E": E, "topk": topk, "hidden": hid, "inter": inter}
            r["fp4_moe_us"] = graph_us(lambda: pk.fp4_moe(*args), it)
            r["fp4_moe_fused_us"] = graph_us(lambda: pk.fp4_moe_fused(*args), it)
            # the GEMMs alone: plain on pre-gathered rows against indexed
            sorted_idx, offs = moe_align(tid, E)
            tok = (sorted_idx // topk).int()
            xg = x.index_select(0, sorted_idx // topk)
            h = pk.mul_nvfp4_a16_moe(xg, w13, s13, gs13, offs, m, n13, hid, E, activation="silu_mul")
            out = torch.empty(m, hid, dtype=torch.bfloat16, device="cuda")
            r["gate_up_plain_us"] = graph_us(lambda: pk.mul_nvfp4_a16_moe(xg, w13, s13, gs13, offs, m, n13, hid, E, activation="silu_mul"), it, 10)
            r["gate_up_indexed_us"] = graph_us(lambda: pk.mul_nvfp4_a16_moe_indexed(x, w13, s13, gs13, offs, m, n13, hid, E, a_row_index=tok,
                                                                                    activation="silu_mul"), it, 10)
            r["down_plain_us"] = graph_us(lambda: pk.mul_nvfp4_a16_moe(h, w2, s2, gs2, offs, m, hid, inter, E), it, 10)
            r["down_indexed_us"] = graph_us(lambda: pk.mul_nvfp4_a16_moe_indexed(h, w2, s2, gs2, offs, m, hid, inter, E, c_row_index=sorted_idx.int(),
                                                                                 out=out), it, 10)
            print(json.dumps(r), file=sys.stderr, flush=True)
            cells.append(r)
        del w13, s13, w2, s2
        torch.cuda.empty_cache()
    return cells


ROUTING = {  # moe_route's keyword arguments per model
    "deepseek": dict(scoring="sigmoid", renormalize=True, n_group=8, topk_group=4, routed_scaling_factor=2.5),
    "qwen3": dict(scoring="softmax", renormalize=True),
    "mixtral": dict(scoring="softmax", renormalize=True),
    "gpt-oss-20b": dict(scoring="softmax", renormalize=True),
    "gpt-oss-120b": dict(scoring="softmax", renormalize=True),
}


def torch_routing(name, logits, topk, bias=None):
    """The routing chain a caller runs in front of fp4_moe_fused today: (topk_weights float32, topk_ids int32)."""
    if name.startswith("gpt-oss"):                      # the top-k logits, softmax over the k
        v, ids = torch.topk(logits, topk, dim=-1)
        return torch.softmax(v.float(), -1), ids.to(torch.int32)
    if name != "deepseek":                              # softmax over all, top-k, renormalise
        w, ids = torch.topk(torch.softmax(logits.float(), -1), topk, dim=-1)
        return w / w.sum(-1, keepdim=True), ids.to(torch.int32)
    r = ROUTING[name]                                   # DeepSeek-V3: sigmoid, correction bias, group-limited top-k, renormalise, scale
    T, E = logits.shape
    scores = logits.float().sigmoid()
    biased = scores + bias
    group_scores = biased.view(T, r["n_group"], -1).topk(2, dim=-1)[0].sum(-1)
    group_idx = torch.topk(group_scores, r["topk_group"], dim=-1, sorted=False)[1]
    group_mask = torch.zeros_like(group_scores).scatter_(1, group_idx, 1)
    score_mask = group_mask.unsqueeze(-1).expand(T, r["n_group"], E // r["n_group"]).reshape(T, E)
    ids = torch.topk(biased.masked_fill(~score_mask.bool(), float("-inf")), topk, dim=-1, sorted=False)[1]
    w = scores.gather(1, ids)
    w = w / (w.sum(-1, keepdim=True) + 1e-20)
    return w * r["routed_scaling_factor"], ids.to(torch.int32)


def kernel_launches(fn):
    """kernels fn launches (eagerly), from torch.profiler's device-side kernel events; None when the profiler reports none"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "emcpy" not in e.name and "emset" not in e.name)
    return n or None


def routed_layer_cells(pk, models, ts, iters):
    """--layer --from-logits (module docstring): a = torch routing chain + fp4_moe_fused, b = fp4_moe_routed, measured a, b, a, b."""
    cells = []
    for name in models:
        (n13, hid), (n2, inter), E, topk = MODELS[name]
        kind = "mxfp4" if MODEL_KIND.get(name) == "mx" else "nvfp4"
        g = torch.Generator(device="cuda").manual_seed(7)
        ri = lambda *shape: torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device="cuda", generator=g)  # noqa: E731
        w13, w2 = ri(E * n13 // 16, 2 * hid), ri(E * n2 // 16, 2 * inter)
        if kind == "nvfp4":
            s13 = torch.randint(0x28, 0x40, (E * n13, hid // 16), dtype=torch.uint8, device="cuda", generator=g).view(torch.float8_e4m3fn)
            s2 = torch.randint(0x28, 0x40, (E * n2, inter // 16), dtype=torch.uint8, device="cuda", generator=g).view(torch.float8_e4m3fn)
            gs13, gs2 = torch.rand(E, device="cuda") * 0.01 + 0.01, torch.rand(E, device="cuda") * 0.01 + 0.01
            extra = {}
        else:
            s13 = torch.randint(118, 127, (E * n13 // 32, hid), dtype=torch.uint8, device="cuda", generator=g)
            s2 = torch.randint(118, 127, (E * n2 // 32, inter), dtype=torch.uint8, device="cuda", generator=g)
            gs13, gs2 = torch.ones(E, device="cuda"), torch.ones(E, device="cuda")
            extra = dict(bias13=torch.randn(E, n13, device="cuda").bfloat16(), bias2=torch.randn(E, n2, device="cuda").bfloat16(),
                         activation="swiglu_oai")
        routing = dict(ROUTING[name])
        bias = torch.randn(E, device="cuda", generator=g) * 0.1 if name == "deepseek" else None
        if bias is not None:
            routing["bias"] = bias
        for T in ts:
            it = iters if T < 1024 else max(5, iters // 5)
            x = torch.randn(T, hid, device="cuda").to(torch.bfloat16)
            logits = torch.randn(T, E, device="cuda", generator=g).to(torch.bfloat16)
            wts = (x, w13, s13, gs13, w2, s2, gs2)

            def a():
                tw, tid = torch_routing(name, logits, topk, bias)
                return pk.fp4_moe_fused(*wts, tw, tid, kind, **extra)

            def b():
                return pk.fp4_moe_routed(x, logits, w13, s13, gs13, w2, s2, gs2, topk, kind, **extra, **routing)

            r = {"model": name, "T": T, "E": E, "topk": topk, "hidden": hid, "inter": inter}
            r["torch_chain_fused_us"], r["routed_us"] = [], []
            for _ in range(2):
                r["torch_chain_fused_us"].append(graph_us(a, it))
                r["routed_us"].append(graph_us(b, it))
            try:
                r["chain_launches"] = kernel_launches(lambda: torch_routing(name, logits, topk, bias))
            except Exception as exc:  # noqa: BLE001 -- a count, not a time: the cell stands without it
                r["chain_launches"], r["chain_launches_error"] = None, repr(exc)
            saving = [x_ - y_ for x_, y_ in zip(r["torch_chain_fused_us"], r["routed_us"])]
            r["saving_us"] = saving
            if r["chain_launches"]:
                r["saving_over_expected"] = [[s_ / (r["chain_launches"] * c) for c in (1.9, 1.6)] for s_ in saving]
            print(json.dumps(r), file=sys.stderr, flush=True)
            cells.append(r)
        del w13, s13, w2, s2
        torch.cuda.empty_cache()
    return cells


ROUTER_K = {"gpt-oss-20b": 2880, "gpt-oss-120b": 2880}   # the router's K where the experts' hidden size is a padded one


def hidden_layer_cells(pk, models, ts, iters):
    """--layer --from-hidden: the layer from the hidden state, each model with its real router (E, K), graph replays on one stream.
    a = the caller's path today: torch.nn.functional.linear(x, W, b) in the model's dtype, .float(), fp4_moe_routed(x, logits, ...);
    b = fp4_moe_routed(x, None, ..., router_weight=W, router_bias=b).  Measured a, b, a, b in one process: the two a's are the spread.
    Per cell also the two routers alone (linear + .float() against moe_router_logits) and the slab count of the form T gets."""
    from petit_kernel import ops
    cells = []
    for name in models:
        (n13, hid), (n2, inter), E, topk = MODELS[name]
        kind = "mxfp4" if MODEL_KIND.get(name) == "mx" else "nvfp4"
        g = torch.Generator(device="cuda").manual_seed(7)
        ri = lambda *shape: torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device="cuda", generator=g)  # noqa: E731
        w13, w2 = ri(E * n13 // 16, 2 * hid), ri(E * n2 // 16, 2 * inter)
        if kind == "nvfp4":
            s13 = torch.randint(0x28, 0x40, (E * n13, hid // 16), dtype=torch.uint8, device="cuda", generator=g).view(torch.float8_e4m3fn)
            s2 = torch.randint(0x28, 0x40, (E * n2, inter // 16), dtype=torch.uint8, device="cuda", generator=g).view(torch.float8_e4m3fn)
            gs13, gs2 = torch.rand(E, device="cuda") * 0.01 + 0.01, torch.rand(E, device="cuda") * 0.01 + 0.01
            extra = {}
        else:
            s13 = torch.randint(118, 127, (E * n13 // 32, hid), dtype=torch.uint8, device="cuda", generator=g)
            s2 = torch.randint(118, 127, (E * n2 // 32, inter), dtype=torch.uint8, device="cuda", generator=g)
            gs13, gs2 = torch.ones(E, device="cuda"), torch.ones(E, device="cuda")
            extra = dict(bias13=torch.randn(E, n13, device="cuda").bfloat16(), bias2=torch.randn(E, n2, device="cuda").bfloat16(),
                         activation="swiglu_oai")
        routing = dict(ROUTING[name])
        if name == "deepseek":
            routing["bias"] = torch.randn(E, device="cuda", generator=g) * 0.1
        K = ROUTER_K.get(name, hid)
        W = (torch.randn(E, K, device="cuda", generator=g) / K ** 0.5).to(torch.bfloat16)
        rb = torch.randn(E, device="cuda", generator=g) if name.startswith("gpt-oss") else None   # gpt-oss's router has a bias
        rb16 = None if rb is None else rb.to(torch.bfloat16)                                       # (the model's own parameter dtype)
        S, L = ops.router_geometry(E, K)
        for T in ts:
            it = iters if T < 1024 else max(5, iters // 5)
            x = torch.randn(T, hid, device="cuda").to(torch.bfloat16)
            xr = x if K == hid else x[:, :K].contiguous()                                          # what the router reads
            rin = {} if K == hid else {"router_input": xr}

            def linear():
                return torch.nn.functional.linear(xr, W, rb16).float()

            def a():
                return pk.fp4_moe_routed(x, linear(), w13, s13, gs13, w2, s2, gs2, topk, kind, **extra, **routing)

            def b():
                return pk.fp4_moe_routed(x, None, w13, s13, gs13, w2, s2, gs2, topk, kind, router_weight=W, router_bias=rb, **rin, **extra,
                                         **routing)

            r = {"model": name, "T": T, "E": E, "K": K, "topk": topk, "hidden": hid, "inter": inter, "slices": S, "slice_k": L,
                 "slabs": ops.router_slabs(T, E, K)}
            r["linear_routed_us"], r["from_hidden_us"] = [], []
            for _ in range(2):
                r["linear_routed_us"].append(graph_us(a, it))
                r["from_hidden_us"].append(graph_us(b, it))
            r["linear_alone_us"] = graph_us(linear, it)
            r["router_logits_alone_us"] = graph_us(lambda: pk.moe_router_logits(xr, W, rb), it)
            r["saving_us"] = [x_ - y_ for x_, y_ in zip(r["linear_routed_us"], r["from_hidden_us"])]
            r["spread_a_us"] = abs(r["linear_routed_us"][0] - r["linear_routed_us"][1])
            r["meets"] = all(s_ > 0 for s_ in r["saving_us"]) if T <= 64 else all(-s_ <= r["spread_a_us"] for s_ in r["saving_us"])
            print(json.dumps(r), file=sys.stderr, flush=True)
            cells.append(r)
        del w13, s13, w2, s2
        torch.cuda.empty_cache()
    return cells


SHARED_T = (1, 16, 64, 512)


def shared_layer_cells(pk, ts, iters):
    """--layer --shared (module docstring): a = fp4_moe_routed with num_shared=1, b = fp4_moe_routed + two dense calls + add; a, b, a, b."""
    (n13, hid), (n2, inter), E, topk = MODELS["deepseek"]
    g = torch.Generator(device="cuda").manual_seed(7)
    ri = lambda *shape: torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device="cuda", generator=g)  # noqa: E731
    EA = E + 1                                                   # the routed experts, then the shared one
    w13, w2 = ri(EA * n13 // 16, 2 * hid), ri(EA * n2 // 16, 2 * inter)
    s13 = torch.randint(0x28, 0x40, (EA * n13, hid // 16), dtype=torch.uint8, device="cuda", generator=g).view(torch.float8_e4m3fn)
    s2 = torch.randint(0x28, 0x40, (EA * n2, inter // 16), dtype=torch.uint8, device="cuda", generator=g).view(torch.float8_e4m3fn)
    gs13, gs2 = torch.rand(EA, device="cuda") * 0.01 + 0.01, torch.rand(EA, device="cuda") * 0.01 + 0.01
    routing = dict(ROUTING["deepseek"], bias=torch.randn(E, device="cuda", generator=g) * 0.1)
    # the routed experts alone (the stacks' first E experts) and the shared expert's dense operands (expert E)
    r13, rs13 = w13.view(-1)[:E * n13 * hid // 8].view(E * n13 // 16, 2 * hid), s13.view(-1)[:E * n13 * hid // 16].view(E * n13, hid // 16)
    r2, rs2 = w2.view(-1)[:E * n2 * inter // 8].view(E * n2 // 16, 2 * inter), s2.view(-1)[:E * n2 * inter // 16].view(E * n2, inter // 16)
    d13, ds13 = w13.view(-1)[E * n13 * hid // 8:].view(n13 // 16, 2 * hid), s13.view(-1)[E * n13 * hid // 16:].view(n13, hid // 16)
    d2, ds2 = w2.view(-1)[E * n2 * inter // 8:].view(n2 // 16, 2 * inter), s2.view(-1)[E * n2 * inter // 16:].view(n2, inter // 16)
    cells = []
    for T in ts:
        x = torch.randn(T, hid, device="cuda").to(torch.bfloat16)
        logits = torch.randn(T, E, device="cuda", generator=g).to(torch.bfloat16)

        def a():
            return pk.fp4_moe_routed(x, logits, w13, s13, gs13, w2, s2, gs2, topk, "nvfp4", num_shared=1, **routing)

        def b():
            out = pk.fp4_moe_routed(x, logits, r13, rs13, gs13[:E], r2, rs2, gs2[:E], topk, "nvfp4", **routing)
            h = pk.mul_nvfp4_a16(x, d13, ds13, gs13[E:], T, n13, hid, -1, activation="silu_mul")
            return out + pk.mul_nvfp4_a16(h, d2, ds2, gs2[E:], T, n2, inter, -1)

        r = {"model": "deepseek", "T": T, "E": E, "topk": topk, "num_shared": 1, "hidden": hid, "inter": inter, "fused_shared_us": [],
             "separate_shared_us": []}
        for _ in range(2):
            r["fused_shared_us"].append(graph_us(a, iters))
            r["separate_shared_us"].append(graph_us(b, iters))
        r["saving_us"] = [y_ - x_ for x_, y_ in zip(r["fused_shared_us"], r["separate_shared_us"])]
        print(json.dumps(r), file=sys.stderr, flush=True)
        cells.append(r)
    return cells


def native_layer_cells(pk, models, ts, iters, fmt):
    """--layer --native FMT: fp4_moe_native (activations quantised to FMT) against fp4_moe_fused on the same weights: MXFP4 weights raw, NVFP4
    weights through their native images (nvfp4_native_images) -- graph replays, as layer_cells"""
    cells = []
    for name in models:
        (n13, hid), (_, inter), E, topk = MODELS[name]
        g = torch.Generator(device="cuda").manual_seed(11)
        rnd = lambda rows, cols: torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, cols), dtype=torch.int32, device="cuda", generator=g)  # noqa: E731
        mx = {"w13": rnd(E * n13 // 16, 2 * hid), "w2": rnd(E * hid // 16, 2 * inter),
              "s13": torch.randint(118, 127, (E * n13 // 32, hid), dtype=torch.uint8, device="cuda", generator=g),
              "s2": torch.randint(118, 127, (E * hid // 32, inter), dtype=torch.uint8, device="cuda", generator=g)}
        nv = {"w13": rnd(E * n13 // 16, 2 * hid), "w2": rnd(E * hid // 16, 2 * inter),
              "s13": torch.randint(0x28, 0x40, (E * n13, hid // 16), dtype=torch.uint8, device="cuda", generator=g).view(torch.float8_e4m3fn),
              "s2": torch.randint(0x28, 0x40, (E * hid, inter // 16), dtype=torch.uint8, device="cuda", generator=g).view(torch.float8_e4m3fn)}
        nv["i13"] = pk.nvfp4_native_images(nv["w13"], nv["s13"], E, n13, hid)
        nv["i2"] = pk.nvfp4_native_images(nv["w2"], nv["s2"], E, hid, inter)
        gs13, gs2 = torch.rand(E, device="cuda") * 0.01 + 0.01, torch.rand(E, device="cuda") * 0.01 + 0.01
        for T in ts:
            it = iters if T < 1024 else max(5, iters // 5)
            x = torch.randn(T, hid, device="cuda").to(torch.bfloat16)
            logits = torch.randn(T, E, device="cuda", generator=g)
            tw, tid = torch.topk(torch.softmax(logits, -1), topk, dim=-1)
            tw, tid = tw.float().contiguous(), tid.to(torch.int32).contiguous()
            r = {"model": name, "T": T, "E": E, "topk": topk, "hidden": hid, "inter": inter, "activations": fmt}
            fused = lambda w, kind: pk.fp4_moe_fused(x, w["w13"], w["s13"], gs13, w["w2"], w["s2"], gs2, tw, tid, kind=kind)  # noqa: E731
            r["mx_fused_us"] = graph_us(lambda: fused(mx, "mxfp4"), it)
            r["mx_native_us"] = graph_us(lambda: pk.fp4_moe_native(x, mx["w13"], mx["s13"], gs13, mx["w2"], mx["s2"], gs2, tw, tid, kind="mxfp4",
                                                                    activations=fmt), it)
            r["nv_fused_us"] = graph_us(lambda: fused(nv, "nvfp4"), it)
            r["nv_native_us"] = graph_us(lambda: pk.fp4_moe_native(x, nv["i13"], None, gs13, nv["i2"], None, gs2, tw, tid, kind="nvfp4",
                                                                    activations=fmt), it)
            r["mx_speedup"] = r["mx_fused_us"] / r["mx_native_us"]
            r["nv_speedup"] = r["nv_fused_us"] / r["nv_native_us"]
            print(json.dumps(r), file=sys.stderr, flush=True)
            cells.append(r)
        del mx, nv
        torch.cuda.empty_cache()
    return cells


def native_single_expert(pk, iters, fmt, m=4096):
    """every row on one expert (DeepSeek-V3 gate_up, MXFP4, E = 256), activations pre-quantised: the native MoE launch against the dense native
    call with the same id (the indirection cost)"""
    E, n, k = 256, 4096, 7168
    g = torch.Generator(device="cuda").manual_seed(5)
    w = torch.randint(-2 ** 31, 2 ** 31 - 1, (E * n // 16, 2 * k), dtype=torch.int32, device="cuda", generator=g)
    s = torch.randint(118, 127, (E * n // 32, k), dtype=torch.uint8, device="cuda", generator=g)
    gs = torch.rand(E, device="cuda") + 0.5
    qa = pk.quantize_activation_rows(torch.randn(m, k, device="cuda").to(torch.bfloat16), fmt)
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = torch.bfloat16
    h.b_type = pk.DataType.mxfloat4_e2m1
    sid = pk.native_moe_resolve_solution(h, E, m, n, k, {"mxfp8": -2, "mxfp4": -3, "mxfp6": -4}[fmt], a_format=fmt)
    offs = []
    for e in range(16):
        o = torch.zeros(E + 1, dtype=torch.int32)
        o[e * 7 + 1:] = m
        offs.append((e * 7, o.to("cuda")))

    def moe(i):
        pk.mul_mxfp4_native_moe(qa, w, s, gs, offs[i % 16][1], m, n, k, E, solution_id=sid)

    def dense(i):
        e = offs[i % 16][0]
        b = w.view(-1)[e * n * k // 8:(e + 1) * n * k // 8].view(n // 16, 2 * k)
        se = s.view(-1)[e * n * k // 32:(e + 1) * n * k // 32].view(n // 32, k)
        pk.mul_mxfp4_native(qa, b, se, gs[e:e + 1], m, n, k, sid)

    mu, du = time_us(moe, iters), time_us(dense, iters)
    return {"m": m, "n": n, "k": k, "E": E, "activations": fmt, "solution": pk.ops._lib.describe_solution(sid), "moe_us": mu, "dense_us": du,
            "moe_over_dense": mu / du}


def gptoss_cells(pk, models, ts, iters):
    """--gptoss: gpt-oss-20b / -120b expert blocks (bf16 x MXFP4, H = I = 2880 -> 3072, top-4, biases, activation="swiglu_oai"), graph replays:
      fused_us / native_us   prepare_gptoss_experts(...).forward on the fused and the native (MXFP8 activations) path, x padding included
      loop_us                the host loop a caller without the MoE launch runs: per active expert one dense gate_up (fused activation and
                             bias) and one dense down (bias) on that expert's rows, eager launches, no gather and no combine (GEMMs only)
      act_fused_us           the gate_up MoE launch with activation="swiglu_oai" and the bias
      act_unfused_us         the same launch with activation=None ([m, 2 I] out) plus the torch expression of the activation on it"""
    from petit_kernel.gptoss import GptOssExperts
    from petit_kernel.moe import moe_align
    cells = []
    for name in models:
        (n13, hp), (hid, ip), E, topk = MODELS[name]
        g = torch.Generator(device="cuda").manual_seed(3)
        rnd = lambda rows, cols: torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, cols), dtype=torch.int32, device="cuda", generator=g)  # noqa: E731
        ex = GptOssExperts(w13=rnd(E * n13 // 16, 2 * hp), s13=torch.randint(118, 124, (E * n13 // 32, hp), dtype=torch.uint8, device="cuda", generator=g),
                           w2=rnd(E * hid // 16, 2 * ip), s2=torch.randint(118, 124, (E * hid // 32, ip), dtype=torch.uint8, device="cuda", generator=g),
                           gs13=torch.ones(E, device="cuda"), gs2=torch.ones(E, device="cuda"),
                           bias13=(torch.randn(E, n13, device="cuda") * 0.5).bfloat16(), bias2=(torch.randn(E, hid, device="cuda") * 0.5).bfloat16(),
                           hidden=hid, inter=hid, hidden_padded=hp, inter_padded=ip)
        for T in ts:
            m = T * topk
            it = iters if T < 1024 else max(5, iters // 5)
            x = (torch.randn(T, hid, device="cuda") * 0.05).to(torch.bfloat16)
            tw, tid = torch.topk(torch.softmax(torch.randn(T, E, device="cuda", generator=g), -1), topk, dim=-1)
            tw, tid = (tw / tw.sum(-1, keepdim=True)).float().contiguous(), tid.to(torch.int32).contiguous()
            r = {"model": name, "T": T, "E": E, "topk": topk, "hidden": hid, "padded": hp}
            r["fused_us"] = graph_us(lambda: ex.forward(x, tw, tid, path="fused"), it)
            r["native_us"] = graph_us(lambda: ex.forward(x, tw, tid, path="native", activations="mxfp8"), it)
            sorted_idx, offs = moe_align(tid, E)
            tok = (sorted_idx // topk).int()
            xg = ex.pad_hidden(x).index_select(0, sorted_idx // topk)
            cnt = (offs[1:] - offs[:-1]).tolist()
            lo_of = offs.tolist()
            hmid = torch.zeros(m, ip, dtype=torch.bfloat16, device="cuda")

            def loop(_i):
                for e in range(E):
                    if cnt[e]:
                        lo = lo_of[e]
                        b13 = ex.w13.view(-1)[e * n13 * hp // 8:(e + 1) * n13 * hp // 8].view(n13 // 16, 2 * hp)
                        s13 = ex.s13.view(-1)[e * n13 * hp // 32:(e + 1) * n13 * hp // 32].view(n13 // 32, hp)
                        hh = pk.mul_mxfp4_a16(xg[lo:lo + cnt[e]], b13, s13, ex.gs13[e:e + 1], cnt[e], n13, hp, -1, bias=ex.bias13[e],
                                              activation="swiglu_oai")
                        b2 = ex.w2.view(-1)[e * hid * ip // 8:(e + 1) * hid * ip // 8].view(hid // 16, 2 * ip)
                        s2 = ex.s2.view(-1)[e * hid * ip // 32:(e + 1) * hid * ip // 32].view(hid // 32, ip)
                        pk.mul_mxfp4_a16(hh, b2, s2, ex.gs2[e:e + 1], cnt[e], hid, ip, -1, bias=ex.bias2[e])

            r["loop_us"] = time_us(loop, max(3, it // 4))
            xp = ex.pad_hidden(x)
            gate_up = lambda act: pk.mul_mxfp4_a16_moe_indexed(xp, ex.w13, ex.s13, ex.gs13, offs, m, n13, hp, E, a_row_index=tok, bias=ex.bias13,  # noqa: E731
                                                               activation=act)

            def unfused():
                y = gate_up(None)
                gt = y[:, :ip].clamp(max=7.0)
                return gt * torch.sigmoid(1.702 * gt) * (y[:, ip:].clamp(-7.0, 7.0) + 1)

            r["act_fused_us"] = graph_us(lambda: gate_up("swiglu_oai"), it, 10)
            r["act_unfused_us"] = graph_us(unfused, it, 10)
            r["fused_over_loop"] = r["loop_us"] / r["fused_us"]
            r["native_over_fused"] = r["fused_us"] / r["native_us"]
            r["act_fused_speedup"] = r["act_unfused_us"] / r["act_fused_us"]
            print(json.dumps(r), file=sys.stderr, flush=True)
            cells.append(r)
        del ex
        torch.cuda.empty_cache()
    return cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="all", choices=["decode", "prefill", "all"])
    ap.add_argument("--models", default="deepseek,qwen3,mixtral")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--only-moe", action="store_true")
    ap.add_argument("--only-loop", action="store_true")
    ap.add_argument("--single-expert", action="store_true")
    ap.add_argument("--layer", action="store_true")
    ap.add_argument("--t", default="", help="--layer: comma-separated token counts (default 1,4,16,64,1024,4096)")
    ap.add_argument("--native", default="", choices=["", "mxfp8", "mxfp6", "mxfp4"],
                    help="--layer: fp4_moe_native with these activations against fp4_moe_fused (MXFP4 raw and NVFP4 images), plus the single-expert cell")
    ap.add_argument("--from-logits", action="store_true", help="--layer: the torch routing chain + fp4_moe_fused against fp4_moe_routed")
    ap.add_argument("--from-hidden", action="store_true",
                    help="--layer: linear + .float() + fp4_moe_routed against fp4_moe_routed(router_weight=...), each model's real router (E, K)")
    ap.add_argument("--shared", action="store_true", help="--layer: DeepSeek-V3 with its shared expert as slot topk of fp4_moe_routed against separate dense calls")
    ap.add_argument("--gptoss", action="store_true", help="the gpt-oss expert block (petit_kernel.gptoss): layer, host loop, native, fused activation")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import petit_kernel as pk
    report = {"device": torch.cuda.get_device_properties(0).gcnArchName, "cells": []}
    if args.gptoss:
        ts = tuple(int(t) for t in args.t.split(",")) if args.t else LAYER_T
        models = [m for m in args.models.split(",") if m in MODEL_KIND] or list(MODEL_KIND)
        report["gptoss"] = gptoss_cells(pk, models, ts, args.iters)
    elif args.layer and args.shared:
        ts = tuple(int(t) for t in args.t.split(",")) if args.t else SHARED_T
        report["shared_layer"] = shared_layer_cells(pk, ts, args.iters)
    elif args.layer and args.from_hidden:
        ts = tuple(int(t) for t in args.t.split(",")) if args.t else LAYER_T
        models = args.models.split(",") if args.models != "deepseek,qwen3,mixtral" else ["deepseek", "qwen3", "mixtral", "gpt-oss-120b"]
        report["hidden_layer"] = hidden_layer_cells(pk, models, ts, args.iters)
    elif args.layer and args.from_logits:
        ts = tuple(int(t) for t in args.t.split(",")) if args.t else LAYER_T
        models = args.models.split(",") if args.models != "deepseek,qwen3,mixtral" else ["deepseek", "qwen3", "mixtral", "gpt-oss-120b"]
        report["routed_layer"] = routed_layer_cells(pk, models, ts, args.iters)
    elif args.layer and args.native:
        ts = tuple(int(t) for t in args.t.split(",")) if args.t else NATIVE_LAYER_T
        report["native_layer"] = native_layer_cells(pk, args.models.split(","), ts, args.iters, args.native)
        report["native_single_expert"] = native_single_expert(pk, args.iters, args.native)
    elif args.layer:
        ts = tuple(int(t) for t in args.t.split(",")) if args.t else LAYER_T
        report["layer"] = layer_cells(pk, args.models.split(","), ts, args.iters)
    elif args.single_expert:
        report["single_expert"] = single_expert(pk, args.iters)
    else:
        ts = (DECODE_T if args.cells != "prefill" else ()) + (PREFILL_T if args.cells != "decode" else ())
        for name in args.models.split(","):
            gate_up, down, E, topk = MODELS[name]
            for proj, (n, k) in (("gate_up", gate_up), ("down", down)):
                pool = Pool(pk, E, n, k, MODEL_KIND.get(name, "nv"))
                for T in ts:
                    r = cell(pk, pool, T, topk, args.iters if T < 1024 else max(5, args.iters // 10), not args.only_loop, not args.only_moe, seed=T)
                    r.update(model=name, proj=proj)
                    print(json.dumps(r), file=sys.stderr, flush=True)
                    report["cells"].append(r)
                del pool
                torch.cuda.empty_cache()
    text = json.dumps(report)
    if args.out:
        Path(args.out).write_text(json.dumps(report, indent=1))
    print(text)


if __name__ == "__main__":
    main()

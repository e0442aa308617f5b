#!/usr/bin/env python3
"""tools/moe_nv_transient_bench.py -- the native-class MoE layer on NVFP4 experts WITHOUT resident images against its two neighbours.

    python tools/moe_nv_transient_bench.py [--models deepseek,qwen3,mixtral] [--ts 16,64,512,4096] [--iters N] [--activations mxfp8] [--out FILE]

Per cell (model, T tokens; random weights and router logits: timing only), each variant captured once in a torch.cuda.graph on one stream and
replayed (tools/moe_bench.py graph_us), measured a, b, c, a, b, c in one process (both passes reported, *_us their mean), microseconds per layer:
  transient_us   fp4_moe_native(kind="nvfp4", transient=True): the packed tensors, the images of the routed experts built per launch
  resident_us    fp4_moe_native(kind="nvfp4") on nvfp4_native_images built once (not timed)
  fused_us       fp4_moe_fused, the exact class, on the packed tensors
and the weight bytes each variant holds per layer (packed 4.5 bits per weight; resident adds the images, 6.25) next to *_call_peak_bytes, what one
eager call of the variant allocates at its peak (torch.cuda.max_memory_allocated over the call: for transient its one scratch for both launches,
the activations and the output; "transient_scratch" is that scratch as computed, E x the larger image).
Per model also the builder alone (petit_nvfp4_native_images on the gate_up stack, graph replays): every expert (null offsets) as bytes read
plus written over time, against the 6.29 TB/s of a pure copy on this part (README.md), and with the routing skip at T = 16 and 64 (the
routing's expert_offsets), with the number of experts that have rows.
One weight set per model: a layer's experts exceed the 256 MB Infinity Cache for every model here (Qwen3-30B-A3B: 0.33 GB packed), so replays
do not find them cached; at T <= 64 the few routed experts of Qwen3 can stay cached between replays, which favours every variant alike.
Prints one JSON object (and writes it to --out).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "petit-kernel_amd"))
sys.path.insert(0, str(ROOT / "tools"))

from moe_bench import MODELS, graph_us  # noqa: E402

COPY_TBS = 6.29


def builder_cells(pk, name, w13, s13, E, n13, hid, topk, iters):
    from petit_kernel import _lib
    per = int(_lib.lib.petit_nvfp4_native_image_bytes(hid, n13))
    out = torch.empty(E * per, dtype=torch.uint8, device="cuda")
    in_bytes = n13 * hid // 2 + n13 * hid // 16

    def build(off, m):
        rc = _lib.lib.petit_nvfp4_native_images(out.data_ptr(), w13.data_ptr(), s13.data_ptr(), E, hid, n13, off.data_ptr() if off is not None else None,
                                                m, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0

    us = graph_us(lambda: build(None, 0), iters)
    moved = E * (in_bytes + per)
    cells = [{"model": name, "builder": "every expert", "experts_built": E, "us": us, "bytes_moved": moved, "TBs": moved / us / 1e6,
              "of_copy_rate": moved / us / 1e6 / COPY_TBS}]
    g = torch.Generator(device="cuda").manual_seed(5)
    for T in (16, 64):
        ids = torch.topk(torch.randn(T, E, device="cuda", generator=g), topk, dim=-1).indices
        counts = torch.bincount(ids.reshape(-1), minlength=E)
        off = torch.zeros(E + 1, dtype=torch.int32, device="cuda")
        off[1:] = torch.cumsum(counts, 0)
        active = int((counts > 0).sum())
        us_skip = graph_us(lambda: build(off, T * topk), iters)
        moved = active * (in_bytes + per)
        cells.append({"model": name, "builder": f"routing skip, T = {T}", "experts_built": active, "us": us_skip, "us_without_skip": us,
                      "bytes_moved": moved, "TBs": moved / us_skip / 1e6, "of_copy_rate": moved / us_skip / 1e6 / COPY_TBS})
    return cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="deepseek,qwen3,mixtral")
    ap.add_argument("--ts", default="16,64,512,4096")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--activations", default="mxfp8")
    ap.add_argument("--out")
    args = ap.parse_args()
    import petit_kernel as pk
    from petit_kernel import _lib
    fmt = args.activations
    layers, builders = [], []
    for name in args.models.split(","):
        (n13, hid), (_, inter), E, topk = MODELS[name]
        g = torch.Generator(device="cuda").manual_seed(11)
        rnd = lambda rows, cols: torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, cols), dtype=torch.int32, device="cuda", generator=g)  # noqa: E731
        w13, w2 = rnd(E * n13 // 16, 2 * hid), rnd(E * hid // 16, 2 * inter)
        s13 = torch.randint(0x28, 0x40, (E * n13, hid // 16), dtype=torch.uint8, device="cuda", generator=g).view(torch.float8_e4m3fn)
        s2 = torch.randint(0x28, 0x40, (E * hid, inter // 16), dtype=torch.uint8, device="cuda", generator=g).view(torch.float8_e4m3fn)
        gs13, gs2 = torch.rand(E, device="cuda") * 0.01 + 0.01, torch.rand(E, device="cuda") * 0.01 + 0.01
        builders += builder_cells(pk, name, w13, s13, E, n13, hid, topk, args.iters)
        for c in builders[-3:]:
            print(json.dumps(c), file=sys.stderr, flush=True)
        i13, i2 = pk.nvfp4_native_images(w13, s13, E, n13, hid), pk.nvfp4_native_images(w2, s2, E, hid, inter)
        packed = sum(t.numel() * t.element_size() for t in (w13, s13, w2, s2))
        images = i13.numel() + i2.numel()
        scratch = E * max(int(_lib.lib.petit_nvfp4_native_image_bytes(hid, n13)), int(_lib.lib.petit_nvfp4_native_image_bytes(inter, hid)))
        for T in map(int, args.ts.split(",")):
            it = args.iters if T < 1024 else max(5, args.iters // 4)
            x = torch.randn(T, hid, device="cuda").to(torch.bfloat16)
            tw, tid = torch.topk(torch.softmax(torch.randn(T, E, device="cuda", generator=g), -1), topk, dim=-1)
            tw, tid = tw.float().contiguous(), tid.to(torch.int32).contiguous()
            r = {"model": name, "T": T, "E": E, "topk": topk, "hidden": hid, "inter": inter, "activations": fmt,
                 "experts_with_rows": int(torch.unique(tid).numel())}
            variants = {
                "transient": lambda: pk.fp4_moe_native(x, w13, s13, gs13, w2, s2, gs2, tw, tid, kind="nvfp4", activations=fmt, transient=True),
                "resident": lambda: pk.fp4_moe_native(x, i13, None, gs13, i2, None, gs2, tw, tid, kind="nvfp4", activations=fmt),
                "fused": lambda: pk.fp4_moe_fused(x, w13, s13, gs13, w2, s2, gs2, tw, tid, kind="nvfp4"),
            }
            for v, fn in variants.items():                         # one eager call each: what the call itself allocates at its peak
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                fn()
                torch.cuda.synchronize()
                r[v + "_call_peak_bytes"] = torch.cuda.max_memory_allocated() - before
            passes = {v: [] for v in variants}
            for _ in range(2):                                     # a, b, c, a, b, c in one process: both passes reported
                for v, fn in variants.items():
                    passes[v].append(graph_us(fn, it))
            for v in variants:
                r[v + "_us_passes"] = passes[v]
                r[v + "_us"] = sum(passes[v]) / 2
            r["transient_over_resident"] = r["transient_us"] / r["resident_us"]
            r["transient_over_fused"] = r["transient_us"] / r["fused_us"]
            r["weight_bytes"] = {"fused": packed, "resident": packed + images, "transient": packed, "transient_scratch": scratch}
            print(json.dumps(r), file=sys.stderr, flush=True)
            layers.append(r)
        del w13, w2, s13, s2, i13, i2
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_properties(0).gcnArchName, "layers": layers, "builder": builders}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""tools/moe_invariant_bench.py -- what batch invariance costs a MoE layer, and where its two forms cross.

    python tools/moe_invariant_bench.py [--reps 7] [--quick] [--out profiles/moe_invariant_session.json] [--md table.md]

Part 1, the price: fp4_moe_fused(..., invariant=True) against fp4_moe_fused on the same weights and routing, for the expert shapes of
Qwen3-30B-A3B (H 2048, I 768, 128 experts, top-8, NVFP4), DeepSeek-V3 (H 7168, I 2048, 256 experts, top-8, NVFP4) and gpt-oss-120b (H and I
padded to 3072 as petit_kernel.gptoss pads them, 128 experts, top-4, MXFP4, swiglu_oai) at T in {1, 16, 64, 512, 4096}, bf16.  Each side is
captured into a HIP graph of `launches` layer calls, every call with a routing of its own (uniform random distinct experts per token, so that
at small T the calls of a graph touch different experts and the weights do not sit in the Infinity Cache), replayed `reps` times, default first,
then invariant, then both once more; reported per layer call: the median over all replays of a side, its minimum and maximum, the ratio.

Part 2, the forms: one gate_up launch (mul_*_a16_moe_invariant, silu_mul) with m rows spread evenly over the first 8 experts, declared with
num_experts = 8 and with the offsets padded to 128 experts (120 of them empty: the same rows on the same experts, the same bits -- asserted).
The form is a function of (m, num_experts), so the two declarations run different forms wherever the switch separates them, and otherwise
show what 120 dead slots cost.  No call can be forced into a form: profiles/moe_invariant.md has this table from three builds of the
library (the switch at its starting constants, a build that always runs the whole form, and the constants chosen from the two).

The weights are random packed bytes (scale bytes inside the formats' normal range): a timing does not read their values."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "petit-kernel_amd"))
sys.path.insert(0, str(ROOT / "tools"))

import benchlib  # noqa: E402
import petit_kernel as pk  # noqa: E402

MODELS = {   # name: (H, I, E, topk, kind, activation)
    "qwen3-30b-a3b": (2048, 768, 128, 8, "nvfp4", "silu_mul"),
    "deepseek-v3": (7168, 2048, 256, 8, "nvfp4", "silu_mul"),
    "gpt-oss-120b": (3072, 3072, 128, 4, "mxfp4", "swiglu_oai"),
}
TS = (1, 16, 64, 512, 4096)


def packed(kind, E, n, k, dev, gen):
    """Random packed weights and scales of E [n, k] experts, and their global scales."""
    b = torch.randint(0, 256, (E * n * k // 2,), dtype=torch.uint8, device=dev, generator=gen)
    lo, hi, group = (0x30, 0x40, 16) if kind == "nvfp4" else (120, 126, 32)
    s = torch.randint(lo, hi, (E * n * k // group,), dtype=torch.uint8, device=dev, generator=gen)
    return b, s, torch.full((E,), 0.01, dtype=torch.float32, device=dev)


def routing(T, E, topk, dev, gen):
    ids = torch.rand(T, E, device=dev, generator=gen).topk(topk, dim=1).indices.to(torch.int32).contiguous()
    w = torch.softmax(torch.rand(T, topk, device=dev, generator=gen), dim=1).contiguous()
    return w, ids


def one_call_us(launch, stream) -> float:
    with torch.cuda.stream(stream):
        launch(0)
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        launch(1)
        e1.record(stream)
        stream.synchronize()
    return e0.elapsed_time(e1) * 1e3


def time_sides(sides, reps, stream, most=64):
    """{side: launch(i)} -> {side: us-per-call samples}, sides alternating, twice."""
    launches = {s: int(max(2, min(most, 20000.0 / max(one_call_us(fn, stream), 1.0)))) for s, fn in sides.items()}
    samples = {s: [] for s in sides}
    for _ in range(2):
        for side, fn in sides.items():
            samples[side] += benchlib.time_graph(fn, launches[side], reps, stream)
    return samples, launches


def stats(xs, prefix):
    return {prefix + "_us": round(benchlib.median(xs), 2), prefix + "_min_us": round(min(xs), 2), prefix + "_max_us": round(max(xs), 2)}


def price_rows(args, dev, stream, gen):
    rows = []
    models = {"small": (512, 512, 8, 2, "nvfp4", "silu_mul")} if args.quick else MODELS
    for name, (H, I, E, topk, kind, act) in models.items():
        w13, w2 = packed(kind, E, 2 * I, H, dev, gen), packed(kind, E, H, I, dev, gen)
        for T in ((1, 64) if args.quick else TS):
            x = torch.randn(T, H, device=dev, generator=gen).to(torch.bfloat16)
            routes = [routing(T, E, topk, dev, gen) for _ in range(64 if T <= 64 else 4)]

            def layer(invariant):
                def launch(i):
                    w, ids = routes[i % len(routes)]
                    return pk.fp4_moe_fused(x, *w13, *w2, w, ids, kind, activation=act, invariant=invariant)
                return launch
            samples, launches = time_sides({"default": layer(False), "invariant": layer(True)}, args.reps, stream)
            row = {"part": "price", "model": name, "H": H, "I": I, "E": E, "topk": topk, "kind": kind, "T": T, "m": T * topk,
                   "form": "split" if pk.moe_invariant_form(T * topk, E) else "whole",
                   "S13": pk.invariant_geometry(2 * I, H, torch.bfloat16, kind)[0], "S2": pk.invariant_geometry(H, I, torch.bfloat16, kind)[0],
                   **stats(samples["default"], "default"), **stats(samples["invariant"], "invariant"), "launches": launches, "reps": 2 * args.reps}
            row["ratio"] = round(row["invariant_us"] / row["default_us"], 3)
            print(json.dumps(row), flush=True)
            rows.append(row)
        del w13, w2
        torch.cuda.empty_cache()
    return rows


def form_rows(args, dev, stream, gen):
    rows = []
    shapes = {"small": (512, 256, "nvfp4")} if args.quick else {"qwen3 gate_up": (2048, 768, "nvfp4"), "deepseek gate_up": (7168, 2048, "nvfp4")}
    E0, E1 = 8, 128
    for name, (H, I, kind) in shapes.items():
        n, k = 2 * I, H
        b, s, gs = packed(kind, E1, n, k, dev, gen)
        group = 16 if kind == "nvfp4" else 32
        ops_of = {E: (b[:E * n * k // 2], s[:E * n * k // group], gs[:E]) for E in (E0, E1)}   # (the first 8 experts are the same bytes)
        mul = pk.mul_nvfp4_a16_moe_invariant if kind == "nvfp4" else pk.mul_mxfp4_a16_moe_invariant
        for m in ((128, 512) if args.quick else (128, 256, 320, 384, 512, 1024, 2048, 4096)):
            a = torch.randn(m, k, device=dev, generator=gen).to(torch.bfloat16)
            per = m // E0
            off = {E: torch.tensor([min(e, E0) * per for e in range(E + 1)], dtype=torch.int32, device=dev) for E in (E0, E1)}
            outs = {E: mul(a, *ops_of[E], off[E], m, n, k, E, activation="silu_mul") for E in (E0, E1)}
            assert torch.equal(outs[E0].view(torch.int16), outs[E1].view(torch.int16))     # the same bits whatever the form
            sides = {E: (lambda i, E=E: mul(a, *ops_of[E], off[E], m, n, k, E, activation="silu_mul")) for E in (E0, E1)}
            samples, launches = time_sides(sides, args.reps, stream)
            row = {"part": "forms", "shape": name, "n": n, "k": k, "m": m, "rows_per_expert": per,
                   "form_E8": "split" if pk.moe_invariant_form(m, E0) else "whole", "form_E128": "split" if pk.moe_invariant_form(m, E1) else "whole",
                   **stats(samples[E0], "E8"), **stats(samples[E1], "E128"), "launches": {str(e): v for e, v in launches.items()}, "reps": 2 * args.reps}
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def to_markdown(rows) -> str:
    lines = ["| model | format | T | m | form | default us | invariant us | invariant / default | default min..max | invariant min..max |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in (r for r in rows if r["part"] == "price"):
        lines.append(f"| {r['model']} | {r['kind']} | {r['T']} | {r['m']} | {r['form']} | {r['default_us']:.1f} | {r['invariant_us']:.1f} | "
                     f"{r['ratio']:.2f} | {r['default_min_us']:.1f}..{r['default_max_us']:.1f} | "
                     f"{r['invariant_min_us']:.1f}..{r['invariant_max_us']:.1f} |")
    lines += ["", "| launch | m | rows / expert | declared E = 8: form, us (min..max) | declared E = 128: form, us (min..max) |", "|---|---|---|---|---|"]
    for r in (r for r in rows if r["part"] == "forms"):
        lines.append(f"| {r['shape']} {r['n']}x{r['k']} | {r['m']} | {r['rows_per_expert']} | {r['form_E8']} {r['E8_us']:.1f} "
                     f"({r['E8_min_us']:.1f}..{r['E8_max_us']:.1f}) | {r['form_E128']} {r['E128_us']:.1f} "
                     f"({r['E128_min_us']:.1f}..{r['E128_max_us']:.1f}) |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="one small shape: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default="")
    ap.add_argument("--md", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to report without one"
    dev = torch.device("cuda")
    stream = torch.cuda.Stream()
    gen = torch.Generator(device=dev).manual_seed(2024)
    rows = price_rows(args, dev, stream, gen) + form_rows(args, dev, stream, gen)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rows, indent=1) + "\n")
    if args.md:
        Path(args.md).write_text(to_markdown(rows))


if __name__ == "__main__":
    main()

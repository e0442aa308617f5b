#!/usr/bin/env python3
"""tools/native_moe_invariant_bench.py -- what batch invariance costs a MoE layer on the native class, and where its two forms cross.

    python tools/native_moe_invariant_bench.py [--reps 7] [--quick] [--out profiles/native_moe_invariant_session.json] [--md table.md]
    PETIT_AMD_LIB=<measurement build> PETIT_AMD_BINDING=ctypes python tools/native_moe_invariant_bench.py --forms [--out forms.json] [--md forms.md]

Part 1, the price: fp4_moe_native(..., invariant=True) against fp4_moe_native (the native default: the pick that moves with the batch) and
against fp4_moe_fused(..., invariant=True) (the exact class's batch-invariant layer) on the same weights and routing, bf16, MXFP4 experts of the
shapes of gpt-oss-120b (H and I padded to 3072 as petit_kernel.gptoss pads them, 128 experts, top-4, swiglu_oai) and Qwen3-30B-A3B (H 2048,
I 768, 128 experts, top-8, silu_mul), activations MXFP8 / MXFP6 / MXFP4, T in {1, 16, 64, 512, 4096}.  Each side is captured into a HIP graph
of up to 64 layer calls, every call with a routing of its own (uniform random distinct experts per token, so that at small T the calls of a
graph touch different experts and the weights do not sit in the Infinity Cache), replayed `reps` times, the sides in turn, then all once more
(14 replays a side with the default --reps 7); reported per layer call: the median over all replays of a side, its minimum and maximum.

--forms, the form switch.  No call can be forced into a form, so the two forms are timed through a measurement-only build of the library
(csrc/gemm_invariant_api.hip compiled with -DPETIT_NATIVE_MOE_INV_MEASURE_FORMS=1 and linked with the other objects), which reads the
switch's two constants from $PETIT_NATIVE_MOE_INV_SPLIT_ROWS_PER / $PETIT_NATIVE_MOE_INV_SPLIT_MAX_M per call.  Three settings stand for the
three builds of profiles/moe_invariant.md: the starting constants (8, 8), always-whole (0, 0) and a candidate (--rows-per, --max-m); the layer
is timed under each at T in {1, 2, 4, 8, 16, 32, 64, 128} -- the range in which the answer can change.  The same bits under every setting,
asserted.

--nvfp4: NVFP4 experts on their native images.  Part 1 times the layer composed from the two petit_gemm_nvfp4_native_moe_invariant launches
(align, gathering quantiser, gate_up, down, combine: examples/nvfp4_native_invariant.py) against fp4_moe_native(kind="nvfp4") on the same images
and fp4_moe_fused(kind="nvfp4", invariant=True) on the packed tensors the images were built from, on the expert shapes of Qwen3-30B-A3B and
DeepSeek-V3 (H 7168, I 2048, 256 experts, top-8, silu_mul).  With --forms it times the two LAUNCHES (gate_up on 16-bit grouped rows, then down)
in the split and in the whole form at 4, 8, 16 and 32 grouped rows, every row on an expert drawn at random: (2^20, 2^20) against (0, 0).

The weights are random packed bytes (scale bytes inside the format's normal range): a timing does not read their values."""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "petit-kernel_amd"))
sys.path.insert(0, str(ROOT / "tools"))

import benchlib  # noqa: E402
import petit_kernel as pk  # noqa: E402

MODELS = {   # name: (H, I, E, topk, activation)
    "gpt-oss-120b": (3072, 3072, 128, 4, "swiglu_oai"),
    "qwen3-30b-a3b": (2048, 768, 128, 8, "silu_mul"),
}
NV_MODELS = {
    "qwen3-30b-a3b": (2048, 768, 128, 8, "silu_mul"),
    "deepseek-v3": (7168, 2048, 256, 8, "silu_mul"),
}
NV_FORM_ROWS = (4, 8, 16, 32)
TS = (1, 16, 64, 512, 4096)
FORM_TS = (1, 2, 4, 8, 16, 32, 64, 128)
FMTS = ("mxfp8", "mxfp6", "mxfp4")


def packed(E, n, k, dev, gen):
    """Random packed MXFP4 weights and scales of E [n, k] experts, and their global scales."""
    b = torch.randint(0, 256, (E * n * k // 2,), dtype=torch.uint8, device=dev, generator=gen)
    s = torch.randint(120, 126, (E * n * k // 32,), dtype=torch.uint8, device=dev, generator=gen)
    return b, s, torch.full((E,), 0.01, dtype=torch.float32, device=dev)


def packed_nv(E, n, k, dev, gen):
    """Random packed NVFP4 weights and e4m3 scales (0.25 .. 3.75) of E [n, k] experts, their global scales, and their native images."""
    b = torch.randint(0, 256, (E * n * k // 2,), dtype=torch.uint8, device=dev, generator=gen)
    s = (torch.rand(E * n * k // 16, device=dev, generator=gen) * 3.5 + 0.25).to(torch.float8_e4m3fn).view(torch.uint8)
    return b, s, torch.full((E,), 0.01, dtype=torch.float32, device=dev), pk.nvfp4_native_images(b, s, E, n, k)


def nv_invariant_layer(x, images13, gs13, images2, gs2, w, ids, fmt, act, E, H, I):
    """the batch-invariant layer on images, composed as fp4_moe_native(invariant=True) composes it for MXFP4 experts"""
    m = x.shape[0] * ids.shape[1]
    sorted_pos, offsets, token_index = pk.moe_align_device(ids, E)
    qa = pk.quantize_activation_rows(x, fmt, token_index)
    h = pk.mul_nvfp4_native_moe_invariant(qa, images13, gs13, offsets, m, 2 * I, H, E, fmt=fmt, activation=act)
    y = pk.mul_nvfp4_native_moe_invariant(h, images2, gs2, offsets, m, H, I, E, c_row_index=sorted_pos, c_rows=m, fmt=fmt)
    return pk.moe_combine(y, w, ids, E)


def nv_price_rows(args, dev, stream, gen):
    rows = []
    models = {"small": (512, 512, 8, 2, "silu_mul")} if args.quick else NV_MODELS
    for name, (H, I, E, topk, act) in models.items():
        b13, s13, gs13, im13 = packed_nv(E, 2 * I, H, dev, gen)
        b2, s2, gs2, im2 = packed_nv(E, H, I, dev, gen)
        for T in ((1, 64) if args.quick else TS):
            x = torch.randn(T, H, device=dev, generator=gen).to(torch.bfloat16)
            routes = [routing(T, E, topk, dev, gen) for _ in range(64 if T <= 64 else 4)]
            exact = None
            for fmt in FMTS:
                def invariant(i, fmt=fmt):
                    w, ids = routes[i % len(routes)]
                    return nv_invariant_layer(x, im13, gs13, im2, gs2, w, ids, fmt, act, E, H, I)

                def native(i, fmt=fmt):
                    w, ids = routes[i % len(routes)]
                    return pk.fp4_moe_native(x, im13, None, gs13, im2, None, gs2, w, ids, "nvfp4", fmt, activation=act)

                def fused(i):
                    w, ids = routes[i % len(routes)]
                    return pk.fp4_moe_fused(x, b13, s13, gs13, b2, s2, gs2, w, ids, "nvfp4", activation=act, invariant=True)
                sides = {"native": native, "invariant": invariant}
                if exact is None:                                                     # (the exact layer does not read the activation format)
                    sides["exact_invariant"] = fused
                samples, launches = time_sides(sides, args.reps, stream)
                exact = exact or (stats(samples["exact_invariant"], "exact_invariant"), launches["exact_invariant"])
                launches["exact_invariant"] = exact[1]
                row = {"part": "price", "model": name + " nvfp4", "H": H, "I": I, "E": E, "topk": topk, "activations": fmt, "T": T, "m": T * topk,
                       "form": "split" if pk.native_moe_invariant_form(T * topk, E) else "whole",
                       "S13": pk.invariant_geometry(2 * I, H, torch.bfloat16, "nvfp4")[0], "S2": pk.invariant_geometry(H, I, torch.bfloat16, "nvfp4")[0],
                       **stats(samples["native"], "native"), **stats(samples["invariant"], "invariant"), **exact[0], "launches": launches,
                       "reps": 2 * args.reps}
                row["vs_native"] = round(row["invariant_us"] / row["native_us"], 3)
                row["vs_exact_invariant"] = round(row["invariant_us"] / row["exact_invariant_us"], 3)
                print(json.dumps(row), flush=True)
                rows.append(row)
        del b13, s13, im13, b2, s2, im2
        torch.cuda.empty_cache()
    return rows


def nv_form_rows(args, dev, stream, gen):
    """The two launches on images in each form (the library must read the settings: checked through the form query)."""
    settings = {"split": (1 << 20, 1 << 20), "whole": (0, 0)}

    def use(name):
        os.environ["PETIT_NATIVE_MOE_INV_SPLIT_ROWS_PER"], os.environ["PETIT_NATIVE_MOE_INV_SPLIT_MAX_M"] = (str(v) for v in settings[name])

    use("whole")
    assert pk.native_moe_invariant_form(4, 128) == 0, "--forms needs the measurement build of the library (see the module's text)"
    use("split")
    assert pk.native_moe_invariant_form(32, 128) == 1, "--forms needs the measurement build of the library (see the module's text)"
    rows = []
    models = {"small": (512, 512, 8, 2, "silu_mul")} if args.quick else NV_MODELS
    for name, (H, I, E, topk, act) in models.items():
        _, _, gs13, im13 = packed_nv(E, 2 * I, H, dev, gen)
        _, _, gs2, im2 = packed_nv(E, H, I, dev, gen)
        for m in NV_FORM_ROWS:
            x = torch.randn(m, H, device=dev, generator=gen).to(torch.bfloat16)
            offs = []
            for _ in range(64):                                                       # every grouped row on an expert drawn at random
                counts = torch.bincount(torch.randint(0, E, (m,), device=dev, generator=gen), minlength=E)
                offs.append(torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), counts.cumsum(0)]).to(torch.int32).contiguous())
            for fmt in FMTS:
                def launches_of(setting, fmt=fmt):
                    def launch(i):
                        use(setting)                                                  # (read by the library at capture, per call)
                        off = offs[i % len(offs)]
                        h = pk.ops.mul_nvfp4_native_moe_invariant(x, im13, gs13, off, m, 2 * I, H, E, fmt=fmt, activation=act)
                        return pk.ops.mul_nvfp4_native_moe_invariant(h, im2, gs2, off, m, H, I, E, fmt=fmt)
                    return launch
                outs = {s: launches_of(s)(0) for s in settings}
                assert torch.equal(outs["split"].view(torch.int16), outs["whole"].view(torch.int16))       # the same bits in either form
                samples, launches = time_sides({s: launches_of(s) for s in settings}, args.reps, stream)
                row = {"part": "nv_forms", "model": name + " nvfp4", "activations": fmt, "m": m, "launches": launches, "reps": 2 * args.reps,
                       **stats(samples["split"], "split"), **stats(samples["whole"], "whole")}
                row["split_over_whole"] = round(row["split_us"] / row["whole_us"], 3)
                print(json.dumps(row), flush=True)
                rows.append(row)
        del im13, im2
        torch.cuda.empty_cache()
    return rows


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
    models = {"small": (512, 512, 8, 2, "silu_mul")} if args.quick else MODELS
    for name, (H, I, E, topk, act) in models.items():
        w13, w2 = packed(E, 2 * I, H, dev, gen), packed(E, H, I, dev, gen)
        for T in ((1, 64) if args.quick else TS):
            x = torch.randn(T, H, device=dev, generator=gen).to(torch.bfloat16)
            routes = [routing(T, E, topk, dev, gen) for _ in range(64 if T <= 64 else 4)]
            exact = None
            for fmt in FMTS:
                def native(invariant, fmt=fmt):
                    def launch(i):
                        w, ids = routes[i % len(routes)]
                        return pk.fp4_moe_native(x, *w13, *w2, w, ids, "mxfp4", fmt, activation=act, invariant=invariant)
                    return launch

                def fused(i):
                    w, ids = routes[i % len(routes)]
                    return pk.fp4_moe_fused(x, *w13, *w2, w, ids, "mxfp4", activation=act, invariant=True)
                sides = {"native": native(False), "invariant": native(True)}
                if exact is None:                                                     # (the exact layer does not read the activation format)
                    sides["exact_invariant"] = fused
                samples, launches = time_sides(sides, args.reps, stream)
                exact = exact or (stats(samples["exact_invariant"], "exact_invariant"), launches["exact_invariant"])
                launches["exact_invariant"] = exact[1]
                row = {"part": "price", "model": name, "H": H, "I": I, "E": E, "topk": topk, "activations": fmt, "T": T, "m": T * topk,
                       "form": "split" if pk.native_moe_invariant_form(T * topk, E) else "whole",
                       "S13": pk.invariant_geometry(2 * I, H, torch.bfloat16, "mxfp4")[0], "S2": pk.invariant_geometry(H, I, torch.bfloat16, "mxfp4")[0],
                       **stats(samples["native"], "native"), **stats(samples["invariant"], "invariant"), **exact[0], "launches": launches,
                       "reps": 2 * args.reps}
                row["vs_native"] = round(row["invariant_us"] / row["native_us"], 3)
                row["vs_exact_invariant"] = round(row["invariant_us"] / row["exact_invariant_us"], 3)
                print(json.dumps(row), flush=True)
                rows.append(row)
        del w13, w2
        torch.cuda.empty_cache()
    return rows


def form_rows(args, dev, stream, gen):
    """The layer under the three settings of the measurement build (the library must read them: checked through the form query)."""
    settings = {"start": (8, 8), "whole": (0, 0), "candidate": (args.rows_per, args.max_m)}

    def use(name):
        os.environ["PETIT_NATIVE_MOE_INV_SPLIT_ROWS_PER"], os.environ["PETIT_NATIVE_MOE_INV_SPLIT_MAX_M"] = (str(v) for v in settings[name])

    use("whole")
    assert pk.native_moe_invariant_form(4, 128) == 0, "--forms needs the measurement build of the library (see the module's text)"
    rows = []
    models = {"small": (512, 512, 8, 2, "silu_mul")} if args.quick else MODELS
    for name, (H, I, E, topk, act) in models.items():
        w13, w2 = packed(E, 2 * I, H, dev, gen), packed(E, H, I, dev, gen)
        for T in ((1, 16) if args.quick else FORM_TS):
            x = torch.randn(T, H, device=dev, generator=gen).to(torch.bfloat16)
            routes = [routing(T, E, topk, dev, gen) for _ in range(64)]
            for fmt in FMTS:
                def layer(setting, fmt=fmt):
                    def launch(i):
                        use(setting)                                                  # (read by the library at capture, per call)
                        w, ids = routes[i % len(routes)]
                        return pk.fp4_moe_native(x, *w13, *w2, w, ids, "mxfp4", fmt, activation=act, invariant=True)
                    return launch
                outs = {s: layer(s)(0) for s in settings}
                assert all(torch.equal(o.view(torch.int16), outs["start"].view(torch.int16)) for o in outs.values())   # the same bits whatever the form
                samples, launches = time_sides({s: layer(s) for s in settings}, args.reps, stream)
                row = {"part": "forms", "model": name, "activations": fmt, "T": T, "m": T * topk, "settings": {s: list(v) for s, v in settings.items()},
                       "launches": launches, "reps": 2 * args.reps}
                for s in settings:
                    use(s)
                    row["form_" + s] = "split" if pk.native_moe_invariant_form(T * topk, E) else "whole"
                    row.update(stats(samples[s], s))
                print(json.dumps(row), flush=True)
                rows.append(row)
        del w13, w2
        torch.cuda.empty_cache()
    return rows


def to_markdown(rows) -> str:
    lines = []
    price = [r for r in rows if r["part"] == "price"]
    if price:
        lines += ["| model | activations | T | m | form | native default us (min..max) | invariant us (min..max) | exact invariant us (min..max) | "
                  "invariant / native | invariant / exact invariant |", "|---|---|---|---|---|---|---|---|---|---|"]
        for r in price:
            lines.append(f"| {r['model']} | {r['activations']} | {r['T']} | {r['m']} | {r['form']} | {r['native_us']:.1f} ({r['native_min_us']:.1f}.."
                         f"{r['native_max_us']:.1f}) | {r['invariant_us']:.1f} ({r['invariant_min_us']:.1f}..{r['invariant_max_us']:.1f}) | "
                         f"{r['exact_invariant_us']:.1f} ({r['exact_invariant_min_us']:.1f}..{r['exact_invariant_max_us']:.1f}) | "
                         f"{r['vs_native']:.2f} | {r['vs_exact_invariant']:.2f} |")
    nv_forms = [r for r in rows if r["part"] == "nv_forms"]
    if nv_forms:
        lines += ["| model | activations | grouped rows | split us (min..max) | whole us (min..max) | split / whole |", "|---|---|---|---|---|---|"]
        for r in nv_forms:
            lines.append(f"| {r['model']} | {r['activations']} | {r['m']} | {r['split_us']:.1f} ({r['split_min_us']:.1f}..{r['split_max_us']:.1f}) | "
                         f"{r['whole_us']:.1f} ({r['whole_min_us']:.1f}..{r['whole_max_us']:.1f}) | {r['split_over_whole']:.2f} |")
    forms = [r for r in rows if r["part"] == "forms"]
    for s in (forms[0]["settings"] if forms else ()):
        a, b = forms[0]["settings"][s]
        lines += ["", f"Setting `{s}` (rows per expert <= {a} and m <= {b}):", "", "| model | T | m | form | mxfp8 us (min..max) | mxfp6 us (min..max) | mxfp4 us (min..max) |",
                  "|---|---|---|---|---|---|---|"]
        for model in dict.fromkeys(r["model"] for r in forms):
            for T in dict.fromkeys(r["T"] for r in forms):
                cell = {r["activations"]: r for r in forms if r["model"] == model and r["T"] == T}
                any_r = next(iter(cell.values()))
                cols = " | ".join(f"{cell[f][s + '_us']:.1f} ({cell[f][s + '_min_us']:.1f}..{cell[f][s + '_max_us']:.1f})" for f in FMTS)
                lines.append(f"| {model} | {T} | {any_r['m']} | {any_r['form_' + s]} | {cols} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="one small shape: a rehearsal of the script, not a measurement")
    ap.add_argument("--forms", action="store_true", help="time the layer under the three form settings (needs the measurement build)")
    ap.add_argument("--rows-per", type=int, default=8, help="--forms: the candidate's rows-per-expert constant")
    ap.add_argument("--max-m", type=int, default=8, help="--forms: the candidate's m constant")
    ap.add_argument("--nvfp4", action="store_true", help="NVFP4 experts on their native images (see the module's text)")
    ap.add_argument("--out", default="")
    ap.add_argument("--md", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to report without one"
    dev = torch.device("cuda")
    stream = torch.cuda.Stream()
    gen = torch.Generator(device=dev).manual_seed(2025)
    if args.nvfp4:
        rows = nv_form_rows(args, dev, stream, gen) if args.forms else nv_price_rows(args, dev, stream, gen)
    else:
        rows = form_rows(args, dev, stream, gen) if args.forms else price_rows(args, dev, stream, gen)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rows, indent=1) + "\n")
    if args.md:
        Path(args.md).write_text(to_markdown(rows))


if __name__ == "__main__":
    main()

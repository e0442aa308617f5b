#!/usr/bin/env python3
"""tools/native_moe_decode_bench.py -- the routed-expert decode GEMM on the native images (petit_gemm_nvfp4_native_moe_decode) and the
fp4_moe_native(decode=True) layer against the paths there were on the same images: mul_nvfp4_native_moe with its quantiser launch, and
fp4_moe_native; and against the stream floor of the ACTIVE experts' image bytes, 1.8 us + bytes / 6.5 TB/s.

    python tools/native_moe_decode_bench.py [--reps 5] [--ts 1,4,16,32] [--models qwen3-30b-a3b,deepseek-v3,gpt-oss-120b] [--quick]
                                            [--out profiles/native_moe_decode.json] [--md profiles/native_moe_decode.md]

The expert shapes of tools/moe_invariant_bench.py (Qwen3-30B-A3B, DeepSeek-V3, gpt-oss-120b), bf16 hidden states, MXFP8 activations.  The
gpt-oss cells run their decode sides with global_scales=None, as MXFP6 images do; the others with NVFP4's global scales.  Images are random
bytes: a timing does not read their values.  Method: moe_invariant_bench.time_sides -- every side captured into a HIP graph of calls with a
routing each (uniform random distinct experts per token, 64 routings, so that the calls of a graph touch different experts), sides in turn,
then all once more; median per call.  The GEMM cells are timed after the align (its outputs precomputed per routing); the layer cells
include it."""
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
from moe_invariant_bench import MODELS, routing, time_sides  # noqa: E402
from petit_kernel import _lib  # noqa: E402

FMT, SID = "mxfp8", pk.SOLUTION_AUTO_NATIVE_MXFP8


def images_of(E, n, k, dev, gen):
    """E random native images of [n, k] back to back (E8M0 bytes near 1.0), and their global scales"""
    per, elem = int(_lib.lib.petit_nvfp4_native_image_bytes(k, n)), n * k * 3 // 4   # 6 bits per weight, then a byte per 32
    img = torch.randint(0, 256, (E, per), dtype=torch.uint8, device=dev, generator=gen)
    img[:, elem:] = torch.randint(120, 126, (E, per - elem), dtype=torch.uint8, device=dev, generator=gen)
    return img.reshape(-1), torch.full((E,), 0.01, dtype=torch.float32, device=dev), per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ts", default="1,4,16,32")
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--quick", action="store_true", help="one small shape: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default="")
    ap.add_argument("--md", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to report without one"
    dev, stream = torch.device("cuda"), torch.cuda.Stream()
    gen = torch.Generator(device=dev).manual_seed(2025)
    models = {"small": (512, 512, 8, 2, "nvfp4", "silu_mul")} if args.quick else {m: MODELS[m] for m in args.models.split(",")}
    rows = []
    for name, (H, I, E, topk, kind, act) in models.items():
        w13, gs13, per13 = images_of(E, 2 * I, H, dev, gen)
        w2, gs2, per2 = images_of(E, H, I, dev, gen)
        dgs13, dgs2 = (None, None) if kind == "mxfp4" else (gs13, gs2)          # the decode sides of an MXFP6-like model: no global scales
        for T in map(int, args.ts.split(",")):
            m = T * topk
            x = torch.randn(T, H, device=dev, generator=gen).to(torch.bfloat16)
            h = torch.randn(m, I, device=dev, generator=gen).to(torch.bfloat16)
            routes = [routing(T, E, topk, dev, gen) for _ in range(64)]
            aligned = [pk.moe_align_device(ids, E) for _, ids in routes]        # (sorted_pos, offsets, token_index)
            active = sum(len(torch.unique(ids)) for _, ids in routes) / len(routes)

            def gate_up(decode):
                def launch(i):
                    pos, off, tok = aligned[i % 64]
                    if decode:
                        return pk.mul_nvfp4_native_moe_decode(x, w13, dgs13, off, m, 2 * I, H, E, a_row_index=tok, fmt=FMT, activation=act)
                    qa = pk.quantize_activation_rows(x, FMT, tok)
                    return pk.mul_nvfp4_native_moe(qa, w13, gs13, off, m, 2 * I, H, E, solution_id=SID, activation=act)
                return launch

            def down(decode):
                def launch(i):
                    pos, off, tok = aligned[i % 64]
                    if decode:
                        return pk.mul_nvfp4_native_moe_decode(h, w2, dgs2, off, m, H, I, E, c_row_index=pos, c_rows=m, fmt=FMT)
                    return pk.mul_nvfp4_native_moe(h, w2, gs2, off, m, H, I, E, solution_id=SID, c_row_index=pos, c_rows=m)
                return launch

            def layer(decode):
                def launch(i):
                    w, ids = routes[i % 64]
                    return pk.fp4_moe_native(x, w13, None, gs13, w2, None, gs2, w, ids, "nvfp4", FMT, activation=act, decode=decode)
                return launch
            cells = {"gate_up": (gate_up, active * per13), "down": (down, active * per2), "layer": (layer, active * (per13 + per2))}
            for cell, (make, stream_bytes) in cells.items():
                samples, launches = time_sides({"decode": make(True), "parent": make(False)}, args.reps, stream)
                row = {"model": name, "H": H, "I": I, "E": E, "topk": topk, "T": T, "m": m, "cell": cell, "fmt": FMT,
                       "global_scales": dgs13 is not None or cell == "layer", "active_experts": round(active, 1),
                       "floor_us": round(1.8 + stream_bytes / 6.5e6, 2), "launches": launches, "reps": 2 * args.reps}
                for side, xs in samples.items():
                    row.update({side + "_us": round(benchlib.median(xs), 2), side + "_min_us": round(min(xs), 2), side + "_max_us": round(max(xs), 2)})
                row["decode_over_parent"] = round(row["decode_us"] / row["parent_us"], 3)
                row["decode_over_floor"] = round(row["decode_us"] / row["floor_us"], 2)
                print(json.dumps(row), flush=True)
                rows.append(row)
        del w13, w2
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rows, indent=1) + "\n")
    if args.md:
        lines = ["| model | cell | T | m | active experts | floor us | decode us (min..max) | parent us (min..max) | decode / parent | decode / floor |",
                 "|---|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            lines.append(f"| {r['model']} | {r['cell']}{'' if r['global_scales'] else ' (no gs)'} | {r['T']} | {r['m']} | {r['active_experts']} | "
                         f"{r['floor_us']:.1f} | {r['decode_us']:.1f} ({r['decode_min_us']:.1f}..{r['decode_max_us']:.1f}) | "
                         f"{r['parent_us']:.1f} ({r['parent_min_us']:.1f}..{r['parent_max_us']:.1f}) | {r['decode_over_parent']:.2f} | "
                         f"{r['decode_over_floor']:.2f} |")
        Path(args.md).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""tools/native_decode_bench.py -- the decode GEMM on the native image (petit_gemm_nvfp4_native_decode) against the only path there was on the
same image, petit_gemm_nvfp4_native's default pick (petit_gemm_fp4_fp16_grid_ws with the matching sentinel on the attached image, quantiser
launch included), and against the stream floor of DESIGN.md section 3.1, 1.8 us + image bytes / 6.5 TB/s.  ONE session, same operands.

    python tools/native_decode_bench.py [--reps 5] [--ms 1,4,16,32] [--fmts mxfp8,mxfp6,mxfp4] [--parts 0,1,2,4] [--quick]
                                        [--out profiles/native_decode.json] [--md profiles/native_decode.md]

The four Llama-3-70B linears, bf16.  Sides per cell: `decode16 P=p` (16-bit input, quantised in the kernel's registers) for every p of
--parts (0: the library's rule, the others feed that rule), `decodeq` (QuantizedActivations input, the library's P, the quantiser NOT
counted: a fused norm wrote them) and `default` (the parent's path).  Method: tools/native_invariant_bench.py's -- every side captured into
HIP graphs over rotating weight copies beyond the 256 MB Infinity Cache, all sides in turn, then all once more; median per launch."""
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

import benchlib  # noqa: E402
from native_invariant_bench import FMTS, SHAPES, time_sides  # noqa: E402
from petit_kernel import _lib  # noqa: E402

L = _lib.lib


def decode_launcher(g: benchlib.Gemm, code: int, parts: int, quantized: bool):
    m, n, k = g.m, g.w.n, g.w.k
    g.w.attach_native()
    images = g.w.images
    need = int(L.petit_gemm_nvfp4_native_decode_workspace_bytes(m, n, k, parts))
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=g.dev)
    a = g.a
    if quantized:
        a = torch.empty(int(L.petit_quantized_activation_bytes(m, k, code)), dtype=torch.uint8, device=g.dev)
        assert L.petit_quantize_activations(C.c_void_p(a.data_ptr()), C.c_void_p(g.a.data_ptr()), m, k, g.a_type, code, None) == 0
        torch.cuda.synchronize()

    def launch(i, _keep=(ws, a)):
        rc = L.petit_gemm_nvfp4_native_decode(C.c_void_p(g.c.data_ptr()), C.c_void_p(a.data_ptr()), C.c_void_p(images[i % len(images)].data_ptr()),
                                              C.c_void_p(g.gs.data_ptr()), m, n, k, C.byref(g.hints), code, int(quantized), None, parts,
                                              C.c_void_p(ws.data_ptr()), need, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise RuntimeError(f"rc={rc} ({_lib.error_string(rc)})")
    return launch


def markdown(rows) -> str:
    sides = sorted({s for r in rows for s in r["sides"]})
    head = ["shape", "fmt", "M", "auto P", "floor us"] + [f"{s} us" for s in sides] + ["decode16 P=0 / default", "decode16 P=0 / floor"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for r in rows:
        t = r["sides"]
        new = t["decode16 P=0"]["us"]
        cell = [f"{r['shape']} {r['N']}x{r['K']}", r["fmt"], str(r["M"]), str(r["auto_parts"]), f"{r['floor_us']:.1f}"]
        cell += [f"{t[s]['us']:.1f}" if s in t else "-" for s in sides]
        cell += [f"{new / t['default']['us']:.2f}" if "default" in t else "-", f"{new / r['floor_us']:.2f}"]
        lines.append("| " + " | ".join(cell) + " |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ms", default="1,4,16,32")
    ap.add_argument("--fmts", default="mxfp8,mxfp6,mxfp4")
    ap.add_argument("--parts", default="0,1,2,4")
    ap.add_argument("--quick", action="store_true", help="one small shape: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default="")
    ap.add_argument("--md", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to report without one"
    dev, stream = torch.device("cuda"), torch.cuda.Stream()
    rows = []
    for name, (n, k) in ({"small": (1024, 1024)} if args.quick else SHAPES).items():
        weights = benchlib.Weights("nv", n, k, 64 if args.quick else 1280, dev)
        image_bytes = int(L.petit_nvfp4_native_image_bytes(k, n))
        for m in map(int, args.ms.split(",")):
            g = benchlib.Gemm(weights, m, torch.bfloat16, dev)
            for f in args.fmts.split(","):
                code, sentinel = FMTS[f]
                sides = {f"decode16 P={p}": decode_launcher(g, code, p, False) for p in map(int, args.parts.split(","))}
                sides["decodeq"] = decode_launcher(g, code, 0, True)
                fn = g.launcher(sentinel)
                try:
                    fn(0)
                    sides["default"] = fn
                except RuntimeError as exc:                               # a cell the native default refuses is reported as missing, not guessed
                    print(f"# native default {f} at {name} M={m}: {exc}", flush=True)
                row = {"shape": name, "N": n, "K": k, "M": m, "fmt": f, "auto_parts": int(L.petit_gemm_nvfp4_native_decode_parts(n, k)),
                       "image_bytes": image_bytes, "floor_us": round(1.8 + image_bytes / 6.5e6, 2),
                       "sides": time_sides(sides, args.reps, stream), "reps": 2 * args.reps}
                print(json.dumps(row), flush=True)
                rows.append(row)
            del g
        del weights
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rows, indent=1) + "\n")
    if args.md:
        Path(args.md).write_text(markdown(rows))


if __name__ == "__main__":
    main()

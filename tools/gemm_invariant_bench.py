#!/usr/bin/env python3
"""tools/gemm_invariant_bench.py -- what batch invariance costs: the batch-invariant entry (petit_gemm_*_fp16_invariant) against the default
pick (solution_id = -1) of the same library, same operands.

    python tools/gemm_invariant_bench.py [--reps 7] [--quick] [--out profiles/gemm_invariant_session.json] [--md table.md]

The four Llama-3-70B linears (qkv 10240 x 8192, o 8192 x 8192, gate_up 57344 x 8192, down 8192 x 28672) at M in {1, 16, 64, 512, 4096},
bf16 x NVFP4 and bf16 x MXFP4.  Both sides go through the C ABI with a per-problem workspace and are captured into HIP graphs of `launches`
calls over rotating weight copies (together beyond the 256 MB Infinity Cache; tools/benchlib.py Weights), replayed `reps` times each, default
first, then invariant, then both once more; reported per launch: the median over all replays of a side, its minimum and maximum, the ratio of
the medians, and the (S, L) and form of the invariant call."""
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
from petit_kernel import _lib  # noqa: E402

SHAPES = {"qkv": (10240, 8192), "o": (8192, 8192), "gate_up": (57344, 8192), "down": (8192, 28672)}
MS = (1, 16, 64, 512, 4096)
FMTS = ("nv", "mx")


def invariant_launcher(g: benchlib.Gemm):
    """launch(i) of the batch-invariant entry on Gemm's operands, and (S, L, slabs) of the call."""
    m, n, k = g.m, g.w.n, g.w.k
    S, L = C.c_uint(0), C.c_uint(0)
    _lib.lib.petit_gemm_invariant_geometry(n, k, g.a_type, g.b_type, C.byref(S), C.byref(L))
    slabs = int(_lib.lib.petit_gemm_invariant_slabs(m, n, k, g.a_type, g.b_type))
    need = int(_lib.lib.petit_gemm_invariant_workspace_bytes(m, n, k, g.a_type, g.b_type))
    ws = torch.empty(need, dtype=torch.uint8, device=g.dev) if need else None
    wsp = C.c_void_p(ws.data_ptr()) if ws is not None else None
    fn = _lib.lib.petit_gemm_fp4_fp16_invariant if g.w.fmt == "nv" else _lib.lib.petit_gemm_mxfp4_fp16_invariant

    def launch(i, _keep=ws):
        b, sp = g.w[i]
        rc = fn(C.c_void_p(g.c.data_ptr()), C.c_void_p(g.a.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(sp.data_ptr()),
                C.c_void_p(g.gs.data_ptr()), m, n, k, C.byref(g.hints), None, wsp, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise RuntimeError(f"rc={rc} ({_lib.error_string(rc)})")
    return launch, S.value, L.value, slabs


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


def to_markdown(rows) -> str:
    lines = ["| shape | format | M | S | L | form | default us | invariant us | invariant / default | default min..max | invariant min..max |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['shape']} {r['N']}x{r['K']} | {r['fmt']} | {r['M']} | {r['S']} | {r['L']} | {r['form']} | {r['default_us']:.1f} | "
                     f"{r['invariant_us']:.1f} | {r['ratio']:.2f} | {r['default_min_us']:.1f}..{r['default_max_us']:.1f} | "
                     f"{r['invariant_min_us']:.1f}..{r['invariant_max_us']:.1f} |")
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
    shapes = {"small": (1024, 1024)} if args.quick else SHAPES
    rows = []
    for name, (n, k) in shapes.items():
        for fmt in FMTS:
            weights = benchlib.Weights(fmt, n, k, 64 if args.quick else 1280, dev)
            for m in ((1, 64) if args.quick else MS):
                g = benchlib.Gemm(weights, m, torch.bfloat16, dev)
                sides = {"default": g.launcher(_lib.PETIT_SOLUTION_AUTO)}
                sides["invariant"], S, L, slabs = invariant_launcher(g)
                samples = {"default": [], "invariant": []}
                launches = {s: int(max(4, min(200, 20000.0 / max(one_call_us(fn, stream), 1.0)))) for s, fn in sides.items()}
                for _ in range(2):                                                     # default, invariant, default, invariant
                    for side, fn in sides.items():
                        samples[side] += benchlib.time_graph(fn, launches[side], args.reps, stream)
                d, v = samples["default"], samples["invariant"]
                row = {"shape": name, "N": n, "K": k, "fmt": fmt, "M": m, "S": S, "L": L, "slabs": slabs,
                       "form": "split" if _lib.lib.petit_gemm_invariant_workspace_bytes(m, n, k, g.a_type, g.b_type) else "whole",
                       "default_us": round(benchlib.median(d), 2), "default_min_us": round(min(d), 2), "default_max_us": round(max(d), 2),
                       "invariant_us": round(benchlib.median(v), 2), "invariant_min_us": round(min(v), 2), "invariant_max_us": round(max(v), 2),
                       "launches": launches, "reps": 2 * args.reps, "default_id": hex(g.resolve(_lib.PETIT_SOLUTION_AUTO))}
                row["ratio"] = round(row["invariant_us"] / row["default_us"], 3)
                print(json.dumps(row), flush=True)
                rows.append(row)
                del g, sides
            del weights
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rows, indent=1) + "\n")
    if args.md:
        Path(args.md).write_text(to_markdown(rows))


if __name__ == "__main__":
    main()

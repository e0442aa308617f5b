#!/usr/bin/env python3
"""tools/native_invariant_bench.py -- what batch invariance costs on the native class, and whether it beats the exact invariant entry: in ONE
session, same operands,
    the new entry    petit_gemm_mxfp4_native_invariant on the 16-bit activations (its quantiser launch included), MXFP8 / MXFP6 / MXFP4;
    exact invariant  petit_gemm_mxfp4_fp16_invariant;
    native default   petit_gemm_mxfp4_fp16_grid_ws with the matching sentinel (the pick that moves with M; quantiser included).

    python tools/native_invariant_bench.py [--reps 5] [--quick] [--out session.json] [--md table.md]
    python tools/native_invariant_bench.py --forms-lib tools/ablate/libpetit_amd_native_inv_forms.so [--out forms.json] [--md forms.md]

    python tools/native_invariant_bench.py --nvfp4 [--forms-lib ...] [--out ...] [--md ...]

--nvfp4: the entry on NVFP4 images (petit_gemm_nvfp4_native_invariant) in the new entry's place, against (a) petit_gemm_fp4_fp16_invariant, the
exact class's invariant entry on the packed NVFP4 tensors, (b) the native default on the same image (petit_gemm_fp4_fp16_grid_ws with the
matching sentinel, the image attached), (c) petit_gemm_mxfp4_native_invariant at the same shape; with --forms-lib both forms of the NVFP4
entry at M = 32 / 64 / 65 / 128.

The four Llama-3-70B linears (qkv 10240 x 8192, o 8192 x 8192, gate_up 57344 x 8192, down 8192 x 28672) at M in {1, 16, 64, 512, 4096}, bf16.
Every side goes through the C ABI with a per-problem workspace and is captured into HIP graphs of `launches` calls over rotating weight copies
(together beyond the 256 MB Infinity Cache; tools/benchlib.py Weights), replayed `reps` times, all sides in turn, then all once more; reported
per launch: the median over a side's replays, its minimum and maximum.

--forms-lib: the form switch.  A measurement-only build of the library (csrc/gemm_invariant_api.hip compiled with
-DPETIT_NATIVE_INV_MEASURE_FORMS=1 and linked with the other objects, -Wl,-Bsymbolic) reads the switch from $PETIT_NATIVE_INV_SPLIT_MAX_M per call; the run
times the split and the whole form of the new entry at M = 16 / 32 / 64 on the four shapes, interleaved."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
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
FORM_MS = (16, 32, 64)
NV_FORM_MS = (32, 64, 65, 128)
FMTS = {"mxfp8": (8, _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP8), "mxfp6": (6, _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP6),
        "mxfp4": (4, _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP4)}


def native_invariant_launcher(g: benchlib.Gemm, code: int, lib=None):
    """launch(i) of the new entry on Gemm's operands (16-bit input: the quantiser runs inside the call); NVFP4 weights: the entry on their images"""
    lib = lib or _lib.lib
    m, n, k = g.m, g.w.n, g.w.k
    need = int(lib.petit_gemm_native_invariant_workspace_bytes(m, n, k, g.a_type, code, 0))
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=g.dev)
    fn = lib.petit_gemm_mxfp4_native_invariant
    if g.w.fmt == "nv":
        g.w.attach_native()
        images, nv = g.w.images, lib.petit_gemm_nvfp4_native_invariant

        def launch_nv(i, _keep=ws):
            rc = nv(C.c_void_p(g.c.data_ptr()), C.c_void_p(g.a.data_ptr()), C.c_void_p(images[i % len(images)].data_ptr()),
                    C.c_void_p(g.gs.data_ptr()), m, n, k, C.byref(g.hints), code, 0, None, C.c_void_p(ws.data_ptr()),
                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
            if rc != 0:
                raise RuntimeError(f"rc={rc} ({_lib.error_string(rc)})")
        return launch_nv

    def launch(i, _keep=ws):
        b, sp = g.w[i]
        rc = fn(C.c_void_p(g.c.data_ptr()), C.c_void_p(g.a.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(sp.data_ptr()),
                C.c_void_p(g.gs.data_ptr()), m, n, k, C.byref(g.hints), code, 0, None, C.c_void_p(ws.data_ptr()),
                C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise RuntimeError(f"rc={rc} ({_lib.error_string(rc)})")
    return launch


def exact_invariant_launcher(g: benchlib.Gemm):
    m, n, k = g.m, g.w.n, g.w.k
    need = int(_lib.lib.petit_gemm_invariant_workspace_bytes(m, n, k, g.a_type, g.b_type))
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=g.dev)

    def launch(i, _keep=ws):
        b, sp = g.w[i]
        rc = (_lib.lib.petit_gemm_fp4_fp16_invariant if g.w.fmt == "nv" else _lib.lib.petit_gemm_mxfp4_fp16_invariant)(C.c_void_p(g.c.data_ptr()), C.c_void_p(g.a.data_ptr()), C.c_void_p(b.data_ptr()),
                                                      C.c_void_p(sp.data_ptr()), C.c_void_p(g.gs.data_ptr()), m, n, k, C.byref(g.hints), None,
                                                      C.c_void_p(ws.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise RuntimeError(f"rc={rc} ({_lib.error_string(rc)})")
    return launch


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


def time_sides(sides: dict, reps: int, stream) -> dict:
    """every side in turn, then all once more -> {side: {us, min, max, launches}}"""
    launches = {s: int(max(4, min(200, 20000.0 / max(one_call_us(fn, stream), 1.0)))) for s, fn in sides.items()}
    samples = {s: [] for s in sides}
    for _ in range(2):
        for side, fn in sides.items():
            samples[side] += benchlib.time_graph(fn, launches[side], reps, stream)
    return {s: {"us": round(benchlib.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2), "launches": launches[s]}
            for s, v in samples.items()}


def cells_markdown(rows) -> str:
    head = ["shape", "M", "S", "L", "form"] + [f"inv {f} us" for f in FMTS] + ["exact inv us"] + [f"default {f} us" for f in FMTS] + \
           [f"inv {f} / exact inv" for f in FMTS] + [f"inv {f} / default {f}" for f in FMTS]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for r in rows:
        t = r["sides"]
        cell = [f"{r['shape']} {r['N']}x{r['K']}", str(r["M"]), str(r["S"]), str(r["L"]), r["form"]]
        cell += [f"{t['inv_' + f]['us']:.1f}" for f in FMTS] + [f"{t['exact_inv']['us']:.1f}"]
        cell += [f"{t['default_' + f]['us']:.1f}" if "default_" + f in t else "-" for f in FMTS]
        cell += [f"{t['inv_' + f]['us'] / t['exact_inv']['us']:.2f}" for f in FMTS]
        cell += [f"{t['inv_' + f]['us'] / t['default_' + f]['us']:.2f}" if "default_" + f in t else "-" for f in FMTS]
        lines.append("| " + " | ".join(cell) + " |")
    return "\n".join(lines) + "\n"


def nv_cells_markdown(rows) -> str:
    head = ["shape", "M", "S", "L", "form"] + [f"image inv {f} us" for f in FMTS] + ["(a) a16 inv us"] + [f"(b) default {f} us" for f in FMTS] + \
           [f"(c) mxfp4 inv {f} us" for f in FMTS] + [f"{f} / (a)" for f in FMTS] + [f"{f} / (b)" for f in FMTS] + [f"{f} / (c)" for f in FMTS]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for r in rows:
        t = r["sides"]
        ratio = lambda f, other: f"{t['inv_' + f]['us'] / t[other]['us']:.2f}" if other in t else "-"  # noqa: E731
        cell = [f"{r['shape']} {r['N']}x{r['K']}", str(r["M"]), str(r["S"]), str(r["L"]), r["form"]]
        cell += [f"{t['inv_' + f]['us']:.1f} ({t['inv_' + f]['min']:.1f}..{t['inv_' + f]['max']:.1f})" for f in FMTS] + [f"{t['exact_inv']['us']:.1f}"]
        cell += [f"{t['default_' + f]['us']:.1f}" if "default_" + f in t else "-" for f in FMTS]
        cell += [f"{t['mx_inv_' + f]['us']:.1f}" for f in FMTS]
        cell += [ratio(f, "exact_inv") for f in FMTS] + [ratio(f, "default_" + f) for f in FMTS] + [ratio(f, "mx_inv_" + f) for f in FMTS]
        lines.append("| " + " | ".join(cell) + " |")
    return "\n".join(lines) + "\n"


def forms_markdown(rows) -> str:
    lines = ["| shape | format | M | split us | whole us | split / whole | split min..max | whole min..max |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        s, w = r["sides"]["split"], r["sides"]["whole"]
        lines.append(f"| {r['shape']} {r['N']}x{r['K']} | {r['fmt']} | {r['M']} | {s['us']:.1f} | {w['us']:.1f} | {s['us'] / w['us']:.2f} | "
                     f"{s['min']:.1f}..{s['max']:.1f} | {w['min']:.1f}..{w['max']:.1f} |")
    return "\n".join(lines) + "\n"


def run_cells(args, dev, stream):
    shapes = {"small": (1024, 1024)} if args.quick else SHAPES
    rows = []
    for name, (n, k) in shapes.items():
        weights = benchlib.Weights("mx", n, k, 64 if args.quick else 1280, dev)
        for m in ((1, 64) if args.quick else MS):
            g = benchlib.Gemm(weights, m, torch.bfloat16, dev)
            S, L = C.c_uint(0), C.c_uint(0)
            _lib.lib.petit_gemm_invariant_geometry(n, k, g.a_type, g.b_type, C.byref(S), C.byref(L))
            sides = {"inv_" + f: native_invariant_launcher(g, code) for f, (code, _) in FMTS.items()}
            sides["exact_inv"] = exact_invariant_launcher(g)
            for f, (_, sentinel) in FMTS.items():
                fn = g.launcher(sentinel)
                try:
                    fn(0)
                    sides["default_" + f] = fn
                except RuntimeError as exc:                               # a cell the native default refuses is reported as missing, not guessed
                    print(f"# native default {f} at {name} M={m}: {exc}", flush=True)
            row = {"shape": name, "N": n, "K": k, "M": m, "S": S.value, "L": L.value,
                   "form": "split" if _lib.lib.petit_gemm_native_invariant_workspace_bytes(m, n, k, g.a_type, 8, 1) else "whole",
                   "sides": time_sides(sides, args.reps, stream), "reps": 2 * args.reps}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del g, sides
        del weights
        torch.cuda.empty_cache()
    return rows


def run_nv_cells(args, dev, stream):
    """the NVFP4-image entry against (a), (b), (c) of the module's text; the MXFP4 side on weights of its own of the same shape"""
    shapes = {"small": (1024, 1024)} if args.quick else SHAPES
    rows = []
    for name, (n, k) in shapes.items():
        weights = benchlib.Weights("nv", n, k, 64 if args.quick else 1280, dev)
        mx = benchlib.Weights("mx", n, k, 64 if args.quick else 1280, dev, seed=4321)
        for m in ((1, 64) if args.quick else MS):
            g, gm = benchlib.Gemm(weights, m, torch.bfloat16, dev), benchlib.Gemm(mx, m, torch.bfloat16, dev)
            S, L = C.c_uint(0), C.c_uint(0)
            _lib.lib.petit_gemm_invariant_geometry(n, k, g.a_type, g.b_type, C.byref(S), C.byref(L))
            sides = {"inv_" + f: native_invariant_launcher(g, code) for f, (code, _) in FMTS.items()}
            sides["exact_inv"] = exact_invariant_launcher(g)
            for f, (code, sentinel) in FMTS.items():
                sides["mx_inv_" + f] = native_invariant_launcher(gm, code)
                fn = g.launcher(sentinel)
                try:
                    fn(0)
                    sides["default_" + f] = fn
                except RuntimeError as exc:                               # a cell the native default refuses is reported as missing, not guessed
                    print(f"# native default {f} at {name} M={m}: {exc}", flush=True)
            row = {"weights": "nvfp4 image", "shape": name, "N": n, "K": k, "M": m, "S": S.value, "L": L.value,
                   "form": "split" if _lib.lib.petit_gemm_native_invariant_workspace_bytes(m, n, k, g.a_type, 8, 1) else "whole",
                   "sides": time_sides(sides, args.reps, stream), "reps": 2 * args.reps}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del g, gm, sides
        del weights, mx
        torch.cuda.empty_cache()
    return rows


def run_forms(args, dev, stream):
    lib = C.CDLL(str(Path(args.forms_lib).resolve()))
    for name in ("petit_gemm_native_invariant_workspace_bytes", "petit_gemm_mxfp4_native_invariant", "petit_gemm_nvfp4_native_invariant"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = getattr(_lib.lib, name).restype, getattr(_lib.lib, name).argtypes
    os.environ["PETIT_NATIVE_INV_SPLIT_MAX_M"] = "0"                      # the library must follow the switch, or the run measures nothing
    assert lib.petit_gemm_native_invariant_workspace_bytes(16, 64, 1024, _lib.CXX_DTYPE_BF16, 8, 1) == 0, "not a measurement-only build"
    os.environ["PETIT_NATIVE_INV_SPLIT_MAX_M"] = str(1 << 20)
    assert lib.petit_gemm_native_invariant_workspace_bytes(64, 64, 1024, _lib.CXX_DTYPE_BF16, 8, 1) > 0, "not a measurement-only build"
    rows = []
    for name, (n, k) in SHAPES.items():
        weights = benchlib.Weights("nv" if args.nvfp4 else "mx", n, k, 1280, dev)
        for m in (NV_FORM_MS if args.nvfp4 else FORM_MS):
            g = benchlib.Gemm(weights, m, torch.bfloat16, dev)
            for f, (code, _) in FMTS.items():
                sides = {}
                for form, switch in (("split", 1 << 20), ("whole", 0)):
                    os.environ["PETIT_NATIVE_INV_SPLIT_MAX_M"] = str(switch)
                    inner = native_invariant_launcher(g, code, lib)       # (the workspace is sized under the same switch)

                    def launch(i, _inner=inner, _switch=str(switch)):
                        os.environ["PETIT_NATIVE_INV_SPLIT_MAX_M"] = _switch
                        _inner(i)
                    sides[form] = launch
                row = {"weights": "nvfp4 image" if args.nvfp4 else "mxfp4", "shape": name, "N": n, "K": k, "M": m, "fmt": f,
                       "sides": time_sides(sides, args.reps, stream), "reps": 2 * args.reps}
                print(json.dumps(row), flush=True)
                rows.append(row)
            del g
        del weights
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="one small shape: a rehearsal of the script, not a measurement")
    ap.add_argument("--forms-lib", default="", help="the measurement-only library: time both forms at M = 16 / 32 / 64 instead of the cells")
    ap.add_argument("--nvfp4", action="store_true", help="the entry on NVFP4 images against (a), (b), (c) of the module's text")
    ap.add_argument("--out", default="")
    ap.add_argument("--md", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to report without one"
    dev = torch.device("cuda")
    stream = torch.cuda.Stream()
    rows = run_forms(args, dev, stream) if args.forms_lib else run_nv_cells(args, dev, stream) if args.nvfp4 else run_cells(args, dev, stream)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rows, indent=1) + "\n")
    if args.md:
        Path(args.md).write_text(forms_markdown(rows) if args.forms_lib else nv_cells_markdown(rows) if args.nvfp4 else cells_markdown(rows))


if __name__ == "__main__":
    main()

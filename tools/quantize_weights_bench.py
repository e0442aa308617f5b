#!/usr/bin/env python3
"""tools/quantize_weights_bench.py -- time the device weight quantiser (petit_kernel.quantize_nvfp4 / quantize_mxfp4) against a chain of torch ops
that does the same recipe on the device and then calls repack_* / process_*_scales (what a caller had to write before the quantiser existed).

    python tools/quantize_weights_bench.py [--reps 10] [--quick] [--out profiles/weight_quant.json]

Shapes: a Llama-70B gate_up [57344, 8192] and a stacked expert tensor [128, 1536, 2048], bf16.  The quantiser is timed as graph replays over
rotating inputs (each copy is 0.8-0.9 GB, beyond the 256 MB Infinity Cache), the chain eagerly with device events (it allocates GBs of f32
intermediates: part of what it costs).  GB/s counts 2 N K bytes in and 0.5625 N K out (NVFP4; MXFP4 writes 0.53125 N K, counted as such), shown
next to the copy ceiling DESIGN.md quotes (6.29 TB/s).  The chain's arithmetic is f32 torch, not the contract's exact thresholds: it is a
comparator for time, not for bits."""
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

COPY_CEILING_TBS = 6.29
SHAPES = {"llama70b_gate_up": (1, 57344, 8192), "stacked_experts_128": (128, 1536, 2048)}
QUICK = {"small_linear": (1, 4096, 4096), "small_experts": (8, 512, 1024)}


def _codes(x: torch.Tensor) -> torch.Tensor:
    mid = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], device=x.device)
    idx = torch.bucketize(x.abs(), mid).to(torch.uint8)
    return idx | ((x < 0) & (idx != 0)).to(torch.uint8) << 3


def _pack(codes: torch.Tensor, rows: int, k: int) -> torch.Tensor:
    codes = codes.view(rows, k)
    return (codes[:, 0::2] | codes[:, 1::2] << 4).contiguous().view(torch.int32)


def chain_nvfp4(w: torch.Tensor):
    E, n, k = w.shape
    wf = w.float()
    amax = wf.abs().amax(dim=(1, 2))
    gs = torch.where(amax == 0, torch.ones_like(amax), amax / 2688.0)
    blk = wf.abs().view(E, n, k // 16, 16).amax(-1)
    sb = ((blk / 6.0) / gs[:, None, None]).clamp(max=448.0).to(torch.float8_e4m3fn)
    s = sb.float() * gs[:, None, None]
    q = _pack(_codes(wf.view(E, n, k // 16, 16) / torch.where(s > 0, s, torch.ones_like(s))[..., None]), E * n, k)
    return pk.repack_nvfp4(q, E * n, k), pk.process_nvfp4_scales(sb.view(E * n, k // 16), E * n, k), gs


def chain_mxfp4(w: torch.Tensor):
    E, n, k = w.shape
    wf = w.float()
    blk = wf.abs().view(E, n, k // 32, 32).amax(-1)
    e = torch.where(blk > 0, torch.ceil(torch.log2(blk / 6.0)), torch.full_like(blk, -126.0)).clamp(-126, 127)
    q = _pack(_codes(wf.view(E, n, k // 32, 32) * torch.exp2(-e)[..., None]), E * n, k)
    sb = (e + 127).to(torch.uint8).view(E * n, k // 32)
    return pk.repack_mxfp4(q, E * n, k), pk.process_mxfp4_scales(sb, E * n, k), torch.ones(E, device=w.device)


def time_eager(fn, reps: int) -> list:
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--copies", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="small shapes: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to report without one"
    stream = torch.cuda.Stream()
    rows = []
    for name, (E, n, k) in (QUICK if args.quick else SHAPES).items():
        gen = torch.Generator(device="cuda").manual_seed(0)
        ws = [(torch.randn((E, n, k), device="cuda", generator=gen) / k ** 0.5).bfloat16() for _ in range(args.copies)]
        gs_in = torch.full((E,), 2.0 ** -12, device="cuda")
        forms = {"nvfp4": (lambda w: pk.quantize_nvfp4(w), chain_nvfp4, 2.5625),
                 "nvfp4_gs_supplied": (lambda w: pk.quantize_nvfp4(w, gs_in), None, 2.5625),
                 "mxfp4": (lambda w: pk.quantize_mxfp4(w), chain_mxfp4, 2.53125)}
        for form, (quant, chain, bytes_per_weight) in forms.items():
            nbytes = bytes_per_weight * E * n * k
            us = benchlib.median(benchlib.time_graph(lambda i: quant(ws[i % len(ws)]), len(ws), args.reps, stream))
            row = {"shape": name, "E": E, "n": n, "k": k, "form": form, "us": round(us, 1), "GBps": round(nbytes / us / 1e3, 1),
                   "of_copy_ceiling": round(nbytes / us / 1e6 / COPY_CEILING_TBS, 3)}
            if chain is not None:
                chain_us = benchlib.median(time_eager(lambda: chain(ws[0]), max(3, args.reps // 3)))
                row.update(torch_chain_us=round(chain_us, 1), speedup_over_chain=round(chain_us / us, 2))
            print(json.dumps(row), flush=True)
            rows.append(row)
        del ws
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()

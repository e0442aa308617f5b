#!/usr/bin/env python3
"""tools/native_image_readback_bench.py -- time the device readers of the native image (petit_kernel.dequant_native_image, mxfp6_export) next to
the writer of the same image (quantize_mxfp6) and to a chain of torch ops that expands the same image on the device.

    python tools/native_image_readback_bench.py [--reps 10] [--quick] [--no-chain] [--out FILE]

Shapes: the four Llama-3-70B linears (qkv, o, gate_up, down) and a stacked expert tensor [128, 1536, 2048].  Every form is timed as graph
replays over rotating images (each copy of the large shapes is beyond the 256 MB Infinity Cache), the chain eagerly with device events (it
allocates GBs of intermediates: part of what it costs).  GB/s counts the bytes the form must move -- an image is 0.78125 N K bytes, the OCP tensor
the same, bf16 / fp16 weights 2 N K, f32 4 N K -- next to the copy ceiling DESIGN.md quotes (6.29 TB/s).  Before anything is timed the chain and
the kernel are held against each other on the first expert (equal bits): the chain is a comparator for time on the same result."""
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
from quantize_weights_bench import COPY_CEILING_TBS, LLAMA70B, time_eager  # noqa: E402

SHAPES = dict(LLAMA70B, stacked_experts_128=(128, 1536, 2048))
QUICK = {"small_linear": (1, 4096, 4096), "small_experts": (8, 512, 1024)}
IMAGE = 0.78125   # bytes per weight of an image, and of an OCP MXFP6 tensor with its scales


def chain_dequant(images: torch.Tensor, E: int, n: int, k: int, dtype=torch.bfloat16) -> torch.Tensor:
    """The image(s) expanded by torch ops (n % 32 == 0): gather each block's 24 bytes, unpack the bits, look the codes up, scale, un-tile."""
    dev, nb, kt, ks = images.device, n // 32, k // 128, 8 if k % 1024 == 0 else 4 if k % 512 == 0 else 2
    img = images.view(E, -1)
    el = img[:, :nb * kt * 3072].reshape(E * nb, kt, 3, 2, 32, 16)                                   # [b, kt, plane, h, r, byte]
    hi = el[:, :, 2].reshape(E * nb, kt, 2, 32, 2, 8).permute(0, 1, 4, 2, 3, 5)                      # [b, kt, q, h, r, 8]: registers 4-5
    bits = (torch.cat([el[:, :, :2], hi], -1)[..., None] >> torch.arange(8, device=dev, dtype=torch.uint8)) & 1
    code = (bits.reshape(E * nb, kt, 2, 2, 32, 32, 6) << torch.arange(6, device=dev, dtype=torch.uint8)).sum(-1, dtype=torch.uint8)
    c = torch.arange(64, device=dev)
    mag = torch.where((c & 24) != 0, (8 + (c & 7)) / 8.0 * torch.exp2(((c >> 3) & 3) - 1.0), (c & 7) / 8.0)
    val = torch.where((c & 32) != 0, -mag, mag).float()[code.long()]                                  # [b, kt, q, h, r, 32]
    sc = img[:, nb * kt * 3072:].reshape(E * nb, kt // ks, 2, 32, 2, ks).permute(0, 1, 5, 4, 2, 3)    # [b, sp, h, r, q, t] -> [b, sp, t, q, h, r]
    val = val * torch.exp2(sc.reshape(E * nb, kt, 2, 2, 32, 1).float() - 127.0)
    return val.permute(0, 4, 1, 2, 3, 5).reshape(E, n, k).to(dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--copies", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="small shapes: a rehearsal of the script, not a measurement")
    ap.add_argument("--no-chain", action="store_true", help="skip the torch-op comparator")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to report without one"
    stream = torch.cuda.Stream()
    rows = []
    for name, (E, n, k) in (QUICK if args.quick else SHAPES).items():
        gen = torch.Generator(device="cuda").manual_seed(0)
        ws = [(torch.randn((E, n, k), device="cuda", generator=gen) / k ** 0.5).bfloat16() for _ in range(args.copies)]
        imgs = [pk.quantize_mxfp6(w) for w in ws]
        per = imgs[0].numel() // E
        assert torch.equal(chain_dequant(imgs[0][:per], 1, n, k)[0], pk.dequant_native_image(imgs[0][:per], n, k)), "the chain is not the kernel's result"
        assert torch.equal(pk.mxfp6_native_image(*pk.mxfp6_export(imgs[0], n, k), n, k), imgs[0])
        forms = {"dequant_bf16": (lambda i: pk.dequant_native_image(imgs[i], n, k, torch.bfloat16), IMAGE + 2),
                 "dequant_fp16": (lambda i: pk.dequant_native_image(imgs[i], n, k, torch.float16), IMAGE + 2),
                 "dequant_f32": (lambda i: pk.dequant_native_image(imgs[i], n, k, torch.float32), IMAGE + 4),
                 "mxfp6_export": (lambda i: pk.mxfp6_export(imgs[i], n, k), 2 * IMAGE),
                 "quantize_mxfp6": (lambda i: pk.quantize_mxfp6(ws[i]), IMAGE + 2)}
        for form, (fn, bytes_per_weight) in forms.items():
            nbytes = bytes_per_weight * E * n * k
            us = benchlib.median(benchlib.time_graph(lambda i: fn(i % len(ws)), len(ws), args.reps, stream))
            row = {"shape": name, "E": E, "n": n, "k": k, "form": form, "us": round(us, 1), "GBps": round(nbytes / us / 1e3, 1),
                   "of_copy_ceiling": round(nbytes / us / 1e6 / COPY_CEILING_TBS, 3)}
            if form == "dequant_bf16" and not args.no_chain:
                chain_us = benchlib.median(time_eager(lambda: chain_dequant(imgs[0], E, n, k), max(3, args.reps // 3)))
                row.update(torch_chain_us=round(chain_us, 1), speedup_over_chain=round(chain_us / us, 2))
            print(json.dumps(row), flush=True)
            rows.append(row)
        del ws, imgs
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()

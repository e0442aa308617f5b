#!/usr/bin/env python3
"""tools/mxfp6_weights_bench.py -- what MXFP6 weights on the native class cost and buy (petit_kernel.quantize_mxfp6 / mxfp6_native_image).

    python tools/mxfp6_weights_bench.py --accuracy [--out profiles/mxfp6_weights_accuracy.json]      # CPU twins, no GPU
    python tools/mxfp6_weights_bench.py [--reps 10] [--quick] [--out profiles/mxfp6_weights_time.json]

--accuracy: checkpoint-like weights (tools/quantize_weights.py) through the MLP block of tools/hadamard_quant_bench.py (hidden 2048, intermediate
4096, 96 tokens, six input columns x 60), evaluated with the CPU twins: the weight's own quantisation error as a share of its rms, and the block's
error (relative to the rms of the bf16-weight block's output) for NVFP4, NVFP4 on its image and MXFP6 weights, with unquantised, MXFP8, MXFP6 and
MXFP4 activations, plain and with hadamard = 32 (the MXFP6 activation quantiser has no rotating form: no such cell).

Time: the Llama-3-70B linears and one stacked-expert shape, bf16, as graph replays over rotating inputs beyond the 256 MB Infinity Cache:
quantize_mxfp6 (2 N K bytes in, 0.78125 N K out), mxfp6_native_image (0.78125 N K in and out) and quantize_mxfp4 on the same inputs (2 N K in,
0.53125 N K out), each next to its bytes at the copy ceiling DESIGN.md quotes (6.29 TB/s)."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "petit-kernel_amd"))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import petit_kernel as pk  # noqa: E402
from petit_kernel import offline  # noqa: E402

COPY_CEILING_TBS = 6.29
SHAPES = {"qkv": (1, 10240, 8192), "o": (1, 8192, 8192), "gate_up": (1, 57344, 8192), "down": (1, 8192, 28672),
          "stacked_experts_128": (128, 1536, 2048)}
QUICK = {"small_linear": (1, 4096, 4096), "small_experts": (8, 512, 1024)}
ROTATE_BYTES = 640 << 20


# --- accuracy (CPU twins) -------------------------------------------------------------------------------------------------------------------------------

def accuracy() -> dict:
    import quantize_weights as QW
    from test_gpu_parity import decode_qact
    hid, inter, m = 2048, 4096, 96
    rng = np.random.default_rng(2027)
    x = rng.standard_normal((m, hid), dtype=np.float32)
    x[:, rng.choice(hid, 6, replace=False)] *= 60.0
    xt = torch.from_numpy(x).bfloat16()
    xf = xt.double().numpy()
    w1, w2 = QW.synthetic_weights(2 * inter, hid, 31), QW.synthetic_weights(hid, inter, 32)

    def silu_mul(y1):
        return y1[:, :inter] / (1.0 + np.exp(-y1[:, :inter])) * y1[:, inter:]

    def act_q(a16: torch.Tensor, fmt, block: int) -> np.ndarray:
        if fmt is None:
            return a16.double().numpy()
        q = offline.quantize_activations_cpu(a16.contiguous(), fmt, hadamard=block)
        return decode_qact(q.data.numpy(), q.m, q.k, fmt).astype(np.float64)

    def image_values(image: torch.Tensor, n: int, k: int) -> np.ndarray:
        if torch.cuda.is_available():   # the device dequantiser (f32: exact); its CPU twin, the same bits, without a GPU
            return pk.dequant_native_image(image.cuda(), n, k, torch.float32).cpu().double().numpy()
        return offline.dequant_native_image_cpu(image, n, k, torch.float32).double().numpy()

    def weights_q(w: np.ndarray, wfmt: str, block: int) -> np.ndarray:
        wt = torch.from_numpy(w).bfloat16()
        n, k = wt.shape
        if block:
            wt = offline.hadamard_rotate_cpu(wt, block, -(block.bit_length() - 1))
        if wfmt == "mxfp6":
            return image_values(offline.quantize_mxfp6_cpu(wt), n, k)
        q, sb, gs = QW.quantize_nvfp4(wt.float().numpy())
        if wfmt == "nvfp4":
            return QW.dequantize("nvfp4", q, sb, gs)
        b = offline.repack_nvfp4_cpu(torch.from_numpy(q.copy()).view(torch.int32), n, k)
        sp = offline.process_nvfp4_scales_cpu(torch.from_numpy(sb.copy()).view(torch.float8_e4m3fn), n, k)
        return image_values(offline.nvfp4_native_image_cpu(b, sp, n, k), n, k) * float(gs)

    ref_bf16 = silu_mul(xf @ w1.astype(np.float64).T) @ w2.astype(np.float64).T
    rms = float(np.sqrt(np.mean(ref_bf16 ** 2)))
    rel = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2)) / rms)  # noqa: E731
    out = {"hidden": hid, "intermediate": inter, "m": m, "outlier_columns": 6, "outlier_factor": 60, "rows": []}
    for block in (0, 32):
        h = np.array([[1.0]])
        while block and h.shape[0] < block:
            h = np.kron(np.array([[1.0, 1.0], [1.0, -1.0]]), h)
        # a rotated weight matrix meets the rotated activation: x . H . (W . H / B)^T, whose exact value is x . (dq . H)^T (H symmetric)
        unrot = (lambda dq: (dq.reshape(dq.shape[0], -1, block) @ h).reshape(dq.shape)) if block else (lambda dq: dq)  # noqa: E731
        for wfmt in ("nvfp4", "nvfp4_image", "mxfp6"):
            dq1, dq2 = weights_q(w1, wfmt, block), weights_q(w2, wfmt, block)
            w_err = float(np.sqrt(np.mean((unrot(dq1) - w1) ** 2) / np.mean(w1.astype(np.float64) ** 2)))
            row = {"hadamard": block, "weights": wfmt, "weight_error_of_weight_rms": w_err}
            for afmt in (None, "mxfp8", "mxfp6", "mxfp4"):
                if block and afmt == "mxfp6":
                    continue
                if afmt is None:
                    y = silu_mul(xf @ unrot(dq1).T) @ unrot(dq2).T
                else:
                    h16 = torch.from_numpy(silu_mul(act_q(xt, afmt, block) @ dq1.T)).bfloat16()      # the 16-bit hand-over between the two GEMMs
                    y = act_q(h16, afmt, block) @ dq2.T
                row["block_error_" + (afmt or "unquantised") + "_activations"] = rel(y, ref_bf16)
            print(json.dumps(row), flush=True)
            out["rows"].append(row)
    return out


# --- time (GPU) -------------------------------------------------------------------------------------------------------------------------------------------

def timing(reps: int, quick: bool) -> list:
    import benchlib
    assert torch.cuda.is_available(), "the timing part measures the GPU; there is nothing to report without one (--accuracy runs on the CPU)"
    stream = torch.cuda.Stream()
    rows = []
    for name, (E, n, k) in (QUICK if quick else SHAPES).items():
        copies = max(2, ROTATE_BYTES // (2 * E * n * k) + 1)
        gen = torch.Generator(device="cuda").manual_seed(0)
        ws = [(torch.randn((E, n, k), device="cuda", generator=gen) / k ** 0.5).bfloat16() for _ in range(copies)]
        elems = [torch.randint(0, 256, (E, n, k // 4 * 3), device="cuda", generator=gen, dtype=torch.uint8) for _ in range(copies)]
        scales = [torch.randint(100, 140, (E, n, k // 32), device="cuda", generator=gen, dtype=torch.uint8) for _ in range(copies)]
        forms = {"quantize_mxfp6": (lambda i: pk.quantize_mxfp6(ws[i % copies]), 2.0, 0.78125),       # (launch, bytes in, bytes out per weight)
                 "mxfp6_native_image": (lambda i: pk.mxfp6_native_image(elems[i % copies], scales[i % copies], n, k), 0.78125, 0.78125),
                 "quantize_mxfp4": (lambda i: pk.quantize_mxfp4(ws[i % copies]), 2.0, 0.53125)}
        for form, (launch, b_in, b_out) in forms.items():
            nbytes = (b_in + b_out) * E * n * k
            us = sorted(benchlib.time_graph(launch, copies, reps, stream))
            med = us[len(us) // 2]
            row = {"shape": name, "E": E, "n": n, "k": k, "form": form, "us": round(med, 1), "us_min": round(us[0], 1), "us_max": round(us[-1], 1),
                   "us_at_copy_ceiling": round(nbytes / COPY_CEILING_TBS / 1e6, 1), "GBps": round(nbytes / med / 1e3, 1),
                   "ps_per_input_byte": round(med * 1e6 / (b_in * E * n * k), 4)}
            print(json.dumps(row), flush=True)
            rows.append(row)
        del ws, elems, scales
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--accuracy", action="store_true", help="the accuracy part (CPU twins) instead of the timing part")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="small shapes: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    result = accuracy() if args.accuracy else timing(args.reps, args.quick)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()

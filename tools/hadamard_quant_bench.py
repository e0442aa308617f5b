#!/usr/bin/env python3
"""tools/hadamard_quant_bench.py -- what the block-Hadamard rotation inside the activation quantisers costs and what it buys
(include/petit_amd.h "Block-Hadamard rotation"); writes profiles/hadamard_quant.md.

    python tools/hadamard_quant_bench.py --accuracy [--json profiles/hadamard_quant_accuracy.json]      (CPU twins: no GPU needed)
    python tools/hadamard_quant_bench.py --time [--reps 20] [--json profiles/hadamard_quant_time.json]   (needs the GPU)
    python tools/hadamard_quant_bench.py --report ACCURACY.json TIME.json --date YYYY-MM-DD [--out profiles/hadamard_quant.md]

--time: bf16, m in {1, 16, 512, 4096}, k in {4096, 8192}, fmt in {mxfp4, mxfp8}, B in {32, 128}; per cell
    (a) quantize_activations(x, fmt, hadamard=B)                      one launch
    (b) quantize_activations(x, fmt)                                  the unrotated quantiser, one launch
    (c) quantize_activations(hadamard_rotate(x, B), fmt)              the unfused chain, two launches and a 16-bit [m][k] round trip
and the same three for rmsnorm_quantize at k = 8192 ((c) = the norm's y16, rotated, then quantised: three launches).
Rule: each of the three is captured into a HIP graph of `launches` calls over inputs that rotate over more than the 256 MB Infinity Cache
(at most 256 launches per graph: the small-m cells are launch-bound and their inputs stay cache-resident, as they do in a decode step);
the three graphs are replayed ALTERNATELY in one process, `reps` times each, timed with device events; reported: the median per launch
and the spread (max - min) / median of each side's replays.  The condition is a / c <= 1 in every cell; a / b is the price of the rotation
and has no bar.  (c) rounds the rotated row to 16 bit before quantising, so its bytes are not (a)'s: it is the chain a caller would
otherwise write, not a reference.

--accuracy: the MLP block of tests/test_gpu_parity.py::test_mlp_block_accuracy_budget_checkpoint_like_weights (hidden 2048, intermediate 4096,
96 tokens, six input columns x 60, weights of tools/quantize_weights.py) evaluated with the CPU twins: MXFP4 activations into gate_up and into
down, unrotated and rotated with B = 32 / 128 (weights rotated by hadamard_rotate_cpu(w, B, -log2 B) before they are quantised), errors
relative to the rms of the bf16-weight block's output.
"""
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
sys.path.insert(0, str(ROOT / "tests"))   # (decode_qact: the tests' numpy reading of "petit-qact/1")
sys.path.insert(0, str(ROOT))

import petit_kernel as pk  # noqa: E402
from petit_kernel import offline  # noqa: E402

MS, KS, FMTS, BLOCKS = (1, 16, 512, 4096), (4096, 8192), ("mxfp4", "mxfp8"), (32, 128)
ROTATE_BYTES = 320 << 20
MAX_LAUNCHES = 256
EPS = 1e-6


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

    def act_q(a16: torch.Tensor, block: int) -> np.ndarray:
        q = offline.quantize_activations_cpu(a16.contiguous(), "mxfp4", hadamard=block)
        return decode_qact(q.data.numpy(), q.m, q.k, "mxfp4").astype(np.float64)

    def weights_q(w: np.ndarray, block: int) -> np.ndarray:
        wt = torch.from_numpy(w).bfloat16()
        if block:
            wt = offline.hadamard_rotate_cpu(wt, block, -(block.bit_length() - 1))
        q, sb, gs = QW.quantize_mxfp4(wt.float().numpy())
        return QW.dequantize("mxfp4", q, sb, gs)

    ref_bf16 = silu_mul(xf @ w1.astype(np.float64).T) @ w2.astype(np.float64).T
    rms = float(np.sqrt(np.mean(ref_bf16 ** 2)))
    rel = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2)) / rms)  # noqa: E731
    out = {"hidden": hid, "intermediate": inter, "m": m, "outlier_columns": 6, "outlier_factor": 60, "rows": {}}
    for block in (0,) + BLOCKS:
        dq1, dq2 = weights_q(w1, block), weights_q(w2, block)
        # the exact-FP4 model on these weights with unquantised activations: a rotated weight matrix meets the rotated activation,
        # x . H . (W . H / B)^T, whose exact value is x . W_dq'^T with W_dq' = dq . H (H symmetric)
        if block:
            h = np.array([[1.0]])
            while h.shape[0] < block:
                h = np.kron(np.array([[1.0, 1.0], [1.0, -1.0]]), h)
            unrot = lambda dq: (dq.reshape(dq.shape[0], -1, block) @ h).reshape(dq.shape)  # noqa: E731
        else:
            unrot = lambda dq: dq  # noqa: E731
        ref_fp4 = silu_mul(xf @ unrot(dq1).T) @ unrot(dq2).T
        h16 = torch.from_numpy(silu_mul(act_q(xt, block) @ dq1.T)).bfloat16()      # the 16-bit hand-over (a rotating `down` takes it)
        y = act_q(h16, block) @ dq2.T
        out["rows"][str(block)] = {"weight_quantisation_vs_bf16_weights": rel(ref_fp4, ref_bf16), "activation_quantisation_vs_exact_fp4": rel(y, ref_fp4),
                                   "total_vs_bf16_weight_block": rel(y, ref_bf16)}
        print(json.dumps({str(block): out["rows"][str(block)]}), flush=True)
    return out


# --- timing (GPU) ---------------------------------------------------------------------------------------------------------------------------------------

def capture(launch, launches: int, stream):
    with torch.cuda.stream(stream):
        launch(0)
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for i in range(launches):
                launch(i)
        for _ in range(3):
            g.replay()
        stream.synchronize()
    return g


def replay_us(g, launches: int, stream) -> float:
    with torch.cuda.stream(stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        g.replay()
        e1.record(stream)
        stream.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def time_three(fa, fb, fc, launches: int, reps: int, stream) -> dict:
    import benchlib
    graphs = [capture(f, launches, stream) for f in (fa, fb, fc)]
    ts = [[], [], []]
    for _ in range(reps):
        for g, t in zip(graphs, ts):
            t.append(replay_us(g, launches, stream))
    med = [benchlib.median(t) for t in ts]
    spread = [(max(t) - min(t)) / benchlib.median(t) for t in ts]
    return {"a_us": round(med[0], 2), "b_us": round(med[1], 2), "c_us": round(med[2], 2), "a_over_b": round(med[0] / med[1], 3),
            "a_over_c": round(med[0] / med[2], 3), "spread": [round(s, 3) for s in spread], "launches": launches}


def timing(reps: int, quick: bool) -> list:
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to report without one"
    stream = torch.cuda.Stream()
    rows = []
    for k in ((1024,) if quick else KS):
        for m in ((16,) if quick else MS):
            copies = min(MAX_LAUNCHES, max(2, -(-ROTATE_BYTES // (2 * m * k)) + 1))
            gen = torch.Generator(device="cuda").manual_seed(m + k)
            xs = [torch.randn((m, k), device="cuda", generator=gen).bfloat16() for _ in range(copies)]
            w = (1.0 + 0.1 * torch.randn(k, device="cuda", generator=gen)).bfloat16()
            for fmt in FMTS:
                for block in BLOCKS:
                    cells = [("quantize", lambda i: pk.quantize_activations(xs[i % copies], fmt, hadamard=block),
                              lambda i: pk.quantize_activations(xs[i % copies], fmt),
                              lambda i: pk.quantize_activations(pk.hadamard_rotate(xs[i % copies], block), fmt))]
                    if k == 8192 or quick:
                        def chain(i):
                            _, y = pk.rmsnorm_quantize(xs[i % copies], w, EPS, fmt, return_normed=True)
                            return pk.quantize_activations(pk.hadamard_rotate(y, block), fmt)
                        cells.append(("rmsnorm", lambda i: pk.rmsnorm_quantize(xs[i % copies], w, EPS, fmt, hadamard=block),
                                      lambda i: pk.rmsnorm_quantize(xs[i % copies], w, EPS, fmt), chain))
                    for name, fa, fb, fc in cells:
                        row = {"entry": name, "M": m, "K": k, "fmt": fmt, "B": block, **time_three(fa, fb, fc, copies, reps, stream)}
                        print(json.dumps(row), flush=True)
                        rows.append(row)
            del xs
            torch.cuda.empty_cache()
    return rows


# --- the report -----------------------------------------------------------------------------------------------------------------------------------------

def report(acc: dict, rows: list, date: str) -> str:
    out = ["# Block-Hadamard rotation in the activation quantisers: price and gain", "",
           f"Session of {date}; `tools/hadamard_quant_bench.py` (its docstring states the rule: three HIP graphs per cell over rotating inputs, replayed",
           "alternately in one process, device events, median per launch; spread = (max - min) / median of a side's replays).", "",
           "## Accuracy (CPU twins, no GPU involved)", "",
           f"MLP block, hidden {acc['hidden']}, intermediate {acc['intermediate']}, {acc['m']} tokens, {acc['outlier_columns']} input columns x {acc['outlier_factor']},",
           "checkpoint-like weights (`tools/quantize_weights.py`), MXFP4 weights and MXFP4 activations into gate_up and into down; errors relative to the",
           "rms of the bf16-weight block's output.", "",
           "| rotation | MXFP4 weight format alone | MXFP4 activations on top | total against the bf16-weight block |", "|---|---|---|---|"]
    for block, r in acc["rows"].items():
        out.append(f"| {'none' if block == '0' else 'B = ' + block} | {100 * r['weight_quantisation_vs_bf16_weights']:.1f} % | "
                   f"{100 * r['activation_quantisation_vs_exact_fp4']:.1f} % | {100 * r['total_vs_bf16_weight_block']:.1f} % |")
    out += ["", "## Time (MI355X, bf16)", "",
            "(a) rotated quantiser, one launch; (b) unrotated quantiser; (c) `hadamard_rotate` + quantiser, the chain (a) replaces.  us per launch.", "",
            "| entry | M | K | format | B | (a) | (b) | (c) | a / b | a / c | spread a, b, c |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['entry']} | {r['M']} | {r['K']} | {r['fmt']} | {r['B']} | {r['a_us']:.2f} | {r['b_us']:.2f} | {r['c_us']:.2f} | {r['a_over_b']:.2f} | "
                   f"{r['a_over_c']:.2f} | " + ", ".join(f"{100 * s:.0f} %" for s in r["spread"]) + " |" + (" SLOWER THAN THE CHAIN" if r["a_over_c"] > 1 else ""))
    worst_c, worst_b = max(r["a_over_c"] for r in rows), max(r["a_over_b"] for r in rows)
    out += ["", f"Condition a / c <= 1: the worst cell is {worst_c:.2f}" + (" -- MISSED." if worst_c > 1 else " -- met in every cell.") +
            f"  The price of the rotation, a / b, is at most {worst_b:.2f} (no bar: its first measurement).", ""]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--quick", action="store_true", help="one small shape: a rehearsal of the script, not a measurement")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default="")
    ap.add_argument("--report", nargs=2, metavar=("ACCURACY_JSON", "TIME_JSON"))
    ap.add_argument("--date", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hadamard_quant.md"))
    args = ap.parse_args()
    if args.report:
        assert args.date, "--report needs --date (the session's date)"
        text = report(json.loads(Path(args.report[0]).read_text()), json.loads(Path(args.report[1]).read_text()), args.date)
        Path(args.out).write_text(text)
        print(text)
        return
    result = accuracy() if args.accuracy else timing(args.reps, args.quick)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()

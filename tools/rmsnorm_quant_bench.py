#!/usr/bin/env python3
"""tools/rmsnorm_quant_bench.py -- time petit_kernel.rmsnorm_quantize against the chain it replaces: (x + r,) torch.nn.functional.rms_norm,
petit_kernel.quantize_activations.

    python tools/rmsnorm_quant_bench.py [--reps 20] [--quick] [--out profiles/rmsnorm_quant_session.json]

bf16, K = 8192, M in {512, 4314, 16375}, the three activation formats, with and without a residual.  Both sides are captured into HIP graphs of
`copies` launches over rotating inputs (together beyond the 256 MB Infinity Cache) and replayed ALTERNATELY in one process: a replay of (a), a
replay of (b), `reps` times; reported per launch: median and minimum, and the spread (max - min) / median of each side's replays.
Bytes of (a): what the fused launch has to move -- x (and r) in, the updated residual out when there is one, the quantised bytes out, the weight
row once -- over its time, as a fraction of the copy rate DESIGN.md quotes (6.29 TB/s).  The 16-bit y is not written on either side's account:
(b) writes and re-reads it because it has to.  Run it twice (two processes) for the session-to-session spread; --merge makes the table."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "petit-kernel_amd"))

import petit_kernel as pk  # noqa: E402

COPY_CEILING_TBS = 6.29
K = 8192
MS = (512, 4314, 16375)
FMTS = {"mxfp8": 8, "mxfp6": 6, "mxfp4": 4}
ROTATE_BYTES = 320 << 20
EPS = 1e-6


def fused_bytes(m: int, k: int, fmt: str, with_res: bool) -> int:
    qa = m * (k // 8 * FMTS[fmt]) + m * (k // 32)
    return 2 * m * k * (3 if with_res else 1) + qa + 2 * k


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


def stats(xs):
    s = sorted(xs)
    med = s[len(s) // 2]
    return round(med, 2), round(s[0], 2), round((s[-1] - s[0]) / med, 3)


def merge(paths, out):
    """Two (or more) session files -> the markdown table of profiles/rmsnorm_quant.md on stdout / in `out`."""
    sessions = [json.loads(Path(p).read_text()) for p in paths]
    lines = ["| M | format | residual | " + " | ".join(f"(a) fused us, s{i + 1}" for i in range(len(sessions))) + " | " +
             " | ".join(f"(b) chain us, s{i + 1}" for i in range(len(sessions))) + " | (b) / (a) | (b) session spread | (a) of 6.29 TB/s |",
             "|---|---|---|" + "---|" * (2 * len(sessions) + 3)]
    for rows in zip(*sessions):
        r0 = rows[0]
        assert all((r["M"], r["fmt"], r["residual"]) == (r0["M"], r0["fmt"], r0["residual"]) for r in rows)
        a = [r["fused_us"] for r in rows]
        b = [r["chain_us"] for r in rows]
        spread = (max(b) - min(b)) / min(b)
        slower = min(a) > max(b) * (1 + spread)
        lines.append(f"| {r0['M']} | {r0['fmt']} | {'yes' if r0['residual'] else 'no'} | " + " | ".join(f"{v:.1f}" for v in a) + " | " +
                     " | ".join(f"{v:.1f}" for v in b) + f" | {sum(b) / sum(a):.2f} | {100 * spread:.1f} % | " +
                     f"{max(r['fused_of_copy_ceiling'] for r in rows):.2f} |" + (" SLOWER" if slower else ""))
    text = "\n".join(lines) + "\n"
    if out:
        Path(out).write_text(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="small shapes: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default="")
    ap.add_argument("--merge", nargs="+", default=None, help="session files -> the markdown table")
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out)
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to report without one"
    stream = torch.cuda.Stream()
    rows = []
    k = 1024 if args.quick else K
    for m in ((64,) if args.quick else MS):
        copies = max(2, -(-ROTATE_BYTES // (2 * m * k)) + 1)
        gen = torch.Generator(device="cuda").manual_seed(m)
        xs = [torch.randn((m, k), device="cuda", generator=gen).bfloat16() for _ in range(copies)]
        rs = [torch.randn((m, k), device="cuda", generator=gen).bfloat16() for _ in range(copies)]
        w = (1.0 + 0.1 * torch.randn(k, device="cuda", generator=gen)).bfloat16()
        for fmt in FMTS:
            for with_res in (True, False):
                def fused(i):
                    return pk.rmsnorm_quantize(xs[i % copies], w, EPS, fmt, residual=rs[i % copies] if with_res else None)

                def chain(i):
                    h = xs[i % copies] + rs[i % copies] if with_res else xs[i % copies]
                    return h, pk.quantize_activations(torch.nn.functional.rms_norm(h, (k,), w, EPS), fmt)

                ga, gb = capture(fused, copies, stream), capture(chain, copies, stream)
                ta, tb = [], []
                for _ in range(args.reps):
                    ta.append(replay_us(ga, copies, stream))
                    tb.append(replay_us(gb, copies, stream))
                (a_med, a_min, a_spread), (b_med, b_min, b_spread) = stats(ta), stats(tb)
                nbytes = fused_bytes(m, k, fmt, with_res)
                row = {"M": m, "K": k, "fmt": fmt, "residual": with_res, "copies": copies, "fused_us": a_med, "fused_min_us": a_min,
                       "fused_spread": a_spread, "chain_us": b_med, "chain_min_us": b_min, "chain_spread": b_spread,
                       "chain_over_fused": round(b_med / a_med, 2), "fused_GBps": round(nbytes / a_med / 1e3, 1),
                       "fused_of_copy_ceiling": round(nbytes / a_med / 1e6 / COPY_CEILING_TBS, 3)}
                print(json.dumps(row), flush=True)
                rows.append(row)
                del ga, gb
        del xs, rs
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""tools/moe_combine_norm_bench.py -- time petit_kernel.moe_combine_rmsnorm against the launches it replaces.

    python tools/moe_combine_norm_bench.py [--reps 20] [--quick] [--out profiles/moe_combine_norm_session.json]
    python tools/moe_combine_norm_bench.py --merge s1.json s2.json [--out table.md]

bf16, (H, topk) in {(2048, 8), (4096, 2), (7168, 9), (2880, 4)}, T in {1, 16, 64, 512, 4096}, fmt 'mxfp8' and None (H = 2880: None only; the
quantised layout needs whole k-tiles).  Side (a) is the fused launch with a residual.  Side (b) is moe_combine then
rmsnorm_quantize(residual=...), and for fmt None moe_combine, x + r and torch.nn.functional.rms_norm: what a caller ran before.

Both sides are captured into HIP graphs of `copies` launches, each launch on inputs of its own, and replayed ALTERNATELY in one process: a replay
of (a), a replay of (b), `reps` times.  Before every replay a 512 MB buffer is overwritten (outside the timed span), so no launch finds its
inputs in the L2 or the 256 MB Infinity Cache whatever T is: at T = 1 a copy is 32 KB, and rotating copies alone would need ten thousand graph
nodes to get past the cache.  Reported per launch (per chain of launches on side (b)): the median and minimum over the replays and the spread
(max - min) / median of each side.  Run it twice (two processes) for the session-to-session spread; --merge makes the table and applies the
condition: (a) not slower than (b) by more than (b)'s own session-to-session spread, and faster at T <= 64."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "petit-kernel_amd"))

import petit_kernel as pk  # noqa: E402

CELLS = ((2048, 8), (4096, 2), (7168, 9), (2880, 4))
TS = (1, 16, 64, 512, 4096)
NUM_EXPERTS = 128
ROTATE_BYTES = 320 << 20
FLUSH_BYTES = 512 << 20
MAX_COPIES = 64
EPS = 1e-6


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


def replay_us(g, launches: int, stream, flush) -> float:
    with torch.cuda.stream(stream):
        flush.add_(1)                      # evicts both caches; ordered before the timed span on the same stream
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
    """Two (or more) session files -> the markdown table of profiles/moe_combine_norm.md on stdout / in `out`."""
    sessions = [json.loads(Path(p).read_text()) for p in paths]
    n = len(sessions)
    lines = ["| H | topk | T | fmt | " + " | ".join(f"(a) fused us, s{i + 1}" for i in range(n)) + " | " +
             " | ".join(f"(b) chain us, s{i + 1}" for i in range(n)) + " | (b) / (a) | (b) session spread | verdict |",
             "|---|---|---|---|" + "---|" * (2 * n + 3)]
    failed = []
    for rows in zip(*sessions):
        r0 = rows[0]
        key = (r0["H"], r0["topk"], r0["T"], r0["fmt"])
        assert all((r["H"], r["topk"], r["T"], r["fmt"]) == key for r in rows)
        a = [r["fused_us"] for r in rows]
        b = [r["chain_us"] for r in rows]
        spread = (max(b) - min(b)) / min(b)
        slower = max(a) > min(b) * (1 + spread)                     # every session of (a) against the best of (b), widened by (b)'s own spread
        not_faster = r0["T"] <= 64 and not max(a) < min(b)
        verdict = "SLOWER" if slower else "NOT FASTER" if not_faster else "ok"
        if verdict != "ok":
            failed.append(key)
        lines.append(f"| {key[0]} | {key[1]} | {key[2]} | {key[3]} | " + " | ".join(f"{v:.1f}" for v in a) + " | " + " | ".join(f"{v:.1f}" for v in b) +
                     f" | {sum(b) / sum(a):.2f} | {100 * spread:.1f} % | {verdict} |")
    text = "\n".join(lines) + f"\n\ncells that miss the condition: {failed if failed else 'none'}\n"
    if out:
        Path(out).write_text(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="two small cells: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default="")
    ap.add_argument("--merge", nargs="+", default=None, help="session files -> the markdown table")
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out)
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to report without one"
    stream = torch.cuda.Stream()
    flush = torch.zeros(FLUSH_BYTES // 4, dtype=torch.int32, device="cuda")
    rows = []
    cells = ((2048, 8), (2880, 4)) if args.quick else CELLS
    for hid, topk in cells:
        for T in ((1, 64) if args.quick else TS):
            per_copy = 2 * T * hid * (topk + 1)                     # the slot rows and the residual
            copies = max(2, min(MAX_COPIES, -(-ROTATE_BYTES // per_copy) + 1))
            gen = torch.Generator(device="cuda").manual_seed(T + hid)
            slots = [torch.randn((T * topk, hid), device="cuda", generator=gen).bfloat16() for _ in range(copies)]
            rs = [torch.randn((T, hid), device="cuda", generator=gen).bfloat16() for _ in range(copies)]
            w = (1.0 + 0.1 * torch.randn(hid, device="cuda", generator=gen)).bfloat16()
            tw = torch.rand((T, topk), device="cuda", generator=gen)
            ids = torch.randint(0, NUM_EXPERTS, (T, topk), device="cuda", generator=gen, dtype=torch.int32)
            for fmt in ((None,) if hid % 256 else ("mxfp8", None)):
                def fused(i):
                    return pk.moe_combine_rmsnorm(slots[i % copies], tw, ids, NUM_EXPERTS, w, EPS, fmt, residual=rs[i % copies])

                def chain(i):
                    c = pk.moe_combine(slots[i % copies], tw, ids, NUM_EXPERTS)
                    if fmt:
                        return pk.rmsnorm_quantize(c, w, EPS, fmt, residual=rs[i % copies])
                    h = c + rs[i % copies]
                    return h, torch.nn.functional.rms_norm(h, (hid,), w, EPS)

                ga, gb = capture(fused, copies, stream), capture(chain, copies, stream)
                ta, tb = [], []
                for _ in range(args.reps):
                    ta.append(replay_us(ga, copies, stream, flush))
                    tb.append(replay_us(gb, copies, stream, flush))
                (a_med, a_min, a_spread), (b_med, b_min, b_spread) = stats(ta), stats(tb)
                row = {"H": hid, "topk": topk, "T": T, "fmt": fmt or "none", "copies": copies, "fused_us": a_med, "fused_min_us": a_min,
                       "fused_spread": a_spread, "chain_us": b_med, "chain_min_us": b_min, "chain_spread": b_spread,
                       "chain_over_fused": round(b_med / a_med, 2)}
                print(json.dumps(row), flush=True)
                rows.append(row)
                del ga, gb
            del slots, rs
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()

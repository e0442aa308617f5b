#!/usr/bin/env python3
"""tools/nv_transient_bench.py -- NVFP4 prefill on a per-call MFMA-native image (petit_gemm_nvfp4_native_transient), measured.

    python tools/nv_transient_bench.py builder --shape 57344x8192 [--calls 50]      # builder calls only (run it under rocprofv3, see below)
    python tools/nv_transient_bench.py builder-stats DIR... --out profiles/nv_transient_builder.json
    python tools/nv_transient_bench.py cells [--out profiles/nv_transient_cells.json]

builder: `calls` image builds of one (N, K) weight, each from a different copy of the packed tensors (rotating over >= 1.3 GB, as benchlib does,
so nothing is served by the Infinity Cache).  Run it alone under
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python ... builder --shape NxK --meta-dir DIR`;
builder-stats reads the kernel_stats CSVs of those runs and reports the builder's effective bandwidth: (bytes read + bytes written) / mean kernel time,
read = N K / 2 + N K / 16 (packed weights and e4m3 scales), written = petit_nvfp4_native_image_bytes.

cells: exact bf16 x NVFP4 (PETIT_SOLUTION_AUTO), the attached image and the transient call, with MXFP8 and MXFP6 activations, at the M of the
issue on Llama-3-70B's four layers; graph replays over rotated weight copies (benchlib.time_graph).  Reports the crossover M per shape: the
smallest measured M from which transient x MXFP8 is faster than exact at every larger measured M.
"""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "petit-kernel_amd"))
sys.path.insert(0, str(ROOT / "tools"))

SHAPES = {"qkv": (10240, 8192), "o": (8192, 8192), "gate_up": (57344, 8192), "down": (8192, 28672)}
TP8 = {"qkv_tp8": (1280, 8192), "o_tp8": (8192, 1024), "gate_up_tp8": (7168, 8192), "down_tp8": (8192, 3584)}
MS = (256, 512, 1024, 2084, 4314, 16375)
COPY_CEILING_GBS = 6290.0     # measured device-to-device copy ceiling of MI355X (profiles/r06_summary.md)


def builder_bytes(n: int, k: int) -> tuple:
    from petit_kernel import _lib
    return n * k // 2 + n * k // 16, int(_lib.lib.petit_nvfp4_native_image_bytes(k, n))


def run_builder(n: int, k: int, calls: int) -> None:
    import torch
    import benchlib
    from petit_kernel import _lib
    dev = torch.device("cuda", 0)
    w = benchlib.Weights("nv", n, k, 1280, dev)
    img = torch.empty(int(_lib.lib.petit_nvfp4_native_image_bytes(k, n)), dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for i in range(calls):
        b, sp = w[i]
        rc = _lib.lib.petit_nvfp4_native_image(C.c_void_p(img.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(sp.data_ptr()), k, n, stream)
        assert rc == 0, rc
    torch.cuda.synchronize()


def builder_stats(dirs: list, out: str) -> None:
    rows = []
    for d in dirs:
        meta = json.loads((Path(d) / "shape.json").read_text())
        stats = sorted(Path(d).rglob("*kernel_stats.csv"))
        assert stats, f"no kernel_stats.csv under {d}"
        with open(stats[0]) as f:
            recs = [r for r in csv.DictReader(f) if "nv6_image_kernel" in r["Name"]]
        assert recs, f"no builder kernel in {stats[0]}"
        r = recs[0]
        calls, avg_ns = int(r["Calls"]), float(r["AverageNs"])
        rd, wr = builder_bytes(meta["n"], meta["k"])
        gbs = (rd + wr) / avg_ns
        rows.append({"shape": meta["name"], "n": meta["n"], "k": meta["k"], "calls": calls, "kernel_us": avg_ns / 1e3, "bytes_read": rd,
                     "bytes_written": wr, "gbs": gbs, "of_copy_ceiling": gbs / COPY_CEILING_GBS})
        print(json.dumps(rows[-1]))
    Path(out).write_text(json.dumps({"copy_ceiling_gbs": COPY_CEILING_GBS, "rows": rows}, indent=1) + "\n")


def cells(out: str, ms, shapes) -> None:
    import torch
    import benchlib
    from petit_kernel import _lib
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    L = _lib.lib
    rows = []
    for name in shapes:
        n, k = SHAPES[name]
        w = benchlib.Weights("nv", n, k, 1280, dev)
        for m in ms:
            g = benchlib.Gemm(w, m, torch.bfloat16, dev)
            row = {"shape": name, "n": n, "k": k, "m": m, "exact_us": g.time(_lib.PETIT_SOLUTION_AUTO, stream)["us"]}
            for fmt, sid in (("mxfp8", _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP8), ("mxfp6", _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP6)):
                row[f"attached_{fmt}_us"] = g.time(sid, stream)["us"]
                w.detach_native()
                need = int(L.petit_gemm_nvfp4_native_transient_workspace_bytes(C.byref(g.hints), m, n, k, C.c_uint64(sid), None, None))
                ws = torch.empty(need, dtype=torch.uint8, device=dev)

                def launch(i, sid=sid, ws=ws, need=need):
                    b, sp = w[i]
                    rc = L.petit_gemm_nvfp4_native_transient(C.c_void_p(g.c.data_ptr()), C.c_void_p(g.a.data_ptr()), C.c_void_p(b.data_ptr()),
                                                             C.c_void_p(sp.data_ptr()), C.c_void_p(g.gs.data_ptr()), m, n, k, C.byref(g.hints),
                                                             C.c_uint64(sid), None, None, C.c_void_p(ws.data_ptr()), C.c_uint64(need),
                                                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
                    if rc != 0:
                        raise RuntimeError(f"transient rc={rc}")
                launches = int(max(10, min(200, 3000.0 / max(row["exact_us"], 1.0))))
                row[f"transient_{fmt}_us"] = benchlib.median(benchlib.time_graph(launch, launches, 7, stream))
                del ws
            row["transient_vs_attached_mxfp8"] = row["transient_mxfp8_us"] / row["attached_mxfp8_us"]
            row["transient_vs_exact_mxfp8"] = row["transient_mxfp8_us"] / row["exact_us"]
            print(json.dumps(row), flush=True)
            rows.append(row)
            Path(out).write_text(json.dumps({"ms": list(ms), "rows": rows}, indent=1) + "\n")   # (partial results survive an interrupted run)
        w.detach_native()
        del w
        torch.cuda.empty_cache()
    cross = {}
    for name in shapes:
        rs = sorted((r for r in rows if r["shape"] == name), key=lambda r: r["m"])
        cm = None
        for r in reversed(rs):
            if r["transient_mxfp8_us"] < r["exact_us"]:
                cm = r["m"]
            else:
                break
        cross[name] = cm
    Path(out).write_text(json.dumps({"ms": list(ms), "crossover_m_mxfp8": cross, "rows": rows}, indent=1) + "\n")
    print(json.dumps({"crossover_m_mxfp8": cross}))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    b = sub.add_parser("builder")
    b.add_argument("--shape", required=True, help="NxK")
    b.add_argument("--name", default="")
    b.add_argument("--calls", type=int, default=50)
    b.add_argument("--meta-dir", default="", help="write shape.json here (read by builder-stats)")
    s = sub.add_parser("builder-stats")
    s.add_argument("dirs", nargs="+")
    s.add_argument("--out", default=str(ROOT / "profiles" / "nv_transient_builder.json"))
    c = sub.add_parser("cells")
    c.add_argument("--out", default=str(ROOT / "profiles" / "nv_transient_cells.json"))
    c.add_argument("--ms", default=",".join(map(str, MS)))
    c.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    if a.cmd == "builder":
        n, k = map(int, a.shape.lower().split("x"))
        if a.meta_dir:
            Path(a.meta_dir).mkdir(parents=True, exist_ok=True)
            (Path(a.meta_dir) / "shape.json").write_text(json.dumps({"name": a.name or a.shape, "n": n, "k": k}))
        run_builder(n, k, a.calls)
    elif a.cmd == "builder-stats":
        builder_stats(a.dirs, a.out)
    else:
        cells(a.out, [int(x) for x in a.ms.split(",")], a.shapes.split(","))


if __name__ == "__main__":
    main()

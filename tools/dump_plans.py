#!/usr/bin/env python3
"""Dump what the host-side queries answer, one line per (query, problem), to compare two builds of the library:

    PETIT_AMD_LIB=<libpetit_amd.so of build A> python tools/dump_plans.py a.txt
    PETIT_AMD_LIB=<libpetit_amd.so of build B> python tools/dump_plans.py b.txt && diff a.txt b.txt

Needs no GPU.  Problems: every (N, K) of csrc/tuned_gfx950.inc plus untabulated neighbours (N +- 256, K +- 256 / 512) of every eighth one, M from decode to
prefill, the four families, no epilogue / SiLU-mul / SwiGLU-OAI, and as solution_id PETIT_SOLUTION_AUTO, the three native sentinels and every enumerated
id with split nibbles 1, 2, 4, 8 (native class enabled); the MoE queries at 8, 128 and 256 experts.  Queries: petit_gemm_resolve_solution (with all the
scratch, and for the sentinels / AUTO also with none), petit_gemm_workspace_bytes_ex, petit_gemm_row_split (petit_gemm_auto_row_split), petit_gemm_get_solutions,
petit_gemm_moe_resolve_solution, petit_gemm_native_moe_resolve_solution / _workspace_bytes, and the tuner's candidate list."""
import ctypes as C
import re
import sys
from multiprocessing import Pool
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "petit-kernel_amd"))
MS = (1, 2, 4, 8, 16, 32, 48, 64, 128, 256, 512, 600, 1024, 1100, 2084, 2200, 4314, 8192, 16375)
EXPERTS = (8, 128, 256)
# petit_amd::tune_candidates(int, int, int, unsigned, unsigned, unsigned, size_t, uint64_t *, uint64_t *, int) (dispatch.hip): the tuner's list has no C
# entry point, so it is reached by its mangled name, which spells that signature -- change one and the other follows (tune_candidates() below says so)
TUNE_CANDIDATES = "_ZN9petit_amd15tune_candidatesEiiijjjmPmS0_i"


def tune_candidates(L):
    try:
        return getattr(L, TUNE_CANDIDATES)
    except AttributeError:
        raise RuntimeError(f"{L._name} exports no {TUNE_CANDIDATES}: petit_amd::tune_candidates (csrc/dispatch.hip) has another signature than "
                           "this tool's TUNE_CANDIDATES spells; update the mangled name (nm -D --defined-only | grep tune_candidates)") from None


def shapes():
    text = (ROOT / "petit-kernel_amd" / "csrc" / "tuned_gfx950.inc").read_text()
    tab = sorted({(int(n), int(k)) for n, k in re.findall(r"^\{\d+, \d+, (\d+)u, (\d+)u,", text, re.M)})
    extra = set()
    for n, k in tab[::8]:
        for dn, dk in ((256, 0), (-256, 0), (0, 256), (0, -256), (0, 512), (0, -512)):
            if n + dn >= 256 and k + dk >= 256 and (n + dn, k + dk) not in tab:
                extra.add((n + dn, k + dk))
    return tab + sorted(extra)


def dump_shape(nk):
    from petit_kernel import _lib
    L = _lib.lib
    for fn in ("petit_gemm_resolve_solution", "petit_gemm_workspace_bytes_ex", "petit_gemm_moe_resolve_solution", "petit_gemm_native_moe_resolve_solution",
               "petit_gemm_native_moe_workspace_bytes"):
        getattr(L, fn).restype = C.c_uint64
    L.petit_enable_native_fp4(1)
    candidates = tune_candidates(L)
    n, k = nk
    out = []
    u64 = C.c_uint64
    auto_ids = (_lib.PETIT_SOLUTION_AUTO, _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP8, _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP6, _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP4)
    for at in (_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP16):
        for bt in (_lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_MXFP4_E2M1):
            h = _lib.SolutionHints(at, bt, at, 0)
            hp = C.byref(h)
            for m in MS:
                cnt = C.c_uint(0)
                L.petit_gemm_get_solutions(hp, m, n, k, None, C.byref(cnt))
                buf = (C.c_uint64 * max(1, cnt.value))()
                L.petit_gemm_get_solutions(hp, m, n, k, buf, C.byref(cnt))
                sols = list(buf[:cnt.value])
                key = f"{at} {bt} {m} {n} {k}"
                out.append(f"sols {key} " + " ".join(f"{s:x}" for s in sols))
                for klass in (0, 8, 6, 4):
                    ids, needs = (C.c_uint64 * 512)(), (C.c_uint64 * 512)()
                    c = candidates(at, bt, klass, m, n, k, u64(1 << 62), ids, needs, 512)
                    out.append(f"cand {key} {klass} " + " ".join(f"{ids[i]:x}:{needs[i]}" for i in range(max(0, c))))
                ids = list(auto_ids) + [(s & ~(0xF << 60)) | (sk << 60) for s in sols for sk in (1, 2, 4, 8)]
                for act in (0, 1, 2):
                    epi = _lib.Epilogue(None, act, 0)
                    ep = C.byref(epi) if act else None
                    for sid in ids:
                        r = L.petit_gemm_resolve_solution(hp, m, n, k, u64(sid), ep, u64(1 << 62))
                        w = L.petit_gemm_workspace_bytes_ex(hp, m, n, k, u64(sid), ep)
                        rs = L.petit_gemm_row_split(hp, m, n, k, u64(sid), ep)
                        out.append(f"resolve {key} {act} {sid:x} {r:x} need {w} rows {rs}")
                    for sid in auto_ids:
                        for ws in (0, L.petit_native_workspace_bytes(m, k)):
                            r = L.petit_gemm_resolve_solution(hp, m, n, k, u64(sid), ep, u64(ws))
                            out.append(f"resolve {key} {act} {sid:x} ws{ws} {r:x}")
                    for e in EXPERTS:
                        for sid in auto_ids:
                            r = L.petit_gemm_moe_resolve_solution(hp, e, m, n, k, u64(sid), ep)
                            rn = L.petit_gemm_native_moe_resolve_solution(hp, e, m, n, k, u64(sid), ep, None)
                            wn = L.petit_gemm_native_moe_workspace_bytes(hp, e, m, n, k, u64(sid), ep, None)
                            out.append(f"moe {key} {act} E{e} {sid:x} {r:x} native {rn:x} {wn}")
    return out


if __name__ == "__main__":
    with Pool(int(sys.argv[2]) if len(sys.argv) > 2 else 8) as pool, open(sys.argv[1], "w") as f:
        for lines in pool.imap(dump_shape, shapes()):
            f.write("\n".join(lines) + "\n")

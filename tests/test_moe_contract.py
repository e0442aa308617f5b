"""The routed-expert (MoE) launches, bit for bit: the slot -> (expert, m-block) map over all 16 chunks of 64 experts, the row limits of an expert,
the per-expert operand bases (weights, block scales, gs[e], bias[e]) and the write contract (rows of no expert are never written, nothing is
written outside C or past the declared workspace).

Method: that of test_exact_contract.py.  The stacked [E * n, k] weights and the [m, k] activations are exact_problem's regimes A / B / G, so every
product and partial sum is exact in fp32 in ANY order and acc is one number whatever kernel, tile or slot computes it; gs[e] is the regime's gs
times 2^j (j from {-1, 0, 1}, neighbouring experts differ) and the bias [E, n] is drawn per expert, so a tile that takes a neighbour's weights,
gs or bias, or a last row computed from the next expert's activations, changes expected bits (the teeth test shows it per expert).  Tolerance:
none; the gated epilogues are judged by test_gated_contract's band and caps.

Which row belongs to which expert is stated ONCE here, in numpy (row_ownership): every offset clamped into [0, m], then the running maximum.  It is
the rule both device statements (moe_locate of csrc/gemm_moe.hpp; moe_expert_rows of csrc/petit_internal.h, the image builder's) are held to.
Every malformed case hands the launch exactly E + 1 allocated int32 offsets, only their values are wrong: moe_locate clamps each raw value with
min(max(raw, 0), m), takes the running maximum and carries `lo` from chunk to chunk before any base address is formed from them.

The GPU tests launch through the C ABI into caller-owned buffers: C sits between two guards and is filled with the output type's NaN poison before
EVERY launch, so an owned output nobody wrote, an unowned output somebody wrote and a write outside C all show; the native class's workspace is the
declared bytes followed by a poisoned guard.
"""
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch

from test_exact_contract import ACTIVATION_NAMES, DEV, FAMILIES, GUARD, POISON, Problem, exact_problem, pk, rne_bits, to_bits  # noqa: F401
from test_gated_contract import CAP, expect
from test_moe_nv_transient import SKIP_ROUTINGS, _has_rows, _many_expert_routings

ALL_BMS = (1, 2, 4, 8, 16, 32, 64, 128, 256)
ID_MS = (1, 2, 4, 8, 16, 64, 512)
# K -> s for (NVFP4, MXFP4) weights, regime G's gs = 3 * 2^-s: test_gated_contract.G_SHIFT with K = 768 between its neighbours, and at K = 2048 one
# step narrower for NVFP4 (9, not 8): a third of the experts carry gs * 2, and at s = 8 their SwiGLU-OAI outputs in fp16 are subnormal for 7 % of
# a problem whatever the seed (the float64 formula alone, over 12 seeds: 4 % .. 10 %), above the 4 % cap; at s = 9 the widest expert has G_SHIFT's gs
MOE_G_SHIFT = {256: (7, 7), 768: (8, 8), 2048: (9, 9)}
NATIVE_BM = 128


# --- 1. the routings ------------------------------------------------------------------------------------------------------------------------

def row_ownership(offsets, m):
    """-> (owner int64 [m]: the expert of grouped row r, -1 for a row of no expert; spans [(lo_e, hi_e)] per expert).  The rule of the MoE launches
    written independently of the library (test_moe_nv_transient._has_rows, extended to rows): every offset clamped into [0, m], the running
    maximum, row r is expert e's when lo_e <= r < hi_e."""
    lo = min(max(int(offsets[0]), 0), m)
    owner, spans = np.full(m, -1, dtype=np.int64), []
    for e in range(len(offsets) - 1):
        hi = max(lo, min(max(int(offsets[e + 1]), 0), m))
        owner[lo:hi] = e
        spans.append((lo, hi))
        lo = hi
    return owner, spans


def _from_counts(counts):
    off = [0]
    for c in counts:
        off.append(off[-1] + int(c))
    return off, off[-1]


def _sparse(E, rows):
    counts = [0] * E
    for e, c in rows.items():
        counts[e] = c
    return _from_counts(counts)


def routings(bm):
    """{name: (E, offsets, m, regimes)}: the smallest routings that reach each mechanism, for a kernel of bm rows per workgroup."""
    out = {"edges": (7,) + _from_counts([1, 0, bm - 1, bm, bm + 1, 2 * bm + 1, 0]) + ("AB",),     # (bm = 1: bm - 1 is one more empty expert)
           "one-each": (65,) + _from_counts([1] * 65) + ("B",),
           "chunks130": (130,) + _sparse(130, {0: 1, 62: bm + 1, 65: 1, 126: bm + 1, 129: 1}) + ("B",),
           "chunks256": (256,) + _sparse(256, {0: bm + 1, 62: 1, 65: bm + 1, 126: 1, 129: bm + 1, 255: 1}) + ("B",),
           "last-chunk": (1024,) + _sparse(1024, {0: 3, 511: 1, 960: 2, 1023: 5}) + ("B",),
           "last-expert": (1024,) + _sparse(1024, {1023: 11}) + ("B",),
           "fewer-rows": (1024,) + _sparse(1024, {64: 1, 700: 1, 1023: 1}) + ("B",)}
    off, m = _from_counts([2, 0, 3, 1, 0, 4, 1, 2])
    out["short"] = (8, off, m + 5, "B")                                                         # offsets[E] = m - 5
    for i, (offsets, m) in enumerate(SKIP_ROUTINGS):
        if m and any(_has_rows(offsets, m)):
            out[f"malformed5-{i}"] = (5, list(offsets), m, "B")
    bad, m = _many_expert_routings(130, 130)[1]
    out["malformed130"] = (130, [int(v) for v in bad], m, "B")
    return out


GROUPS = {"edges": ("edges",), "one-each": ("one-each",), "chunks": ("chunks130", "chunks256"),
          "last-chunk": ("last-chunk", "last-expert", "fewer-rows"),
          "malformed": ("short", "malformed130") + tuple(f"malformed5-{i}" for i in (0, 1, 3, 4, 5, 6))}
BM_DEPENDENT = ("edges", "chunks130", "chunks256")


def shapes(kind, E, name, wide=False):
    """[(n, k)] of a routing: E >= 130 one tile of N and one span (1024 experts' weights are 4 MB); else ragged n-tile counts and two span sizes
    (MXFP4: both sides of K % 512), `edges` also K = 256, the span size of the many-expert cases."""
    if E >= 130:
        return [(32 if kind == "mx" or wide else 16, 256)]
    n = 288 if kind == "mx" or wide else 272                                                   # (wide: the gated epilogues and the native image need n % 32 == 0)
    return [(n, k) for k in ((256, 768, 2048) if name == "edges" else (768, 2048))]


def tiles(spans, bm):
    return [-(-(hi - lo) // bm) for lo, hi in spans]


def test_routings_cover_what_they_claim():
    """Which experts own rows, in which 64-chunk, and that the tiles of every routing fit the grid's slots for every rows-per-workgroup."""
    for bm in ALL_BMS:
        R = routings(bm)
        assert sorted(sum(GROUPS.values(), ())) == sorted(R)
        for name, (E, offsets, m, _) in R.items():
            assert len(offsets) == E + 1, name                                                 # exactly E + 1 offsets, whatever their values
            owner, spans = row_ownership(offsets, m)
            assert [hi > lo for lo, hi in spans] == _has_rows(offsets, m), name
            assert sum(hi - lo for lo, hi in spans) == int((owner >= 0).sum()) and all(0 <= lo <= hi <= m for lo, hi in spans), name
            for b in ALL_BMS:
                assert sum(tiles(spans, b)) <= -(-m // b) + min(E, m), (name, bm, b)
        active = lambda name: [e for e, (lo, hi) in enumerate(row_ownership(*R[name][1:3])[1]) if hi > lo]
        rows = lambda name: [hi - lo for lo, hi in row_ownership(*R[name][1:3])[1]]
        assert rows("edges") == [1, 0, bm - 1, bm, bm + 1, 2 * bm + 1, 0]
        assert tiles(row_ownership(*R["edges"][1:3])[1], bm) == [1, 0, 1 if bm > 1 else 0, 1, 2, 3, 0]   # a full block, a ragged last block, three blocks
        # one row on each of m = E experts: as many tiles as experts, and a second chunk that holds one expert
        assert rows("one-each") == [1] * 65 and sum(tiles(row_ownership(*R["one-each"][1:3])[1], bm)) == 65
        slots = -(-65 // bm) + min(65, 65)
        assert slots - 65 == -(-65 // bm) and (bm < 64 or slots - 65 <= 2)                     # the slots left over: ceil(m / bm), the fewest a routing can leave
        assert active("chunks130") == [0, 62, 65, 126, 129] and active("chunks256") == [0, 62, 65, 126, 129, 255]
        for name in ("chunks130", "chunks256"):
            assert {rows(name)[e] for e in active(name)} == {1, bm + 1} and not any(rows(name)[e] for e in (63, 64, 127, 128))
            assert len({e // 64 for e in active(name)}) == (3 if name == "chunks130" else 4)
        assert active("last-chunk") == [0, 511, 960, 1023] and [e // 64 for e in active("last-chunk")] == [0, 7, 15, 15]
        assert active("last-expert") == [1023] and R["last-expert"][2] == 11
        assert R["fewer-rows"][2] == 3 < 1024 and [e // 64 for e in active("fewer-rows")] == [1, 10, 15]
        E, offsets, m, _ = R["short"]
        assert offsets[E] == m - 5 and list(row_ownership(offsets, m)[0][-5:]) == [-1] * 5 and (row_ownership(offsets, m)[0][:-5] >= 0).all()
        # the malformed routings: the clamp decides; unowned rows exist in front (a first offset that is not 0), behind and nowhere
        E, bad, m, _ = R["malformed130"]
        owner, spans = row_ownership(bad, m)
        assert bad[3] > max(bad[4:70]) and not any(hi > lo for lo, hi in spans[3:70]) and min(bad) < 0 and max(bad) > m
        assert any(hi > lo for lo, hi in spans[:64]) and any(hi > lo for lo, hi in spans[70:128]) and not any(hi > lo for lo, hi in spans[104:])
        assert (row_ownership(*R["malformed5-5"][1:3])[0][:4] == -1).all() and (row_ownership(*R["malformed5-4"][1:3])[0] == 0).all()


# --- 2. the generator and the CPU model ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=3)
def stacked_weights(kind, is_bf16, rows, k, regime, seed, shift):
    """exact_problem's draw of a [rows, k] weight (rows = E * n): one draw serves every routing of the same E, n and K."""
    base = exact_problem(kind, is_bf16, 1, rows, k, regime, seed, shift=shift)
    base.w32, base.checked = base.w.astype(np.float32), set()                                 # (multiples of 1/4 below 32: exact in float32)
    return base


def moe_exact_problem(kind, is_bf16, E, offsets, m, n, k, regime, seed, a_rows=None):
    """-> Problem: the stacked weights (q u8 [E * n, k / 2], s block scale bytes) and the activations of exact_problem's regime (two draws of it, one
    for the stacked [E * n, k] weights and one for the activations: the same code sets, scale sets and densities), a per-expert gs [E] = the
    regime's gs times 2^j, a per-expert bias [E, n] drawn as the regime draws it, the row ownership (owner, spans) and the expected bits `want` u16 [m, n]: the owner's epilogue on an owned
    row, the poison on a row of no expert.  acc_all [m, E * n] holds every grouped row against EVERY expert (the teeth test's wrong-expert mutants).
    a_rows: the activations are a_src [a_rows, k] and grouped row r reads row a_index[r] of it: a gather with repeated tokens, a few indices out of
    range (those rows read zeros); consecutive grouped rows never read the same token."""
    shift = MOE_G_SHIFT[k][kind == "mx"] if regime == "G" else None
    base = stacked_weights(kind, is_bf16, E * n, k, regime, seed, shift)                       # the stacked weights and their block scales
    acts = exact_problem(kind, is_bf16, a_rows or m, 32, k, regime, seed + 1, shift=shift)    # the activations (its 32 weight rows are not used)
    rng = np.random.default_rng([seed, kind == "mx", is_bf16, E, m, n, k, "ABG".index(regime), a_rows or 0, 0x4D6F45])
    P = Problem()
    P.kind, P.is_bf16, P.E, P.offsets, P.m, P.n, P.k, P.regime = kind, is_bf16, E, [int(v) for v in offsets], m, n, k, regime
    P.q, P.s, P.quantum, P.w, P.base = base.q, base.s, base.quantum, base.w32, base
    P.a_src, P.a_src_bits, P.a_index = acts.a, acts.a_bits, None
    if a_rows:
        idx = rng.integers(0, a_rows, m)
        for r in range(1, m):
            if idx[r] == idx[r - 1]:
                idx[r] = (idx[r] + 1) % a_rows
        if m >= 8:
            idx[1], idx[m // 2], idx[m - 3] = a_rows + 5, -1, a_rows
        P.a_index = idx.astype(np.int32)
        inside = (idx >= 0) & (idx < a_rows)
        P.a = np.where(inside[:, None], P.a_src[np.clip(idx, 0, a_rows - 1)], 0.0)
    else:
        P.a = P.a_src
    j = np.empty(E, dtype=np.int64)
    j[0] = rng.integers(-1, 2)
    step = rng.integers(1, 3, E)
    for e in range(1, E):
        j[e] = (j[e - 1] + 1 + step[e]) % 3 - 1                                               # (never its predecessor's)
    P.gs0, P.gs = base.gs, base.gs * 2.0 ** j
    if regime == "A":
        P.bias = None
    elif regime == "B":
        P.bias = rng.integers(-32, 33, (E, n)) * 0.25
    else:
        gate, up = rng.integers(16, 33, (E, n // 2)), rng.integers(24, 33, (E, n // 2)) * rng.choice(np.array([-1, 1]), (E, n // 2))
        P.bias = np.concatenate([gate, up], axis=1) * 2.0 ** -4
    P.bias_bits = None if P.bias is None else to_bits(P.bias, is_bf16)
    P.owner, P.spans = row_ownership(P.offsets, m)
    P.acc_all = P.a @ base.w.T                                                                # float64: exact, see the preconditions
    P.y = np.full((m, n), np.nan)
    P.want = np.full((m, n), POISON[is_bf16], dtype=np.uint16)
    for e, (lo, hi) in enumerate(P.spans):
        if hi > lo:
            P.y[lo:hi] = model_rows(P, e, lo, hi)
            P.want[lo:hi] = rne_bits(P.y[lo:hi], is_bf16)
    return P


def model_rows(P, e, lo, hi, w_of=None, gs_of=None, bias_of=None, a_from=None):
    """y of grouped rows lo .. hi-1 as expert e's: fma(acc, gs[e], bias[e]); the keyword arguments name the expert (or the first row) a mutant takes an
    operand from instead."""
    w_of, gs_of, bias_of = (e if v is None else v for v in (w_of, gs_of, bias_of))
    a_from = lo if a_from is None else a_from
    acc = P.acc_all[a_from:a_from + hi - lo, w_of * P.n:(w_of + 1) * P.n]
    return acc * P.gs[gs_of] + (0.0 if P.bias is None else P.bias[bias_of][None, :])         # (+ 0.0: the fma adds a +0 bias, -0 becomes +0)


@functools.lru_cache(maxsize=2)
def problem(kind, is_bf16, E, offsets, m, n, k, regime, seed=0, a_rows=None):
    return moe_exact_problem(kind, is_bf16, E, list(offsets), m, n, k, regime, seed, a_rows)


def gathered_rows(m):
    return max(2, m - m // 3)                                                                 # a_rows < m (from m = 3 on)


def check_preconditions(P, tag, native=False):
    """Per expert that has rows: what makes "any order gives the same bits" true (test_exact_contract.test_generator_preconditions_and_teeth)."""
    from oracle import oracle as O
    is_bf16 = P.is_bf16
    a16 = O.bf16_bits_to_f32(P.a_src_bits) if is_bf16 else O.f16_bits_to_f32(P.a_src_bits)
    assert np.array_equal(a16.astype(np.float64), P.a_src) and np.array_equal(np.rint(P.a), P.a), tag
    assert np.isin(P.gs / P.gs0, (0.5, 1.0, 2.0)).all() and (P.gs[1:] != P.gs[:-1]).all() and (P.E < 64 or np.unique(P.gs).size == 3), tag
    if P.bias is not None:
        assert (P.bias[1:] != P.bias[:-1]).any(axis=1).all(), tag
    for e, (lo, hi) in enumerate(P.spans):
        if hi == lo:
            continue
        q, s, w = (x[e * P.n:(e + 1) * P.n] for x in (P.q, P.s, P.w))
        a, y = P.a[lo:hi], P.y[lo:hi]
        w64 = w.astype(np.float64)
        if e not in P.base.checked:                                                           # (the weights are shared by the routings of one E, n, K)
            dq = O.dequant_nvfp4(q, s) if P.kind == "nv" else O.dequant_mxfp4(q, s)
            assert np.array_equal(dq, w), (tag, e)                                            # the bytes mean what the model says
            assert np.array_equal(np.rint(w64 / P.quantum), w64 / P.quantum), (tag, e)         # every product a multiple of the quantum
            P.base.checked.add(e)
        assert (np.abs(a) @ np.abs(w64).T).max() / P.quantum < 2 ** 24, (tag, e)               # any partial sum in any association is exact in fp32
        assert np.abs(y).max() < (3e38 if is_bf16 else 65504.0), (tag, e)                      # (y survives float32: rne_bits asserted it)
        assert (y == 0).all() or np.abs(y[y != 0]).min() >= 2.0 ** -14, (tag, e)
        assert not np.any(P.want[lo:hi] == POISON[is_bf16]), (tag, e)
        if native:
            from test_gpu_parity import quantize_act_mxfp4, quantize_act_mxfp6, quantize_act_mxfp8

            def spread(x):
                g = np.abs(x).reshape(x.shape[0], -1, 8)
                low = np.where(g > 0, g, np.inf).min(axis=2)
                return np.where(np.isfinite(low), g.max(axis=2) / np.where(np.isfinite(low), low, 1.0), 1.0).max()
            assert spread(a) * spread(w64) < 2 ** 13, (tag, e)                                # the 8-k spread of the e4m3 products
            for quant in (quantize_act_mxfp8, quantize_act_mxfp6, quantize_act_mxfp4):
                assert np.array_equal(quant(a.astype(np.float32)).astype(np.float64), a), (tag, e, quant.__name__)
    assert (P.want[P.owner < 0] == POISON[is_bf16]).all(), tag


def check_teeth(P, tag):
    """Each wrong operand base and the wrong row limit change at least one expected bit in every expert that has rows (and a neighbour to err to)."""
    b = lambda y: rne_bits(y, P.is_bf16)
    for e, (lo, hi) in enumerate(P.spans):
        if hi == lo or P.E < 2:
            continue
        o = e + 1 if e + 1 < P.E else e - 1                                                   # the neighbouring expert
        want = P.want[lo:hi]
        mutants = {"the neighbour's weights": model_rows(P, e, lo, hi, w_of=o), "the neighbour's gs": model_rows(P, e, lo, hi, gs_of=o)}
        if not P.a[lo:hi].any():
            # the expert's only rows read zeros (an A index out of range): acc is 0 whatever the weights and gs, these two mutants do not concern it
            assert P.a_index is not None and ((P.a_index[lo:hi] < 0) | (P.a_index[lo:hi] >= P.a_src.shape[0])).all() and hi - lo <= 2, (tag, e)
            mutants = {}
        if P.bias is not None:
            mutants["the neighbour's bias"] = model_rows(P, e, lo, hi, bias_of=o)
        for name, y in mutants.items():
            assert (b(y) != want).any(), (tag, e, name)
        if hi < P.m:                                                                          # the last row from the following grouped row's activations
            assert (P.a[hi] != P.a[hi - 1]).any(), (tag, e)
            assert (b(model_rows(P, e, hi - 1, hi, a_from=hi)) != want[-1:]).any(), (tag, e, "last row from the next grouped row")
        if P.regime == "A" and P.a[lo:hi].any():                                              # one k index dropped
            w = P.w[e * P.n:(e + 1) * P.n].astype(np.float64)
            live = np.flatnonzero((P.a[lo:hi] != 0).any(axis=0) & (w != 0).any(axis=0))
            assert live.size, (tag, e)
            for k0 in live[:: max(1, live.size // 4)][:4]:
                rows = P.a[lo:hi, k0] != 0
                changed = (b(P.y[lo:hi] - P.gs[e] * np.outer(P.a[lo:hi, k0], w[:, k0])) != want).any(axis=1)
                assert changed[rows].all(), (tag, e, int(k0))


# --- 3. which ids, which cases ----------------------------------------------------------------------------------------------------------------

def c_hints(kind, is_bf16):
    from petit_kernel import _lib
    a_type = _lib.CXX_DTYPE_BF16 if is_bf16 else _lib.CXX_DTYPE_FP16
    return _lib.SolutionHints(a_type, _lib.CXX_DTYPE_FP4_E2M1 if kind == "nv" else _lib.CXX_DTYPE_MXFP4_E2M1, a_type, 0)


def py_hints(kind, is_bf16):
    import petit_kernel as pkm
    h = pkm.PetitSolutionHints()
    h.a_type = h.c_type = torch.bfloat16 if is_bf16 else torch.float16
    h.b_type = pkm.DataType.float4_e2m1 if kind == "nv" else pkm.DataType.mxfloat4_e2m1
    return h


def moe_bm(sid):
    """Rows per workgroup of an id's MoE form: workgroup_tile(shape).moe_rows() of csrc/solution.h restated on the id's fields -- the staged and decode
    kernels hold 1 / 2 / 4 / 8 / 16 activation rows, the tiled kernel tile_m m-tiles of 16, the 32x32 MFMA kinds tile_m blocks of 32."""
    code, wm, mt = (sid >> 48) & 0xF, (sid >> 36) & 0xF, sid & 0xFF
    staged = {1: 1, 2: 2, 3: 4, 5: 1, 6: 2, 7: 4, 10: 8, 11: 16, 4: 1, 14: 2, 15: 8 if wm == 2 else 4}
    return staged[code] if code in staged else (32 if code in (12, 13) else 16) * mt


def is_tiled(sid):
    return (sid >> 48) & 0xF == 8


@functools.lru_cache(maxsize=None)
def listed_ids(kind, is_bf16, n, k, native=False):
    import petit_kernel as pkm
    h, ids = py_hints(kind, is_bf16), set()
    if native:
        pkm.ops.enable_native_fp4(True)
    try:
        for mm in ID_MS:
            ids.update(pkm.ops.get_fp4_solutions(h, mm, n, k))
    finally:
        if native:
            pkm.ops.enable_native_fp4(False)
    return tuple(sorted(i for i in ids if not native or (i >> 48) & 0xF in (9, 13)))


def resolves(kind, is_bf16, E, m, n, k, sid, act=0, native=False):
    from petit_kernel import _lib
    h = c_hints(kind, is_bf16)
    epi = C.byref(_lib.Epilogue(None, act, 0)) if act else None
    if native:
        na = _lib.NativeArgs(C.sizeof(_lib.NativeArgs), 0, 0, 0)
        return int(_lib.lib.petit_gemm_native_moe_resolve_solution(C.byref(h), E, m, n, k, C.c_uint64(sid & (2 ** 64 - 1)), epi, C.byref(na)))
    return int(_lib.lib.petit_gemm_moe_resolve_solution(C.byref(h), E, m, n, k, C.c_uint64(sid & (2 ** 64 - 1)), epi))


def cases(kind, is_bf16, group, act=0, native=False, names=None):
    """-> [(name, bm, E, offsets, m, n, k, regimes, ids)]: every routing of the group at its shapes; a routing that depends on the rows per
    workgroup once per distinct bm among the ids that have a MoE form for the shape (their ids with it), the others once with every id.  The
    default pick (-1; the native class: its three sentinels) runs on every case.  ids the resolver refuses for the case (under a gated epilogue: the
    kernels that cannot pair the halves) stay in the list: the launcher of the test counts them."""
    from petit_kernel import _lib
    auto = (_lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP8, _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP6, _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP4) if native else (-1,)
    out = []
    for name in names or GROUPS[group]:
        E = routings(1)[name][0]
        for n, k in shapes(kind, E, name, wide=bool(act) or native):
            ids = [i for i in listed_ids(kind, is_bf16, n, k, native) if resolves(kind, is_bf16, E, min(E, 64), n, k, i, 0, native)]
            by_bm = {}
            for i in ids:
                by_bm.setdefault(moe_bm(i) if name in BM_DEPENDENT else 0, []).append(i)
            for bm, some in sorted(by_bm.items()):
                E, offsets, m, regimes = routings(bm or 16)[name]
                out.append((name, bm, E, tuple(offsets), m, n, k, "G" if act else regimes, list(auto) + some))
    return out


@pytest.mark.parametrize("group,only_k", [("edges", 256), ("edges", 768), ("edges", 2048)] + [(g, None) for g in GROUPS if g != "edges"])
@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_generator_preconditions_and_teeth(kind, is_bf16, group, only_k):
    """Every problem of the plain, indexed and native legs (`edges`, the group with the most, one K at a time): the preconditions per expert, and the
    teeth."""
    t0, count = time.time(), 0
    seen = set()
    todo = [(c, None, False) for c in cases(kind, is_bf16, group)]
    if group in ("edges", "chunks", "malformed"):
        todo += [(c, gathered_rows(c[4]), False) for c in cases(kind, is_bf16, group, names=[x for x in GROUPS[group] if x in INDEXED_NAMES])]
    if group in NATIVE_GROUPS:
        for c in native_cases(is_bf16, group, kind):
            todo += [(c, None, True), (c, gathered_rows(c[4]), True)]
    for (name, bm, E, offsets, m, n, k, regimes, ids), a_rows, native in todo:
        for regime in regimes:
            key = (E, offsets, m, n, k, regime, a_rows, native)
            if key in seen or only_k not in (None, k):
                continue
            seen.add(key)
            P = problem(kind, is_bf16, E, offsets, m, n, k, regime, 0, a_rows)
            tag = f"{kind} bf16={is_bf16} {name} bm={bm} n={n} k={k} {regime} a_rows={a_rows}"
            check_preconditions(P, tag, native)
            check_teeth(P, tag)
            count += 1
    assert count
    print(f"moe_contract {kind} bf16={is_bf16} {group} {only_k or ''}: {count} problems, {time.time() - t0:.1f} s")


# --- 4. the GPU side: through the C ABI into caller-owned, poisoned, guarded buffers --------------------------------------------------------------

def operands(pk, P):
    """The launch operands of a problem on the device, built once: packed stacked weights and scales, gs [E], bias [E, n], activations, offsets."""
    if not hasattr(P, "dev"):
        dev16 = lambda b: torch.from_numpy(np.ascontiguousarray(b).view(np.int16).copy()).to(DEV)
        d = P.dev = Problem()
        qd = torch.from_numpy(P.q).to(DEV).view(torch.int32)
        if P.kind == "nv":
            d.b = pk.repack_nvfp4(qd, P.E * P.n, P.k)
            d.sp = pk.process_nvfp4_scales(torch.from_numpy(P.s).to(DEV).view(torch.float8_e4m3fn), P.E * P.n, P.k)
        else:
            d.b = pk.repack_mxfp4(qd, P.E * P.n, P.k)
            d.sp = pk.process_mxfp4_scales(torch.from_numpy(P.s).to(DEV), P.E * P.n, P.k)
        d.gs = torch.from_numpy(P.gs.astype(np.float32)).to(DEV)
        assert np.array_equal(P.gs.astype(np.float32).astype(np.float64), P.gs)
        d.bias = None if P.bias_bits is None else dev16(P.bias_bits)
        d.a = dev16(P.a_src_bits)
        d.offsets = torch.tensor(P.offsets, dtype=torch.int32, device=DEV)
        assert d.offsets.numel() == P.E + 1
        d.a_index = None if P.a_index is None else torch.from_numpy(P.a_index).to(DEV)
    return P.dev


def scatter_index(m, c_rows, seed):
    """c_row_index: a permutation of c_rows > m rows cut to m entries, some of them -1 and some >= c_rows."""
    rng = np.random.default_rng([seed, m, c_rows])
    idx = rng.permutation(c_rows)[:m].astype(np.int32)
    if m >= 3:
        idx[m // 3] = -1
        idx[m - 1] = c_rows
    if m >= 8:
        idx[m // 2 + 1] = c_rows + 7
    return idx


class MoeDevice:
    """One problem's operands on the device, its guarded C (rows x n_out between two guards) and the launch + check of one solution id, after
    test_exact_contract.Device.  form: "plain" petit_gemm_fp4_fp16_moe, "ex" petit_gemm_fp4_fp16_moe_ex, "native" petit_gemm_native_moe (MXFP4 experts:
    the packed tensors; NVFP4 experts: their resident images), "transient" petit_gemm_native_moe_transient (NVFP4 experts, packed tensors); the native
    forms' workspace is the declared bytes, then a guard.  c_index: the scatter (C then has c_rows rows, and the rows no index names stay poison); the gather is the
    problem's own (P.a_index).  gated: (want, alt, wrong) of gated_expect."""

    def __init__(self, pk, P, form="plain", activation=0, gated=None, c_index=None, c_rows=None):
        from petit_kernel import _lib
        self.pk, self.L, self.P, self.form, self.activation = pk, _lib, P, form, activation
        self.d = operands(pk, P)
        self.n_out = P.n // 2 if activation else P.n
        self.poison = POISON[P.is_bf16]
        want, alt = (P.want, P.want) if gated is None else gated[:2]
        self.wrong = None if gated is None else gated[2]
        self.rows, self.row_expert = P.m, P.owner
        self.c_index = None
        if c_index is not None:
            named = (c_index >= 0) & (c_index < c_rows)
            assert np.unique(c_index[named]).size == int(named.sum())                         # no row of C is named twice
            full = lambda v, fill, dtype: np.full((c_rows,) + v.shape[1:], fill, dtype=dtype)
            w2, a2, e2 = full(want, self.poison, np.uint16), full(alt, self.poison, np.uint16), full(P.owner, -1, np.int64)
            w2[c_index[named]], a2[c_index[named]], e2[c_index[named]] = want[named], alt[named], P.owner[named]
            want, alt, self.rows, self.row_expert = w2, a2, c_rows, e2
            self.c_index = torch.from_numpy(c_index).to(DEV)
        self.want_np = want.reshape(-1)
        dev16 = lambda b: torch.from_numpy(np.ascontiguousarray(b).view(np.int16).copy()).to(DEV).reshape(-1)
        self.want, self.alt = dev16(want), dev16(alt)
        self.hints = c_hints(P.kind, P.is_bf16)
        with_epilogue = self.d.bias is not None or activation
        self.epilogue = _lib.Epilogue(None if self.d.bias is None else self.d.bias.data_ptr(), activation, 0) if with_epilogue else None
        self.epi = C.byref(self.epilogue) if with_epilogue else None
        g, total = GUARD // 2, self.rows * self.n_out
        assert self.want.numel() == total
        self.c_all = torch.empty(g + total + g, dtype=torch.int16, device=DEV)               # [guard | rows * n_out outputs | guard]
        self.c_lo, self.c_out, self.c_hi = self.c_all[:g], self.c_all[g:g + total], self.c_all[g + total:]
        self.guard = torch.full((g,), self.poison, dtype=torch.int16, device=DEV)
        self.first = None
        self.na = _lib.NativeArgs(C.sizeof(_lib.NativeArgs), 0, 0, 0)
        self.ws_all = self.ws_ref = None

    def need(self, sid):
        if self.form not in ("native", "transient"):
            return 0
        P = self.P
        query = self.L.lib.petit_gemm_native_moe_workspace_bytes if self.form == "native" else self.L.lib.petit_gemm_native_moe_transient_workspace_bytes
        return int(query(C.byref(self.hints), P.E, P.m, P.n, P.k, C.c_uint64(sid & (2 ** 64 - 1)), self.epi,
                                                                    C.byref(self.na)))

    def reserve_scratch(self, most):
        total = (most + GUARD + 511) // 512 * 512
        self.ws_all = torch.empty(total, dtype=torch.uint8, device=DEV)
        self.ws_ref = torch.full((total,), 0xA5, dtype=torch.uint8, device=DEV)

    def launch(self, sid, need, plain_indices=False):
        P, d, p = self.P, self.d, lambda t: None if t is None else C.c_void_p(t.data_ptr())
        head = (p(self.c_out), p(d.a), p(d.b), p(d.sp), p(d.gs), p(d.offsets), P.E, P.m, P.n, P.k)
        a_rows = P.a_src.shape[0]
        index = (None, P.m, None, P.m) if plain_indices else (p(d.a_index), a_rows, p(self.c_index), self.rows)
        tail = (C.byref(self.hints), C.c_uint64(sid), self.epi)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if self.form == "plain":
            assert d.a_index is None and self.c_index is None
            return self.L.lib.petit_gemm_fp4_fp16_moe(*head, *tail, stream)
        if self.form == "ex":
            return self.L.lib.petit_gemm_fp4_fp16_moe_ex(*head, *index, *tail, stream)
        rest = (*index, *tail, C.byref(self.na), p(self.ws_all) if need else None, C.c_uint64(need), stream)
        if self.form == "transient":
            return self.L.lib.petit_gemm_native_moe_transient(*head, *rest)
        if P.kind == "nv":                                                                    # the resident images in place of b, no scales
            if not hasattr(d, "images"):
                d.images = self.pk.nvfp4_native_images(d.b, d.sp, P.E, P.n, P.k)
            head = head[:2] + (p(d.images), None) + head[4:]
        return self.L.lib.petit_gemm_native_moe(*head, *rest)

    def compare(self):
        if self.wrong is None:
            if torch.equal(self.c_out, self.want):
                return []
            got = self.c_out.cpu().numpy().view(np.uint16)
            return [self.describe(got, np.flatnonzero(got != self.want_np))]
        what = []
        if not bool(((self.c_out == self.want) | (self.c_out == self.alt)).all()):
            got = self.c_out.cpu().numpy().view(np.uint16)
            bad = np.flatnonzero(self.wrong(got))
            if bad.size:
                what.append(self.describe(got, bad))
        if self.first is None:
            self.first = self.c_out.clone()
        elif not torch.equal(self.c_out, self.first):
            differ = torch.nonzero(self.c_out != self.first).reshape(-1)
            what.append(f"{differ.numel()} outputs differ from the first launch of this problem, first at (row {int(differ[0]) // self.n_out}, "
                        f"col {int(differ[0]) % self.n_out})")
        return what

    def describe(self, got, bad):
        rows, cols = bad // self.n_out, bad % self.n_out
        unowned = self.row_expert[rows] < 0
        return (f"{bad.size} of {got.size} outputs differ, {int((got[bad] == self.poison).sum())} of them unwritten (still poison), {int(unowned.sum())} "
                f"of them in rows of no expert; first at (row {rows[0]}, col {cols[0]}), a row of expert {self.row_expert[rows[0]]}: got "
                f"{got[bad[0]]:#06x} want {self.want_np[bad[0]]:#06x}; rows {rows.min()}..{rows.max()}, cols {cols.min()}..{cols.max()}")

    def run(self, sid, plain_indices=False):
        """Poison, launch, compare on the device -> None, or the report of what is wrong."""
        sid &= 2 ** 64 - 1
        need = self.need(sid)
        self.c_all.fill_(self.poison)
        if self.ws_all is not None:
            self.ws_all.fill_(0xA5)
        rc = self.launch(sid, need, plain_indices)
        what = []
        if rc != 0:
            what.append(f"the resolver accepts the call, the launch returns {rc} ({self.L.error_string(rc)})")
        else:
            what += self.compare()
        if not torch.equal(self.c_lo, self.guard):
            what.append("the guard in front of C was written")
        if not torch.equal(self.c_hi, self.guard):
            what.append("the guard behind C was written")
        if self.ws_all is not None and not torch.equal(self.ws_all[need:], self.ws_ref[need:]):
            first = int(torch.nonzero(self.ws_all[need:] != self.ws_ref[need:])[0])
            what.append(f"workspace written {first} bytes past the {need} bytes the workspace query declares")
        if not what:
            return None
        P = self.P
        return (f"{self.form} E={P.E} m={P.m} n={P.n} k={P.k} regime {P.regime} activation {ACTIVATION_NAMES[self.activation]} id {sid:#x} [{self.L.describe_solution(sid)}] "
                f"offsets {P.offsets if P.E <= 8 else '...'}: " + "; ".join(what))


def run_case(D, ids, counts, native=False, plain_indices=False):
    """Every id of the case on the device D: launched when the resolver takes it with the case's epilogue, counted when it refuses."""
    P, failures = D.P, []
    runnable = []
    for sid in ids:
        if resolves(P.kind, P.is_bf16, P.E, P.m, P.n, P.k, sid, D.activation, native):
            runnable.append(sid)
        else:
            counts["refused"] += 1
    if native and runnable:
        D.reserve_scratch(max(D.need(sid) for sid in runnable))
    for sid in runnable:
        report = D.run(sid, plain_indices)
        counts["launched"] += 1
        if sid >= 0 and not native:
            key = (P.E, "tiled" if is_tiled(sid) else "streaming")
            counts["by_kind"][key] = counts["by_kind"].get(key, 0) + 1
        elif native:
            counts["by_kind"][(P.E, "native")] = counts["by_kind"].get((P.E, "native"), 0) + 1
        if report:
            failures.append(report)
    return failures


def new_counts():
    return {"launched": 0, "refused": 0, "by_kind": {}}


def finish(label, counts, failures, t0, kinds=("streaming", "tiled"), experts=()):
    shown = {f"E={e} {kind}": v for (e, kind), v in sorted(counts["by_kind"].items())}
    print(f"moe_contract {label}: launched {counts['launched']}, refused {counts['refused']}, {shown}, {time.time() - t0:.1f} s")
    for e in experts:
        for kind in kinds:
            assert counts["by_kind"].get((e, kind), 0) > 0, f"no {kind} id ran at E = {e}"
    assert not failures, f"{len(failures)} of {counts['launched']} launches wrong:\n" + "\n".join(failures[:20])


GROUP_EXPERTS = {"edges": (7,), "one-each": (65,), "chunks": (130, 256), "last-chunk": (1024,), "malformed": (5, 8, 130)}


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_plain_form_every_id_bit_for_bit(pk, kind, is_bf16, group):
    """petit_gemm_fp4_fp16_moe, every id with a MoE form and the default pick on every routing of the group: every owned output has the expected bits,
    every unowned output is still poison, both guards are untouched; epilogue 0 with the per-expert bias (regime B) and without a bias (A)."""
    t0, counts, failures = time.time(), new_counts(), []
    for name, bm, E, offsets, m, n, k, regimes, ids in cases(kind, is_bf16, group):
        for regime in regimes:
            D = MoeDevice(pk, problem(kind, is_bf16, E, offsets, m, n, k, regime))
            failures += [f"{name}: {f}" for f in run_case(D, ids, counts)]
    finish(f"plain {kind} bf16={is_bf16} {group}", counts, failures, t0, experts=GROUP_EXPERTS[group])


# --- the gated forms ---------------------------------------------------------------------------------------------------------------------------------

GATED_GROUPS = {"edges": ("edges",), "chunks": ("chunks130",), "last-chunk": ("last-chunk", "last-expert")}
GATED_SEEDS = 8


def gated_expect(P, act):
    """(want, alt u16 [m, n / 2], wrong(got bits) -> mask, undecided share) of a regime-G problem under the gated epilogue `act`: test_gated_contract's
    expectation and band on the owned rows, the poison on the rows of no expert."""
    own = P.owner >= 0
    Q = Problem()
    Q.y = P.y[own]
    expect(Q, P.is_bf16, act)
    nh = P.n // 2
    want, alt = (np.full((P.m, nh), POISON[P.is_bf16], dtype=np.uint16) for _ in range(2))
    want[own], alt[own] = Q.want, Q.alt
    assert not np.any(Q.want == POISON[P.is_bf16]) and not np.any(Q.alt == POISON[P.is_bf16])
    yg, yu = Q.y[:, :nh], Q.y[:, nh:]
    assert np.array_equal((yu + 1.0).astype(np.float32).astype(np.float64), yu + 1.0)          # u + 1 is exact in fp32 (y itself: rne_bits asserted it)

    def wrong(got):
        got = got.reshape(P.m, nh)
        bad = got != POISON[P.is_bf16]
        bad[own] = Q.wrong(got[own].reshape(-1)).reshape(-1, nh)
        return bad.reshape(-1)
    return want, alt, wrong, Q.undecided


@functools.lru_cache(maxsize=4)
def gated_problem(kind, is_bf16, E, offsets, m, n, k):
    """The regime-G problem of a gated case at the first seed that keeps BOTH activations within the cap on the float64 formula alone."""
    for seed in range(GATED_SEEDS):
        P = moe_exact_problem(kind, is_bf16, E, list(offsets), m, n, k, "G", seed)
        G = {act: gated_expect(P, act) for act in (1, 2)}
        if max(g[3] for g in G.values()) <= CAP[is_bf16]:
            P.seed = seed
            return P, G
    raise AssertionError(f"no seed below {GATED_SEEDS} keeps {kind} bf16={is_bf16} E={E} m={m} n={n} k={k} within the cap")


@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_every_gated_problem_is_within_the_cap(kind, is_bf16):
    """The regime-G problems the gated GPU test launches: the preconditions, the teeth, and both activations within test_gated_contract's cap on the
    float64 formula alone, at a seed below GATED_SEEDS."""
    worst, reseeded, count = 0.0, 0, 0
    for group in GATED_GROUPS:
        for name, bm, E, offsets, m, n, k, _, ids in cases(kind, is_bf16, group, act=1, names=GATED_GROUPS[group]):
            P, G = gated_problem(kind, is_bf16, E, offsets, m, n, k)
            tag = f"{kind} bf16={is_bf16} {name} bm={bm} n={n} k={k} seed={P.seed}"
            check_preconditions(P, tag)
            check_teeth(P, tag)                                                               # (on the plain epilogue of the same y)
            for act in (1, 2):
                assert G[act][3] <= CAP[is_bf16], (tag, act)
            worst, reseeded, count = max(worst, max(G[1][3], G[2][3])), reseeded + (P.seed != 0), count + 1
    print(f"moe_contract gated {kind} bf16={is_bf16}: {count} problems, largest undecided share {worst:.4f} (cap {CAP[is_bf16]}), {reseeded} not at seed 0")


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GATED_GROUPS))
@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_gated_forms_every_id(pk, kind, is_bf16, group):
    """SiLU-mul and SwiGLU-OAI with the per-expert bias through petit_gemm_fp4_fp16_moe: test_gated_contract's band per output, every launch of a
    problem the bits of its first, unowned rows poison, guards untouched.  An id the resolver refuses under the activation is counted."""
    t0, counts, failures, worst = time.time(), new_counts(), [], 0.0
    for act in (1, 2):
        for name, bm, E, offsets, m, n, k, _, ids in cases(kind, is_bf16, group, act=act, names=GATED_GROUPS[group]):
            P, G = gated_problem(kind, is_bf16, E, offsets, m, n, k)
            worst = max(worst, G[act][3])
            D = MoeDevice(pk, P, activation=act, gated=G[act])
            failures += [f"{name}: {f}" for f in run_case(D, ids, counts)]
    assert worst <= CAP[is_bf16]
    finish(f"gated {kind} bf16={is_bf16} {group} (largest undecided share {worst:.4f}, cap {CAP[is_bf16]})", counts, failures, t0)
    assert counts["launched"] > 0


# --- the indexed form ------------------------------------------------------------------------------------------------------------------------------

INDEXED_NAMES = ("edges", "chunks130", "short")


@pytest.mark.gpu
@pytest.mark.parametrize("name", INDEXED_NAMES)
@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_indexed_form_every_id_bit_for_bit(pk, kind, is_bf16, name):
    """petit_gemm_fp4_fp16_moe_ex: a_row_index a gather with repeated tokens from a_rows < m rows, a few indices out of range (zeros); c_row_index a
    permutation of c_rows > m rows with entries -1 and >= c_rows; rows of C that no index names stay poison.  Both indices null: the plain form's bits."""
    t0, counts, failures = time.time(), new_counts(), []
    group = next(g for g, names in GROUPS.items() if name in names)
    for _, bm, E, offsets, m, n, k, regimes, ids in cases(kind, is_bf16, group, names=[name]):
        for regime in regimes:
            P = problem(kind, is_bf16, E, offsets, m, n, k, regime, 0, gathered_rows(m))
            c_rows = m + 9
            D = MoeDevice(pk, P, form="ex", c_index=scatter_index(m, c_rows, 1), c_rows=c_rows)
            failures += [f"{name} gather + scatter: {f}" for f in run_case(D, ids, counts)]
            D = MoeDevice(pk, P, form="ex")
            failures += [f"{name} gather: {f}" for f in run_case(D, ids, counts)]
            D = MoeDevice(pk, problem(kind, is_bf16, E, offsets, m, n, k, regime), form="ex")
            failures += [f"{name} null indices: {f}" for f in run_case(D, ids, counts, plain_indices=True)]
    finish(f"indexed {kind} bf16={is_bf16} {name}", counts, failures, t0, experts=(routings(1)[name][0],))


# --- the native class ------------------------------------------------------------------------------------------------------------------------------

NATIVE_GROUPS = {"edges": ("edges",), "chunks": ("chunks130",), "last-chunk": ("last-chunk", "last-expert"),
                 "malformed": tuple(f"malformed5-{i}" for i in (0, 1, 3, 4, 5, 6))}


def native_cases(is_bf16, group, kind="mx"):
    """MXFP4 experts: regimes A and B.  NVFP4 experts (the image forms): regime A alone -- the image is not the exact dequant of regime B's weights
    (test_nvfp4_native_image_is_exact_on_regime_a_alone_per_expert)."""
    out = []
    for name, bm, E, offsets, m, n, k, _, ids in cases(kind, is_bf16, group, native=True, names=NATIVE_GROUPS[group]):
        assert bm in (0, NATIVE_BM), "the native MoE forms are the 128-row tile"
        out.append((name, bm, E, offsets, m, n, k, "AB" if kind == "mx" else "A", ids))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(NATIVE_GROUPS))
@pytest.mark.parametrize("is_bf16", [True, False])
def test_native_moe_mxfp4_every_id_bit_for_bit(pk, is_bf16, group):
    """petit_gemm_native_moe on MXFP4 experts, MXFP8 / MXFP6 / MXFP4 activations (every id the native resolver accepts and the three sentinels), 16-bit
    rows quantised by the call: the exact class's bits (test_exact_contract's argument; its preconditions are asserted on these problems by
    test_generator_preconditions_and_teeth), with and without a_row_index / c_row_index; the workspace is exactly the declared bytes and nothing is
    written past them."""
    t0, counts, failures = time.time(), new_counts(), []
    for name, bm, E, offsets, m, n, k, regimes, ids in native_cases(is_bf16, group):
        assert len(ids) > 3, "no explicit native id has a MoE form for the shape"
        for regime in regimes:
            D = MoeDevice(pk, problem("mx", is_bf16, E, offsets, m, n, k, regime), form="native")
            failures += [f"{name}: {f}" for f in run_case(D, ids, counts, native=True, plain_indices=True)]
            c_rows = m + 9
            D = MoeDevice(pk, problem("mx", is_bf16, E, offsets, m, n, k, regime, 0, gathered_rows(m)), form="native",
                          c_index=scatter_index(m, c_rows, 2), c_rows=c_rows)
            failures += [f"{name} gather + scatter: {f}" for f in run_case(D, ids, counts, native=True)]
    finish(f"native mx bf16={is_bf16} {group}", counts, failures, t0, kinds=("native",), experts=NATIVE_EXPERTS[group])


NATIVE_EXPERTS = {"edges": (7,), "chunks": (130,), "last-chunk": (1024,), "malformed": (5,)}


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(NATIVE_GROUPS))
@pytest.mark.parametrize("is_bf16", [True, False])
def test_native_moe_nvfp4_image_forms_bit_for_bit(pk, is_bf16, group):
    """NVFP4 experts on the native class, from resident images (petit_gemm_native_moe) and without them (petit_gemm_native_moe_transient, whose workspace
    holds the images of the experts with rows, then the quantised rows): regime A, on which the image is the exact dequant, so the exact class's bits;
    with and without the indices; nothing written past the declared workspace."""
    t0, counts, failures = time.time(), new_counts(), []
    for name, bm, E, offsets, m, n, k, regimes, ids in native_cases(is_bf16, group, "nv"):
        assert len(ids) > 3 and regimes == "A"
        P, c_rows = problem("nv", is_bf16, E, offsets, m, n, k, "A"), m + 9
        Pg = problem("nv", is_bf16, E, offsets, m, n, k, "A", 0, gathered_rows(m))
        for form in ("native", "transient"):
            failures += [f"{name} {form}: {f}" for f in run_case(MoeDevice(pk, P, form=form), ids, counts, native=True, plain_indices=True)]
            D = MoeDevice(pk, Pg, form=form, c_index=scatter_index(m, c_rows, 2), c_rows=c_rows)
            failures += [f"{name} {form} gather + scatter: {f}" for f in run_case(D, ids, counts, native=True)]
    finish(f"native nv images bf16={is_bf16} {group}", counts, failures, t0, kinds=("native",), experts=NATIVE_EXPERTS[group])


def test_nvfp4_native_image_is_exact_on_regime_a_alone_per_expert():
    """test_exact_contract.test_nvfp4_native_image_is_not_exact_on_regime_b per expert of a stacked problem: every expert's image dequantises to the
    model's weights on regime A and to something else on regime B, so the image forms run regime A alone."""
    from petit_kernel import offline
    E, n, k = 5, 288, 768
    offsets, m = _from_counts([1] * E)
    for regime in "AB":
        P = moe_exact_problem("nv", True, E, offsets, m, n, k, regime, 0)
        for e in range(E):
            q, s = (np.ascontiguousarray(x[e * n:(e + 1) * n]) for x in (P.q, P.s))
            b = offline.repack_nvfp4_cpu(torch.from_numpy(q).view(torch.int32), n, k)
            sp = offline.process_nvfp4_scales_cpu(torch.from_numpy(s).view(torch.float8_e4m3fn), n, k)
            dq = offline.nvfp4_native_image_dequant_cpu(offline.nvfp4_native_image_cpu(b, sp, n, k), n, k).numpy()
            assert bool(np.array_equal(dq, P.w[e * n:(e + 1) * n])) == (regime == "A"), (regime, e)


# --- the Python route --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_python_route_writes_every_output(pk, kind, is_bf16):
    """mul_*_a16_moe and mul_*_a16_moe_indexed (torch.empty for C): the allocator's cache is emptied and a block of C's size filled with poison and freed
    before every call (test_exact_contract.test_python_route_writes_every_output); the default pick, one streaming and one tiled id on a well-formed
    routing write the expected bits into every output (indexed: into every row an index names)."""
    dtype = torch.bfloat16 if is_bf16 else torch.float16
    name, bm, E, offsets, m, n, k, _, ids = next(c for c in cases(kind, is_bf16, "edges") if c[1] == 16 and c[6] == 768)
    some = [-1, next(i for i in ids if i >= 0 and not is_tiled(i))]
    some.append(next(i for c in cases(kind, is_bf16, "edges") if c[6] == 768 for i in c[8] if i >= 0 and is_tiled(i)))
    mul, mul_idx = ((pk.mul_nvfp4_a16_moe, pk.mul_nvfp4_a16_moe_indexed) if kind == "nv" else (pk.mul_mxfp4_a16_moe, pk.mul_mxfp4_a16_moe_indexed))
    P = problem(kind, is_bf16, E, offsets, m, n, k, "B")
    assert (P.owner >= 0).all()
    d = operands(pk, P)
    want = torch.from_numpy(P.want.view(np.int16).copy()).to(DEV)
    c_rows = m + 9
    c_index = scatter_index(m, c_rows, 3)
    named = (c_index >= 0) & (c_index < c_rows)
    c_dev = torch.from_numpy(c_index).to(DEV)
    rows_dev = torch.from_numpy(c_index[named].astype(np.int64)).to(DEV)
    for sid in some:
        for indexed in (False, True):
            rows = c_rows if indexed else m
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            poison = torch.full((rows, n), POISON[is_bf16], dtype=torch.int16, device=DEV)
            del poison
            a, bias = d.a.view(dtype).reshape(m, k), d.bias.view(dtype).reshape(E, n)
            if indexed:
                c = mul_idx(a, d.b, d.sp, d.gs, d.offsets, m, n, k, E, c_row_index=c_dev, c_rows=c_rows, solution_id=sid, bias=bias)
                got, expected = c.view(torch.int16)[rows_dev], want[torch.from_numpy(np.flatnonzero(named)).to(DEV)]
            else:
                c = mul(a, d.b, d.sp, d.gs, d.offsets, m, n, k, E, sid, bias=bias)
                got, expected = c.view(torch.int16), want
            assert c.shape == (rows, n) and c.dtype == dtype
            assert torch.equal(got, expected), f"{'indexed ' if indexed else ''}{sid:#x} [{describe(sid)}]"


def describe(sid):
    from petit_kernel import _lib
    return _lib.describe_solution(sid & (2 ** 64 - 1))

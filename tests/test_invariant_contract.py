"""The batch-invariant GEMMs (include/petit_amd.h "Batch-invariant GEMM", "Batch-invariant MoE launch") pinned to their definition, bit for bit:
the entries have no solution id, so none of test_exact_contract / test_gated_contract / test_value_contract / test_moe_contract launches them.
This module carries those modules' generators and judging to the four entry points petit_gemm_{fp4,mxfp4}_fp16_invariant and
petit_gemm_{fp4,mxfp4}_fp16_moe_invariant, and to the CPU twin petit_gemm_fp4_invariant_host.

Leg V, the value domain.  test_value_contract's truth tables (every e4m3 / e8m0 scale byte x 16 codes, the ends of bf16 / fp16, fp16 subnormal
activations, negative / full-mantissa / tiny gs), its shifted e8m0 regime and its non-finite activations, through both launch forms of the dense
entry, through the MoE entry (E = 3 experts with rows and a rowless one, gathered A, scattered C) and, without a GPU, through the CPU twin.
  The plain call of these entries rounds TWICE (y = f32(f32(fold * gs) + bias), the header's statement), where the table's expectation
  (table_expect) is the exact-class contract's ONE rounding fma(acc, gs, bias).  invariant_table_expect takes table_expect as it is -- its
  generator conditions, its NaN columns, its zeros -- and restates the 16 bits with the two roundings; the two differ only where a set has a
  bias AND a gs that is no power of two (test_table_expectation_two_roundings counts them), and there the header is the contract.
Leg X, the stated order.  fold_problem: weights periodic in the slice length L, activations whose slices play the roles BIG+ / BIG- / SMALL, so
that every in-slice sum is exact in any order and the fold ACROSS slices is inexact and order-dependent in the 16 output bits.  The expectation
is numpy float32, one operation at a time.  The slabs of the split forms are read back from the caller's workspace and compared with p_s.
A second generator (rounding_problem) separates the plain call's multiply-then-add from the gated calls' fma.

Every GPU launch goes through the C ABI into the guarded, poisoned C of test_exact_contract.Device / test_moe_contract.MoeDevice and a guarded,
poisoned workspace: the return code, the outputs, both C guards, every workspace byte past the queried size and -- in the whole forms -- every
workspace byte at all are checked after every launch.  M sets: the dense switch is read from petit_gemm_invariant_slabs, the MoE form from
petit_gemm_moe_invariant_form.  profiles/invariant_contract.md records launch counts, mutant shares and times.
"""
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_exact_contract import DEV, FP4, POISON, Device, Problem, exact_problem, pk, to_bits  # noqa: F401
from test_gated_contract import GatedDevice, expect
from test_gemm_invariant import _switch
from test_moe_contract import MoeDevice, row_ownership
from test_value_contract import (INF_BITS, KS, MS as VALUE_MS, SHIFTS, TABLE_N, ValueDevice, activation_classes, injections, nonfinite_bases,
                                 nonfinite_problem, pairs_read, required_pairs, shifted_and_switched, table_expect, table_series, two_sum_odd,
                                 values16)

FAMILIES = [("nv", True), ("nv", False), ("mx", True)]           # bf16 x NVFP4, fp16 x NVFP4, bf16 x MXFP4 (fp16 x MXFP4 is refused: asserted once)
DTYPES = {True: torch.bfloat16, False: torch.float16}


def _lib():
    from petit_kernel import _lib as lib
    return lib


def type_codes(kind, is_bf16):
    L = _lib()
    return (L.CXX_DTYPE_BF16 if is_bf16 else L.CXX_DTYPE_FP16), (L.CXX_DTYPE_FP4_E2M1 if kind == "nv" else L.CXX_DTYPE_MXFP4_E2M1)


def geometry(kind, is_bf16, n, k):
    """(S, L) of petit_gemm_invariant_geometry."""
    S, Lk = C.c_uint(0), C.c_uint(0)
    _lib().lib.petit_gemm_invariant_geometry(n, k, *type_codes(kind, is_bf16), C.byref(S), C.byref(Lk))
    return S.value, Lk.value


@functools.lru_cache(maxsize=None)
def dense_ms(kind, is_bf16, n, k):
    """{1, 5, 16, 17, last split M, first whole M, 65, 129}, the switch read from petit_gemm_invariant_slabs at a K of several slices."""
    split_m, whole_m = _switch(n, k if geometry(kind, is_bf16, n, k)[0] > 1 else 4 * k, DTYPES[is_bf16], kind)
    assert _lib().lib.petit_gemm_invariant_workspace_bytes(split_m, n, k, *type_codes(kind, is_bf16)) > 0
    assert _lib().lib.petit_gemm_invariant_workspace_bytes(whole_m, n, k, *type_codes(kind, is_bf16)) == 0
    return tuple(sorted({1, 5, 16, 17, split_m, whole_m, 65, 129}))


def moe_form(m, E):
    return int(_lib().lib.petit_gemm_moe_invariant_form(m, E))


@functools.lru_cache(maxsize=None)
def moe_counts(E=3):
    """Per-expert row counts of both forms, named by petit_gemm_moe_invariant_form: {"split": (3, 2, 3), "whole": (17, 5, 40)} today."""
    out = {}
    for counts in ((3, 2, 3), (17, 5, 40)):
        out.setdefault("split" if moe_form(sum(counts), E + 1) == 1 else "whole", counts)
    assert set(out) == {"split", "whole"}, out
    return out


# --- the CPU twin ------------------------------------------------------------------------------------------------------------------------------

def packed_cpu(kind, q, s, n, k):
    from petit_kernel import offline
    b = offline.repack_nvfp4_cpu(torch.from_numpy(np.ascontiguousarray(q)).view(torch.int32), n, k).contiguous()
    if kind == "nv":
        sp = offline.process_nvfp4_scales_cpu(torch.from_numpy(np.ascontiguousarray(s)).view(torch.float8_e4m3fn), n, k).contiguous()
    else:
        sp = offline.process_mxfp4_scales_cpu(torch.from_numpy(np.ascontiguousarray(s)), n, k).contiguous()
    return b, sp


def twin(kind, is_bf16, packed, a_bits, gs, bias_bits, n, k):
    """petit_gemm_fp4_invariant_host -> bits u16 [m, n]."""
    b, sp = packed
    a_bits = np.ascontiguousarray(a_bits)
    m = a_bits.shape[0]
    out = np.full((m, n), POISON[is_bf16], dtype=np.uint16)
    gsf = None if gs is None else C.byref(C.c_float(gs))
    bias_bits = None if bias_bits is None else np.ascontiguousarray(bias_bits)
    rc = _lib().lib.petit_gemm_fp4_invariant_host(out.ctypes.data, a_bits.ctypes.data, b.data_ptr(), sp.data_ptr(), gsf,
                                                  None if bias_bits is None else bias_bits.ctypes.data, m, n, k, *type_codes(kind, is_bf16))
    assert rc == 0, rc
    return out


def judge(got, want, is_bf16, must_nan=None, is_zero=None):
    """ValueDevice.wrong in numpy: an output that must be NaN is any NaN but the poison, an expected zero is a zero of either sign, the rest
    by bits.  -> the mask of wrong outputs."""
    got, mag = got.astype(np.uint16), got.astype(np.uint16) & 0x7FFF
    ok = got == want
    if must_nan is not None:
        ok = np.where(must_nan, (mag > INF_BITS[is_bf16]) & (got != POISON[is_bf16]), ok)
    if is_zero is not None:
        ok = ok | (is_zero & (mag == 0))
    return ~ok


def f32_to_16(y32, is_bf16):
    with np.errstate(over="ignore", invalid="ignore"):
        return O.f32_to_bf16_bits(y32) if is_bf16 else y32.astype(np.float16).view(np.uint16)


# --- leg V: the tables under the plain call's two roundings ---------------------------------------------------------------------------------------

def invariant_table_expect(P, is_bf16):
    """-> (bits, must_nan, is_zero, differs): table_expect as it is (its conditions asserted, its NaN columns and zeros), the bits restated as
    the PLAIN invariant call forms them: y = f32(f32(a w gs) + bias), two roundings, then the one rounding to 16 bits.  a w gs is exact in
    float64 (17 + 24 bits), so its float32 conversion is the multiply's rounding, and the add is numpy's float32 add.  differs: where these
    bits are not table_expect's."""
    bits1, must_nan, is_zero = table_expect(P, is_bf16)
    T, m = P.T, P.a_bits.shape[0]
    a = values16(P.a_bits[np.arange(m), P.kappa], is_bf16)
    with np.errstate(invalid="ignore", over="ignore"):
        y1 = (a[:, None] * T.w[:, P.kappa].T * P.gs).astype(np.float32)
        if P.bias_bits is not None:
            y2 = y1 + values16(P.bias_bits, is_bf16).astype(np.float32)[None, :]
        else:
            y2 = y1
        fin = ~must_nan
        assert not ((y2[fin] != 0) & (np.abs(y2[fin]) < 2.0 ** -126)).any(), "an fp32 subnormal sum: no part of the contract"
        bits = f32_to_16(np.where(must_nan, np.float32(0), y2), is_bf16)
    bits = np.where(must_nan, bits1, bits).astype(np.uint16)
    zero2 = (y2 == 0) & ~must_nan
    return bits, must_nan, zero2, (bits != bits1) & ~(zero2 & is_zero)


def table_problem(P, is_bf16):
    """A copy of a table_series problem whose want / must_nan / is_zero are the plain invariant call's."""
    Q = type(P)()
    Q.__dict__.update(P.__dict__)
    Q.want, Q.must_nan, Q.is_zero, Q.differs = invariant_table_expect(P, is_bf16)
    return Q


# --- the device side: the dense entries ------------------------------------------------------------------------------------------------------------

class InvariantDevice(Device):
    """test_exact_contract.Device (operands, poison, guarded C) launched through petit_gemm_{fp4,mxfp4}_fp16_invariant into a guarded, poisoned
    workspace of the test's own.  need() is petit_gemm_invariant_workspace_bytes.  run() checks the return code, compare() (the base's, or a
    mixed-in judge's), both C guards, every workspace byte past the queried size, and in the whole form (a query of 0) every byte."""

    def __init__(self, pk, kind, is_bf16, m, n, k, P, activation=0):
        super().__init__(pk, kind, is_bf16, m, n, k, P, activation)
        self.fn = self.L.lib.petit_gemm_fp4_fp16_invariant if kind == "nv" else self.L.lib.petit_gemm_mxfp4_fp16_invariant
        self.types = type_codes(kind, is_bf16)
        self.S, self.slice_k = geometry(kind, is_bf16, n, k)
        self.slabs = int(self.L.lib.petit_gemm_invariant_slabs(m, n, k, *self.types))
        self.whole = self.need() == 0
        assert self.slabs == (1 if self.whole else self.S) and (self.whole or self.need() == (self.S * m * n * 4 + 255) // 256 * 256)
        self.reserve_scratch(self.need())
        assert self.ws_all.data_ptr() % 256 == 0

    def need(self, sid=None) -> int:
        return int(self.L.lib.petit_gemm_invariant_workspace_bytes(self.m, self.n, self.k, *self.types))

    def run(self, use_gs=True, use_bias=True):
        """Poison, launch, compare on the device -> None, or the report of what is wrong."""
        need = self.need()
        self.c_all.fill_(self.poison)
        self.ws_all.fill_(self.poison)
        epi = self.epi
        if self.bias is not None and not use_bias:
            self.no_bias = self.L.Epilogue(None, self.activation, 0)
            epi = C.byref(self.no_bias)
        rc = self.fn(C.c_void_p(self.c_out.data_ptr()), C.c_void_p(self.a.data_ptr()), C.c_void_p(self.b.data_ptr()), C.c_void_p(self.sp.data_ptr()),
                     C.c_void_p(self.gs.data_ptr()) if use_gs else None, self.m, self.n, self.k, C.byref(self.hints), epi,
                     C.c_void_p(self.ws_all.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        what = []
        if rc != 0:
            what.append(f"the launch returns {rc} ({self.L.error_string(rc)})")
        else:
            what += self.compare()
        if not torch.equal(self.c_lo, self.guard):
            what.append("the guard in front of C was written")
        if not torch.equal(self.c_hi, self.guard):
            what.append("the guard behind C was written")
        ws8 = self.ws_all.view(torch.uint8)
        if not torch.equal(ws8[need:], self.ws_ref[need:]):
            first = int(torch.nonzero(ws8[need:] != self.ws_ref[need:])[0])
            what.append(f"workspace written {first} bytes past the {need} bytes petit_gemm_invariant_workspace_bytes declares" if need else
                        f"the whole form wrote its workspace (byte {first})")
        if not what:
            return None
        return f"{self.kind} bf16={self.is_bf16} m={self.m} n={self.n} k={self.k} {'whole' if self.whole else 'split'} form: " + "; ".join(what)

    def slab_values(self):
        """The S slabs [S, m, n] float32 the split form's first launch left in the caller's workspace."""
        assert not self.whole
        return self.ws_all.view(torch.float32)[:self.S * self.m * self.n].reshape(self.S, self.m, self.n).cpu().numpy()


class InvariantValueDevice(InvariantDevice, ValueDevice):
    """... judged as test_value_contract.ValueDevice judges (its compare, unchanged)."""


class InvariantGatedDevice(InvariantDevice, GatedDevice):
    """... judged as test_gated_contract.GatedDevice judges (its compare, unchanged: the band, and every launch the bits of the first)."""


def counts_for(counts, D):
    counts["whole" if D.whole else "split"] += 1


def new_counts():
    return {"split": 0, "whole": 0}


def finish(tag, counts, failures, t0, both=True):
    print(f"invariant_contract {tag}: launches {counts}, {time.time() - t0:.1f} s")
    assert not both or (counts["split"] and counts["whole"]), ("a form did not run", counts)
    assert not failures, f"{len(failures)} of {counts['split'] + counts['whole']} launches wrong:\n" + "\n".join(failures[:20])


# --- the device side: the MoE entries -----------------------------------------------------------------------------------------------------------------

class MoeInvariantDevice(MoeDevice):
    """test_moe_contract.MoeDevice (operand stacking, row ownership, guarded C with the scatter, rows of no expert stay poison) launched
    through petit_gemm_{fp4,mxfp4}_fp16_moe_invariant into a guarded workspace.  The form is petit_gemm_moe_invariant_form's.  P.must_nan /
    P.is_zero (optional, [m, n]) are judged as ValueDevice judges them."""

    def __init__(self, pk, P, activation=0, gated=None, c_index=None, c_rows=None):
        super().__init__(pk, P, "ex", activation, gated, c_index, c_rows)
        self.types = type_codes(P.kind, P.is_bf16)
        self.split = moe_form(P.m, P.E) == 1
        self.S, self.slice_k = geometry(P.kind, P.is_bf16, P.n, P.k)
        assert (self.need(0) > 0) == self.split and (not self.split or self.need(0) == (self.S * P.m * P.n * 4 + 255) // 256 * 256)
        self.reserve_scratch(self.need(0))
        assert self.ws_all.data_ptr() % 256 == 0
        self.masks = None
        if hasattr(P, "must_nan"):
            masks = []
            for mask in (P.must_nan, P.is_zero):
                if c_index is not None:
                    named = (c_index >= 0) & (c_index < c_rows)
                    full = np.zeros((c_rows, self.n_out), dtype=bool)
                    full[c_index[named]] = mask[named]
                    mask = full
                masks.append(torch.from_numpy(np.ascontiguousarray(mask)).to(DEV).reshape(-1))
            self.masks = masks

    def need(self, sid):
        P = self.P
        return int(self.L.lib.petit_gemm_moe_invariant_workspace_bytes(P.E, P.m, P.n, P.k, *self.types))

    def launch(self, sid, need, plain_indices=False):
        P, d, p = self.P, self.d, lambda t: None if t is None else C.c_void_p(t.data_ptr())
        fn = self.L.lib.petit_gemm_fp4_fp16_moe_invariant if P.kind == "nv" else self.L.lib.petit_gemm_mxfp4_fp16_moe_invariant
        return fn(p(self.c_out), p(d.a), p(d.b), p(d.sp), p(d.gs), p(d.offsets), P.E, P.m, P.n, P.k, p(d.a_index), P.a_src.shape[0],
                  p(self.c_index), self.rows, C.byref(self.hints), self.epi, p(self.ws_all), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def compare(self):
        if self.masks is None or self.wrong is not None:
            return super().compare()
        must_nan, is_zero = self.masks
        got = self.c_out.to(torch.int32) & 0xFFFF
        mag = got & 0x7FFF
        ok = torch.where(must_nan, (mag > INF_BITS[self.P.is_bf16]) & (got != self.poison), self.c_out == self.want)
        bad = ~(ok | (is_zero & (mag == 0)))
        if not bool(bad.any()):
            return []
        return [self.describe(self.c_out.cpu().numpy().view(np.uint16), np.flatnonzero(bad.cpu().numpy()))]

    def run(self, sid=0, plain_indices=False):
        report = super().run(sid, plain_indices)
        return report and f"{'split' if self.split else 'whole'} form: {report}"

    def slab_values(self):
        assert self.split
        P = self.P
        return self.ws_all.view(torch.float32)[:self.S * P.m * P.n].reshape(self.S, P.m, P.n).cpu().numpy()


def moe_stack(kind, is_bf16, n, k, experts, rowless_w, a_src_bits, a_index, c_rows_extra=3, seed=0):
    """-> (Problem for MoeInvariantDevice, c_index, c_rows).  experts: [(q, s, gs, bias_bits or None, want [rows, n], must_nan, is_zero)] in
    grouped-row order, every one with rows; a rowless expert (rowless_w = (q, s)) is appended, so E = len(experts) + 1 and the last two offsets
    are equal.  a_src_bits [a_rows, k] and a_index [m] are the caller's gather.  The scatter is a permutation of m + c_rows_extra rows with one
    entry out of range (that row is skipped)."""
    P = Problem()
    E = len(experts) + 1
    counts = [e[4].shape[0] for e in experts]
    m = sum(counts)
    P.kind, P.is_bf16, P.E, P.m, P.n, P.k, P.regime = kind, is_bf16, E, m, n, k, "-"
    P.offsets = [0] + [int(v) for v in np.cumsum(counts)] + [m]
    P.q = np.concatenate([e[0] for e in experts] + [rowless_w[0]])
    P.s = np.concatenate([e[1] for e in experts] + [rowless_w[1]])
    P.gs = np.array([e[2] for e in experts] + [1.0])
    zero = np.zeros(n, dtype=np.uint16)
    P.bias_bits = np.stack([zero if e[3] is None else e[3] for e in experts] + [zero])       # (a +0 bias where a set has none: y + 0 = y)
    P.a_src, P.a_src_bits, P.a_index = a_src_bits, a_src_bits, a_index.astype(np.int32)
    P.owner, P.spans = row_ownership(P.offsets, m)
    assert (P.owner >= 0).all() and P.spans[-1][0] == P.spans[-1][1] and len(set(P.owner.tolist())) == E - 1
    P.want = np.concatenate([e[4] for e in experts])
    P.must_nan = np.concatenate([e[5] for e in experts])
    P.is_zero = np.concatenate([e[6] for e in experts])
    rng = np.random.default_rng([seed, m, n, k])
    c_rows = m + c_rows_extra
    c_index = rng.permutation(c_rows)[:m].astype(np.int32)
    c_index[m // 2] = c_rows + 2                                                                # out of range: skipped
    return P, c_index, c_rows


def gather(rows_bits, seed, zero_row):
    """rows_bits [m, k] in grouped order -> (a_src_bits [m, k], a_index [m]): a permutation, a_src[a_index[r]] = rows_bits[r], but a_index of
    `zero_row` (whose rows_bits must be zeros) is out of range."""
    m = rows_bits.shape[0]
    perm = np.random.default_rng([seed, m, 0x6A]).permutation(m)
    src = np.empty_like(rows_bits)
    src[perm] = rows_bits
    assert not rows_bits[zero_row].any()
    src[perm[zero_row]] = 0x3C00                                                                # (a row of ones in its place: nothing reads it)
    perm = perm.astype(np.int32)
    perm[zero_row] = m + 4
    return src, perm


# --- leg X: the generator of the stated order -----------------------------------------------------------------------------------------------------------

FOLD_EXP = {True: (24, 0), False: (14, -10)}      # (E, e): BIG activations 2^E b, SMALL ones 2^e d; bf16 / fp16
FOLD_KS = (768, 1024, 4352)                       # S = 3, S = 4, and (at one n-tile) S = 9 with L = 512 and a last slice half as long
FOLD_NS = {"nv": (16, 208), "mx": (32, 224)}
FOLD_ROWS = 129
FOLD_GS = float(np.float32(4.0 / 3.0))
FOLD_SEEDS = 16
MUTANTS = ("descending", "pairwise", "moved boundary", "one chain")
SHARE = 0.05


def fold_shapes(kind):
    return [(n, k) for n in FOLD_NS[kind] for k in FOLD_KS if k != 4352 or n == FOLD_NS[kind][0]]


def fold_draw(kind, is_bf16, n, k, seed):
    """One draw of the generator for FOLD_ROWS rows (a problem of m rows is its first m: the definition is row-wise)."""
    S, L = geometry(kind, is_bf16, n, k)
    rng = np.random.default_rng([seed, kind == "mx", is_bf16, n, k, 0xF01D])
    group, M = 16 if kind == "nv" else 32, FOLD_ROWS
    P = Problem()
    P.kind, P.is_bf16, P.n, P.k, P.S, P.L, P.seed = kind, is_bf16, n, k, S, L, seed
    reps = -(-k // L)
    code0 = rng.integers(0, 16, (n, L), dtype=np.uint8)
    sidx0 = rng.integers(0, 3, (n, L // group))
    code, sidx = np.tile(code0, (1, reps))[:, :k], np.tile(sidx0, (1, reps))[:, :k // group]       # W[n][k] = W0[n][k mod L]
    P.q = (code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8)
    P.s = np.array([0x38, 0x40, 0x48] if kind == "nv" else [127, 128, 129], dtype=np.uint8)[sidx]
    P.w = FP4[code] * np.repeat(np.array([1.0, 2.0, 4.0])[sidx], group, axis=1)
    # the roles: the full slices hold pairs of BIG+ / BIG- in a random order, everything else is SMALL (a short last slice always)
    full = k // L
    P.roles = np.zeros((M, S), dtype=np.int64)
    for r in range(M):
        pairs = 1 if full < 4 else int(rng.integers(1, full // 2 + 1))
        where = rng.choice(full, 2 * pairs, replace=False)
        P.roles[r, where] = rng.permutation(np.repeat([1, -1], pairs))
    # the first rows (the problems of one row and of five) get the patterns that tell EVERY mutant apart by themselves, either sign first:
    # [SMALL, BIG, -BIG] where there are three full slices (ascending rounds the SMALL once, descending never, a carried chain twice),
    # [BIG, SMALL, -BIG, SMALL] repeated where there are four or more (pairwise rounds the second SMALL too)
    for r in range(min(8, M)):
        sign = 1 - 2 * (r % 2)
        P.roles[r] = 0
        if full < 4:
            P.roles[r, full - 2:full] = (sign, -sign)
        else:
            for g in range(0, full - 3, 4):
                P.roles[r, g], P.roles[r, g + 2] = sign, -sign
    big, small = FOLD_EXP[is_bf16]
    b = rng.integers(-3, 4, (M, L)) * (rng.random((M, L)) < 0.5)
    d = rng.integers(-3, 4, (M, S, L)) * (rng.random((M, S, L)) < 0.5)
    ints = np.where(P.roles[:, :, None] == 0, d, P.roles[:, :, None] * b[:, None, :]).reshape(M, S * L)[:, :k]
    scale = np.repeat(np.where(P.roles == 0, 2.0 ** small, 2.0 ** big), L, axis=1)[:, :k]
    P.a = ints * scale + 0.0
    P.a_bits = to_bits(P.a, is_bf16)
    P.bias = rng.integers(-100, 101, n) * 2.0 ** small                                          # (of the outputs' size; at most 7 bits)
    P.bias_bits = to_bits(P.bias, is_bf16)
    P.gs = FOLD_GS
    # float64, exact: the 128-k tile sums, and the slice sums p_s
    tiles = np.stack([P.a[:, j:j + 128] @ P.w[:, j:j + 128].T for j in range(0, k, 128)], axis=1) + 0.0      # [M, k / 128, n]
    P.tiles, P.tiles_per = tiles, L // 128
    P.p = np.stack([tiles[:, s * P.tiles_per:(s + 1) * P.tiles_per].sum(axis=1) for s in range(S)], axis=1) + 0.0   # [M, S, n]
    return P


def fold_bits(P, parts, use_gs, use_bias):
    """The definition in numpy float32, one operation at a time: parts [m, S', n] float32 added ascending, * gs, + bias, one RNE to 16 bits."""
    y = parts[:, 0].copy()
    for s in range(1, parts.shape[1]):
        y = y + parts[:, s]
    if use_gs:
        y = y * np.float32(P.gs)
    if use_bias:
        y = y + P.bias.astype(np.float32)[None, :]
    assert y.dtype == np.float32
    return f32_to_16(y, P.is_bf16)


def fold_expect(P, m, use_gs=True, use_bias=True, mutant=None):
    """Expected bits u16 [m, n]; mutant: one of MUTANTS, a wrong kernel's order instead."""
    p = P.p[:m].astype(np.float32)
    if mutant == "descending":
        p = p[:, ::-1]
    elif mutant == "pairwise":                                                                  # (p_0 + p_1) + (p_2 + p_3), level by level
        level = [p[:, s] for s in range(P.S)]
        while len(level) > 1:
            level = [level[i] + level[i + 1] if i + 1 < len(level) else level[i] for i in range(0, len(level), 2)]
        p = level[0][:, None]
    elif mutant == "moved boundary":                                                            # every inner boundary one k-tile of 128 later
        T, nt = P.tiles_per, P.tiles.shape[1]
        edges = [0] + [min(s * T + 1, nt) for s in range(1, P.S)] + [nt]
        p = np.stack([P.tiles[:m, edges[s]:edges[s + 1]].sum(axis=1) for s in range(P.S)], axis=1).astype(np.float32)
    elif mutant == "one chain":                                                                 # one accumulator carried across all slices
        y = np.zeros((m, P.n), dtype=np.float32)
        for j in range(P.tiles.shape[1]):
            y = y + P.tiles[:m, j].astype(np.float32)
        p = y[:, None]
    else:
        assert mutant is None
    return fold_bits(P, p, use_gs, use_bias)


def fold_shares(P, ms):
    """{mutant: the smallest share of changed outputs over the problems (m of ms) x (gs and bias, neither)}."""
    out = {}
    for name in MUTANTS:
        if name == "pairwise" and P.S == 3:
            continue                                              # (p_0 + p_1) + p_2 IS the definition: nothing to tell apart
        out[name] = min(float((fold_expect(P, m, *v, mutant=name) != fold_expect(P, m, *v)).mean()) for m in ms for v in ((True, True), (False, False)))
    return out


@functools.lru_cache(maxsize=None)
def fold_generator(kind, is_bf16, n, k):
    """The first seed at which every mutant changes at least one output in twenty of EVERY problem the GPU tests run (every M of the set, with
    and without gs and bias) -- a condition on the generator, as test_gated_contract.gated_problem's cap is."""
    ms = dense_ms(kind, is_bf16, n, k)
    for seed in range(FOLD_SEEDS):
        P = fold_draw(kind, is_bf16, n, k, seed)
        P.shares = fold_shares(P, ms)
        if min(P.shares.values()) >= SHARE:
            return P
    raise AssertionError(f"no seed below {FOLD_SEEDS} gives every mutant its share: {kind} bf16={is_bf16} n={n} k={k}")


def fold_problem(kind, is_bf16, m, n, k, seed=None):
    """-> Problem of m rows for InvariantDevice: operands, p [m, S, n] (float32-exact slice sums), want (gs and bias)."""
    G = fold_generator(kind, is_bf16, n, k) if seed is None else fold_draw(kind, is_bf16, n, k, seed)
    P = Problem()
    P.__dict__.update(G.__dict__)
    P.m, P.a, P.a_bits, P.p = m, G.a[:m], G.a_bits[:m], G.p[:m]
    P.want = fold_expect(G, m)
    return P


# --- leg X: two roundings against one ------------------------------------------------------------------------------------------------------------------

ROUND_N, ROUND_K = 32, 256
# j of gs = (1 + 2^-23) 2^j.  Plain: the cancelling outputs, 1 or 2 ulp32(acc 2^j) >= 2^(j - 24), are normal numbers of the output type.
# Gated (activation, bf16): SiLU-mul multiplies the tiny up value by silu(gate) = O(1..40), so j keeps the gates of the chosen rows small;
# SwiGLU-OAI adds 1 to the up value, so the up value itself must reach the last bits of 1 + u in the output type: j as large as the 16-bit
# bias -acc 2^j allows (bf16: any; fp16: |acc| 2^j < 65504).
ROUND_J = {(0, True): 0, (0, False): 10, (1, True): 0, (1, False): 2, (2, True): 20, (2, False): 11}
ROUND_GATED_MS = (17, 129)


def mant_ulps(acc):
    """mant(acc) in [1, 2) (0 where acc is 0): what acc (1 + 2^-23) - acc is in units of ulp32(acc)."""
    return np.abs(np.frexp(acc)[0]) * 2.0


@functools.lru_cache(maxsize=None)
def rounding_problem(kind, is_bf16, m, act=0):
    with np.errstate(over="ignore"):                                                            # (exp of a far gate: the float64 model's inf is meant)
        return _rounding_problem(kind, is_bf16, m, act)


def _rounding_problem(kind, is_bf16, m, act):
    """Regime "A" of exact_problem at K = 256, n = 32 (|acc| < 128 in multiples of 1/2), gs = (1 + 2^-23) 2^j, and in every column n (gated: every
    column of the up half; the gate half has regime G's ordinary bias) bias[n] = -acc[r_n][n] 2^j for ONE row r_n: at (r_n, n) the plain
    contract f32(f32(acc gs) + bias) leaves 1 or 2 ulp32(acc 2^j), the gated contract's fma(acc, gs, bias) mant(acc) ulp.
    -> Problem with want (plain: bits; gated: test_gated_contract.expect's want / alt / wrong), chosen [(r_n, n)], and `swapped`: the bits the
    other formula would give."""
    from test_gated_contract import band, gated64, round16, bits16
    n, k = ROUND_N, ROUND_K
    B = exact_problem(kind, is_bf16, m, n, k, "A", 0)
    P = Problem()
    P.__dict__.update(B.__dict__)
    j = ROUND_J[(act, is_bf16)]
    P.gs = float(np.float32((1.0 + 2.0 ** -23) * 2.0 ** j))
    assert P.gs == (1.0 + 2.0 ** -23) * 2.0 ** j
    acc = B.acc
    assert np.abs(acc).max() < 128 and np.array_equal(np.rint(acc * 2), acc * 2)
    prod = acc * P.gs                                                                          # 8 + 24 bits: exact in float64
    one = prod.astype(np.float32).astype(np.float64)                                            # the multiply's rounding
    limit = 3e38 if is_bf16 else 65504.0
    rng = np.random.default_rng([kind == "mx", is_bf16, m, act, 0x2B1])
    nh = n // 2
    cols = range(n) if act == 0 else range(nh, n)
    bias = np.zeros(n)
    if act:
        bias[:nh] = rng.integers(16, 33, nh) * 2.0 ** -4
        yg = (two_sum_odd(prod[:, :nh], np.broadcast_to(bias[None, :nh], (m, nh)).copy())[0]).astype(np.float32).astype(np.float64)
        u_fma, u_two = acc[:, nh:] * 2.0 ** (j - 23), one[:, nh:] - acc[:, nh:] * 2.0 ** j      # what is left at (r, n) were r the chosen row
        ref_f, ref_t, d = gated64(yg, u_fma, act), gated64(yg, u_two, act), band(yg, act)
        tiny = 2.0 ** -126 if is_bf16 else 2.0 ** -14

        def r16(v):                                                                             # (a tiny reference: 1.0, and `normal` leaves it out)
            return round16(np.where(np.abs(v) >= tiny, v, 1.0), is_bf16)
        normal = (np.abs(ref_f) >= tiny) & (np.abs(ref_t) >= tiny)
        seen = normal & (r16(ref_t) != r16(ref_f * (1 - d))) & (r16(ref_t) != r16(ref_f * (1 + d)))       # the band does not reach the other formula's value
    P.chosen = []
    for col in cols:
        order = [(col + i) % m for i in range(m)]
        ok = [r for r in order if acc[r, col] != 0 and abs(acc[r, col]) * 2.0 ** j < limit]
        if act:
            best = [r for r in ok if seen[r, col - nh]]
        else:
            best = [r for r in ok if mant_ulps(acc[r, col]) != 1.0]
        r = (best or ok or order)[0]
        if acc[r, col] != 0 and abs(acc[r, col]) * 2.0 ** j < limit:                        # (else: no bias in this column)
            bias[col] = -acc[r, col] * 2.0 ** j
            P.chosen.append((r, col))
    P.bias, P.bias_bits = bias, to_bits(bias, is_bf16)                                          # (to_bits asserts that the bias is representable)
    rows, cc = np.array([r for r, _ in P.chosen]), np.array([c for _, c in P.chosen])
    y_fma = two_sum_odd(prod, np.broadcast_to(bias[None, :], prod.shape).copy())[0].astype(np.float32)     # one rounding of the exact sum
    with np.errstate(over="ignore"):
        y_two = one.astype(np.float32) + bias.astype(np.float32)[None, :]                                  # two roundings
    # at the chosen outputs: the fma leaves mant(acc) ulp32(acc 2^j) exactly, the two roundings 1 or 2 of them
    ulp = 2.0 ** (np.frexp(acc[rows, cc])[1] - 1 + j - 23)
    assert np.array_equal(np.abs(y_fma[rows, cc].astype(np.float64)), mant_ulps(acc[rows, cc]) * ulp)
    assert np.isin(np.abs(y_two[rows, cc].astype(np.float64)) / ulp, (1.0, 2.0)).all()
    if act == 0:
        P.want, P.swapped = f32_to_16(y_two, is_bf16), f32_to_16(y_fma, is_bf16)
        at = P.want[rows, cc]
        assert ((at & 0x7FFF) >= (0x0080 if is_bf16 else 0x0400)).all() and ((at & 0x7FFF) < INF_BITS[is_bf16]).all()    # normal numbers
        P.share = float((P.want[rows, cc] != P.swapped[rows, cc]).mean())
    else:
        P.y = y_fma.astype(np.float64)
        expect(P, is_bf16, act)
        Q = Problem()
        Q.y = np.concatenate([P.y[:, :nh], y_two[:, nh:].astype(np.float64)], axis=1)
        P.swapped = bits16(round16(gated64(Q.y[:, :nh], Q.y[:, nh:], act), is_bf16), is_bf16)
        P.share = float(P.wrong(P.swapped).reshape(m, nh)[rows, cc - nh].mean())
    return P


# --- CPU tests ---------------------------------------------------------------------------------------------------------------------------------------------

def test_fp16_mxfp4_is_refused():
    """The fourth family has no batch-invariant kernel: the query is 0 and both entries return PETIT_ERROR_KERNEL_SHAPE before any launch."""
    L = _lib()
    ptr, fp16, mx = C.c_void_p(0x1000), L.CXX_DTYPE_FP16, L.CXX_DTYPE_MXFP4_E2M1
    hints = L.SolutionHints(fp16, mx, fp16, 0)
    assert L.lib.petit_gemm_invariant_workspace_bytes(4, 32, 256, fp16, mx) == 0
    assert L.lib.petit_gemm_mxfp4_fp16_invariant(ptr, ptr, ptr, ptr, ptr, 4, 32, 256, C.byref(hints), None, ptr, None) == L.PETIT_ERROR_KERNEL_SHAPE
    assert L.lib.petit_gemm_moe_invariant_workspace_bytes(2, 4, 32, 256, fp16, mx) == 0
    assert L.lib.petit_gemm_mxfp4_fp16_moe_invariant(ptr, ptr, ptr, ptr, ptr, ptr, 2, 4, 32, 256, None, 4, None, 4, C.byref(hints), None, ptr,
                                                     None) == L.PETIT_ERROR_KERNEL_SHAPE
    assert L.lib.petit_gemm_fp4_invariant_host(ptr, ptr, ptr, ptr, None, None, 4, 32, 256, fp16, mx) == L.PETIT_ERROR_KERNEL_SHAPE


@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_table_m_sets_cover_every_pair(kind, is_bf16):
    """The assertions of test_value_contract.test_table_generator_coverage_and_preconditions for every M of the dense set (those of its own MS
    included: the set is read from the library): the series of every (M, K) reads every (code, scale byte) pair and both signs of every
    activation class; the N of the tables has S = 1, 5 and 8 slices over KS."""
    need = required_pairs(kind)
    n = TABLE_N[kind]
    assert [geometry(kind, is_bf16, n, k)[0] for k in KS] == [1, 5, 8]
    for k in KS:
        ms = dense_ms(kind, is_bf16, n, k)
        assert len(ms) == 8 and set(ms) - set(VALUE_MS), ms
        for m in ms:
            series = table_series(kind, is_bf16, m, k)
            assert pairs_read(series) == need, (kind, is_bf16, m, k, sorted(need ^ pairs_read(series))[:8])
            seen = {c for P in series for c in P.classes}
            assert seen == {(nm, sg) for nm in activation_classes(is_bf16, False) for sg in (0, 1)}, (kind, is_bf16, m, k, seen)
            for P in series:
                assert (P.a_bits != 0).sum(axis=1).tolist() == [1] * m


@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_table_expectation_two_roundings(kind, is_bf16):
    """Where the plain invariant call's bits (two roundings) are not table_expect's (one): only in sets with a bias and a gs that is no power
    of two, and there in a handful of outputs -- printed per K; at least one per family, so the distinction is not idle."""
    total = 0
    for k in KS:
        per_k, outs = 0, 0
        for m in dense_ms(kind, is_bf16, TABLE_N[kind], k):
            for P in table_series(kind, is_bf16, m, k):
                Q = table_problem(P, is_bf16)
                count = int(Q.differs.sum())
                assert count == 0 or (P.bias_bits is not None and np.frexp(abs(P.gs))[0] != 0.5), (kind, is_bf16, m, k, P.set)
                assert np.array_equal(Q.must_nan, P.must_nan) and not (Q.want[~Q.must_nan] == POISON[is_bf16]).any()
                per_k, outs = per_k + count, outs + Q.want.size
        print(f"invariant_contract tables {kind} bf16={is_bf16} k={k}: {per_k} of {outs} expected outputs differ between two roundings and one")
        total += per_k
    assert total > 0 or not is_bf16


def table_twin_failures(kind, is_bf16, k, ms):
    n = TABLE_N[kind]
    T0 = table_series(kind, is_bf16, ms[0], k)[0].T
    packed = packed_cpu(kind, T0.q, T0.s, n, k)
    failures, sets = [], 0
    for m in ms:
        for P in table_series(kind, is_bf16, m, k):
            Q = table_problem(P, is_bf16)
            got = twin(kind, is_bf16, packed, P.a_bits, P.gs, P.bias_bits, n, k)
            bad = judge(got, Q.want, is_bf16, Q.must_nan, Q.is_zero)
            sets += 1
            if bad.any():
                r, c = np.argwhere(bad)[0]
                kp = P.kappa[r]
                failures.append(f"m={m} k={k} set {P.set}: {int(bad.sum())} outputs differ, first at (row {r}, col {c}): got {got[r, c]:#06x} want "
                                f"{Q.want[r, c]:#06x}; a = {P.a_bits[r, kp]:#06x} at k {kp}, code {P.T.code[c, kp]} scale byte {P.T.s[c, kp // P.T.group]:#04x}, "
                                f"gs {P.gs!r}")
    return failures, sets


@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_twin_equals_the_tables(kind, is_bf16):
    """petit_gemm_fp4_invariant_host on every table problem of the dense M sets, judged as the device is: every scale byte, e8m0 byte 0 as
    2^-127 (where `byte << 23` gave 0.0: every |code| >= 2 column under byte 0 was wrong), byte 255 and e4m3 0x7F / 0xFF a NaN column, the
    twenty excluded pairs zero weights."""
    for k in KS:
        failures, sets = table_twin_failures(kind, is_bf16, k, dense_ms(kind, is_bf16, TABLE_N[kind], k))
        assert not failures, f"{len(failures)} of {sets} sets wrong:\n" + "\n".join(failures[:10])
    if kind == "mx":                                   # byte 0 is met with a non-zero weight, byte 255 exactly once
        T = table_series(kind, is_bf16, 1, KS[0])[0].T
        s_k = np.repeat(T.s, 32, axis=1)
        assert ((s_k == 0) & (T.w != 0)).any() and (T.s == 255).sum() == 1 and (np.abs(T.w[(s_k == 0) & (T.w != 0)]) == 2.0 ** -127 * np.abs(
            FP4[T.code[(s_k == 0) & (T.w != 0)]])).all()


def moe_table_problem(kind, is_bf16, k, counts, i):
    """Leg V on the MoE entry, activation set i: experts 0 and 2 hold the table W under the sets i and i + 1 of their row counts' series,
    expert 1 a regime-B W and regime-B rows (its last row reads an out-of-range A index: zeros, so that row is round16(bias)); a rowless
    fourth expert pads the stack."""
    n = TABLE_N[kind]
    c0, c1, c2 = counts
    s0, s2 = table_series(kind, is_bf16, c0, k), table_series(kind, is_bf16, c2, k)
    P0, P2 = table_problem(s0[i % len(s0)], is_bf16), table_problem(s2[(i + 1) % len(s2)], is_bf16)
    B = exact_problem(kind, is_bf16, c1, n, k, "B", i)
    b_a, b_want = B.a_bits.copy(), B.want.copy()
    b_a[c1 - 1], b_want[c1 - 1] = 0, B.bias_bits
    none = np.zeros((c1, n), dtype=bool)
    experts = [(P0.q, P0.s, P0.gs, P0.bias_bits, P0.want, P0.must_nan, P0.is_zero), (B.q, B.s, B.gs, B.bias_bits, b_want, none, none),
               (P2.q, P2.s, P2.gs, P2.bias_bits, P2.want, P2.must_nan, P2.is_zero)]
    src, index = gather(np.concatenate([P0.a_bits, b_a, P2.a_bits]), i, c0 + c1 - 1)
    return moe_stack(kind, is_bf16, n, k, experts, (B.q, B.s), src, index, seed=i), max(len(s0), len(s2))


def scattered(P, c_index, c_rows, what):
    named = (c_index >= 0) & (c_index < c_rows)
    out = np.full((c_rows, P.n), POISON[P.is_bf16], dtype=np.uint16) if what.dtype == np.uint16 else np.zeros((c_rows, P.n), dtype=bool)
    out[c_index[named]] = what[named]
    return out


def moe_twin(P, c_index, c_rows, use_gs_bias=True):
    """petit_gemm_fp4_moe_invariant_host on a moe_stack problem -> bits u16 [c_rows, n] over a poisoned C."""
    packs = [packed_cpu(P.kind, P.q[e * P.n:(e + 1) * P.n], P.s[e * P.n:(e + 1) * P.n], P.n, P.k) for e in range(P.E)]
    b = torch.cat([p[0].reshape(-1).view(torch.uint8) for p in packs]).contiguous()
    sp = torch.cat([p[1].reshape(-1).view(torch.uint8) for p in packs]).contiguous()
    out = np.full((c_rows, P.n), POISON[P.is_bf16], dtype=np.uint16)
    gs, off = np.ascontiguousarray(P.gs.astype(np.float32)), np.array(P.offsets, dtype=np.int32)
    a, bias, ai, ci = (np.ascontiguousarray(v) for v in (P.a_src_bits, P.bias_bits, P.a_index, c_index))
    rc = _lib().lib.petit_gemm_fp4_moe_invariant_host(out.ctypes.data, a.ctypes.data, b.data_ptr(), sp.data_ptr(), gs.ctypes.data, bias.ctypes.data,
                                                      off.ctypes.data, P.E, P.m, P.n, P.k, ai.ctypes.data, a.shape[0], ci.ctypes.data, c_rows,
                                                      *type_codes(P.kind, P.is_bf16))
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_moe_twin_equals_the_tables(kind, is_bf16):
    """The MoE twin inherits the dense twin's decode: the stacked table problems of the GPU test (both forms' row counts, K = 1280), rows of
    no C index and the skipped row still poison."""
    k = 1280
    for form, counts in moe_counts().items():
        i, sets = 0, 1
        while i < sets:
            (P, c_index, c_rows), sets = moe_table_problem(kind, is_bf16, k, counts, i)
            got = moe_twin(P, c_index, c_rows)
            bad = judge(got, scattered(P, c_index, c_rows, P.want), is_bf16, scattered(P, c_index, c_rows, P.must_nan), scattered(P, c_index, c_rows, P.is_zero))
            assert not bad.any(), (kind, is_bf16, form, i, int(bad.sum()), np.argwhere(bad)[0])
            i += 1


def fold_preconditions(G, tag):
    big, small = FOLD_EXP[G.is_bf16]
    S, L, k = G.S, G.L, G.k
    assert G.w.shape == (G.n, k) and np.array_equal(G.w[:, L:], G.w[:, :k - L]), tag                    # periodic in L
    assert {0.5, 1.5, 6.0, 24.0} <= set(np.abs(G.w).reshape(-1).tolist()), tag
    vals = values16(G.a_bits, G.is_bf16)
    assert np.array_equal(vals, G.a), tag
    nz = np.abs(G.a[G.a != 0])
    lo = 2.0 ** -126 if G.is_bf16 else 2.0 ** -14
    assert nz.min() >= lo and nz.max() < (3e38 if G.is_bf16 else 65504.0), tag                           # normal 16-bit numbers
    p32 = G.p.astype(np.float32)
    assert np.array_equal(p32.astype(np.float64), G.p), tag                                              # every p_s is an fp32 number
    for s in range(S):
        sl = slice(s * L, min(k, (s + 1) * L))
        role = G.roles[:, s]
        quantum = np.where(role == 0, 2.0 ** small, 2.0 ** big) / 2
        a = G.a[:, sl]
        assert np.array_equal(np.rint(a / (2 * quantum[:, None])), a / (2 * quantum[:, None])), tag      # integers times the role's power of two
        assert ((np.abs(a) @ np.abs(G.w[:, sl]).T) / quantum[:, None]).max() < 2 ** 24, tag              # any in-slice order is exact
    assert (G.roles.sum(axis=1) == 0).all() and (np.abs(G.roles).sum(axis=1) >= 2).all(), tag            # the BIGs cancel in total
    if k % L:
        assert (G.roles[:, -1] == 0).all(), tag
    for r in range(G.a.shape[0]):
        plus, minus = np.flatnonzero(G.roles[r] == 1), np.flatnonzero(G.roles[r] == -1)
        assert np.array_equal(G.p[r, minus[0]], -G.p[r, plus[0]]) and all(np.array_equal(G.p[r, s], G.p[r, plus[0]]) for s in plus), tag
    # ulp32 of a typical BIG partial is at least 2^3 quanta of a SMALL partial
    typical = np.median(np.abs(G.p[G.roles != 0][G.p[G.roles != 0] != 0]))
    assert 2.0 ** (np.frexp(typical)[1] - 24) >= 2.0 ** 3 * 2.0 ** small / 2, tag


@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_fold_generator_preconditions_teeth_and_twin(kind, is_bf16):
    """fold_problem's preconditions, the shares of outputs each wrong order changes (>= 1 in 20 of EVERY problem the GPU tests run; printed),
    and (a): the CPU twin equals the expectation bit for bit, with and without gs and bias."""
    for n, k in fold_shapes(kind):
        G = fold_generator(kind, is_bf16, n, k)
        tag = f"{kind} bf16={is_bf16} n={n} k={k} S={G.S} L={G.L} seed={G.seed}"
        fold_preconditions(G, tag)
        assert G.S == {768: 3, 1024: 4, 4352: 9}[k] and (k != 4352 or (G.L == 512 and k % G.L == 256)), tag
        print(f"invariant_contract fold {tag}: smallest share of changed outputs " + ", ".join(f"{nm} {100 * v:.1f} %" for nm, v in G.shares.items()))
        assert min(G.shares.values()) >= SHARE and set(G.shares) == set(MUTANTS) - ({"pairwise"} if G.S == 3 else set()), tag
        if G.S == 3:
            assert np.array_equal(fold_expect(G, FOLD_ROWS, mutant="pairwise"), fold_expect(G, FOLD_ROWS)), tag
        packed = packed_cpu(kind, G.q, G.s, n, k)
        m = 33
        for use_gs, use_bias in ((True, True), (False, False), (True, False)):
            got = twin(kind, is_bf16, packed, G.a_bits[:m], G.gs if use_gs else None, G.bias_bits if use_bias else None, n, k)
            assert np.array_equal(got, fold_expect(G, m, use_gs, use_bias)), (tag, use_gs, use_bias)


@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_rounding_generator_teeth_and_twin(kind, is_bf16):
    """rounding_problem: at the chosen outputs the two formulas differ in at least one output in twenty of every problem the GPU tests run
    (plain: bits; gated: the other formula's bits are outside what the band accepts) -- printed; the CPU twin, a plain call, rounds twice."""
    ms = dense_ms(kind, is_bf16, ROUND_N, 1024)
    for m in ms:
        P = rounding_problem(kind, is_bf16, m, 0)
        assert len(P.chosen) >= (ROUND_N * 3) // 4 and P.share >= SHARE, (kind, is_bf16, m, len(P.chosen), P.share)
        got = twin(kind, is_bf16, packed_cpu(kind, P.q, P.s, ROUND_N, ROUND_K), P.a_bits, P.gs, P.bias_bits, ROUND_N, ROUND_K)
        assert np.array_equal(got, P.want), (kind, is_bf16, m)
    shares = {f"plain m={m}": rounding_problem(kind, is_bf16, m, 0).share for m in ms}
    for act in (1, 2):
        for m in ROUND_GATED_MS:
            P = rounding_problem(kind, is_bf16, m, act)
            assert len(P.chosen) >= ROUND_N // 4 and P.share >= SHARE, (kind, is_bf16, act, m, len(P.chosen), P.share)
            shares[f"act {act} m={m}"] = P.share
    print(f"invariant_contract rounding {kind} bf16={is_bf16}: share of the chosen outputs the other formula changes: " +
          ", ".join(f"{nm} {100 * v:.0f} %" for nm, v in shares.items()))


# --- GPU tests: leg V ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_tables_dense_both_forms(pk, kind, is_bf16, k):
    """Leg V.1: every activation set of every M of the set through the dense entry, judged as ValueDevice judges; S = 1, 5, 8."""
    n, counts, failures, t0 = TABLE_N[kind], new_counts(), [], time.time()
    for m in dense_ms(kind, is_bf16, n, k):
        for P in table_series(kind, is_bf16, m, k):
            D = InvariantValueDevice(pk, kind, is_bf16, m, n, k, table_problem(P, is_bf16))
            report = D.run()
            counts_for(counts, D)
            if report:
                failures.append(f"set {P.set}: {report}")
    finish(f"tables {kind} bf16={is_bf16} k={k}", counts, failures, t0)


@pytest.mark.gpu
@pytest.mark.parametrize("activation", (0, 1))
def test_shifted_e8m0_both_forms(pk, activation):
    """Leg V.4: bf16 x MXFP4 with every e8m0 byte moved by +-100 (bytes 26..29 and 226..229) and gs moved back, K = 1280: the unshifted
    problem's bits, zero tolerance; SiLU-mul under test_gated_contract's band."""
    from test_gated_contract import CAP, check_preconditions, gated_problem
    n, k, counts, failures, t0 = 288, 1280, new_counts(), [], time.time()
    for m in dense_ms("mx", True, n, k):
        if activation:
            problems = [(f"F{d:+d}", gated_problem("mx", True, m, n, k, 1, mx_shift=d)) for d in SHIFTS[True]]
        else:
            problems = shifted_and_switched(True, m, n, k)
        for name, P in problems:
            assert name[0] == "F" and (int(P.s.min()) < 40 or int(P.s.max()) > 214)
            if activation:
                check_preconditions(P, True, (name, m))
                assert P.undecided <= CAP[True]
            D = (InvariantGatedDevice if activation else InvariantValueDevice)(pk, "mx", True, m, n, k, P, activation)
            report = D.run()
            counts_for(counts, D)
            if report:
                failures.append(f"{name}: {report}")
    finish(f"shifted e8m0 activation {activation}", counts, failures, t0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_nonfinite_activations_both_forms(pk, kind, is_bf16):
    """Leg V.5: +-inf and NaN activations (test_value_contract's injections on regime B, K = 1280): every output of an injected row by its
    class, clean rows by bits."""
    n, k, counts, failures, t0 = TABLE_N[kind], 1280, new_counts(), [], time.time()
    for m in dense_ms(kind, is_bf16, n, k):
        for name, base in nonfinite_bases(kind, is_bf16, m, k):
            for i, v in enumerate(injections(is_bf16, m, k)):
                D = InvariantValueDevice(pk, kind, is_bf16, m, n, k, nonfinite_problem(base, is_bf16, v))
                report = D.run()
                counts_for(counts, D)
                if report:
                    failures.append(f"{name} variant {i}: {report}")
    finish(f"nonfinite {kind} bf16={is_bf16}", counts, failures, t0)


def moe_finish(tag, counts, failures, t0):
    print(f"invariant_contract {tag}: launches {counts}, {time.time() - t0:.1f} s")
    assert counts["split"] and counts["whole"], ("a form did not run", counts)
    assert not failures, f"{len(failures)} launches wrong:\n" + "\n".join(failures[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_tables_moe_both_forms(pk, kind, is_bf16, k):
    """Leg V.6: the table W on experts 0 and 2 of a stack of three with rows (and a rowless fourth), a plain W between them; gathered A with
    one out-of-range index, scattered C with one out-of-range index; rows of no C index stay poison."""
    counts, failures, t0 = new_counts(), [], time.time()
    for form, rows in moe_counts().items():
        i, sets = 0, 1
        while i < sets:
            (P, c_index, c_rows), sets = moe_table_problem(kind, is_bf16, k, rows, i)
            D = MoeInvariantDevice(pk, P, c_index=c_index, c_rows=c_rows)
            assert D.split == (form == "split")
            report = D.run()
            counts[form] += 1
            if report:
                failures.append(f"set {i}: {report}")
            i += 1
    moe_finish(f"moe tables {kind} bf16={is_bf16} k={k}", counts, failures, t0)


# --- GPU tests: leg X ------------------------------------------------------------------------------------------------------------------------------------

def slab_report(D, p, tag):
    """(c): slab s of the workspace holds p_s, exactly, for every s."""
    got = D.slab_values()
    if np.array_equal(got, p):
        return []
    bad = np.argwhere(~(got == p))
    s, r, c = bad[0]
    per_slab = [int((~(got[i] == p[i])).sum()) for i in range(got.shape[0])]
    return [f"{tag}: {len(bad)} slab values are not their slice's sum (per slab: {per_slab}); first at slab {s} (row {r}, col {c}): got {got[s, r, c]!r} "
            f"want {p[s, r, c]!r}"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_fold_order_dense_both_forms(pk, kind, is_bf16):
    """Leg X (b), (c): the dense entry gives fold_problem's bits for every M of the set, with gs and bias, with neither, with gs alone; in the
    split form slab s of the caller's workspace is p_s."""
    counts, failures, t0 = new_counts(), [], time.time()
    for n, k in fold_shapes(kind):
        for m in dense_ms(kind, is_bf16, n, k):
            P = fold_problem(kind, is_bf16, m, n, k)
            for use_gs, use_bias in ((True, True), (False, False), (True, False)):
                P.want = fold_expect(P, m, use_gs, use_bias)
                D = InvariantDevice(pk, kind, is_bf16, m, n, k, P)
                report = D.run(use_gs, use_bias)
                counts_for(counts, D)
                failures += [report] if report else []
                if not D.whole:
                    failures += slab_report(D, np.transpose(P.p, (1, 0, 2)).astype(np.float32), f"m={m} n={n} k={k}")
    finish(f"fold {kind} bf16={is_bf16}", counts, failures, t0)


def moe_fold_problem(kind, is_bf16, n, k, rows):
    """Three experts with rows, each its own fold draw (W, gs 2^(e - 1) FOLD_GS, bias), expert e's rows the first rows of its draw; the last
    row of expert 1 reads an out-of-range A index.  -> ((Problem, c_index, c_rows), p [S, m, n] of the grouped rows)."""
    experts, a_rows, ps = [], [], []
    for e, count in enumerate(rows):
        G0 = fold_generator(kind, is_bf16, n, k) if e == 0 else fold_draw(kind, is_bf16, n, k, 100 + e)
        G = Problem()
        G.__dict__.update(G0.__dict__)
        G.gs = FOLD_GS * 2.0 ** (e - 1)
        p, a_bits = G0.p[:count].copy(), G0.a_bits[:count].copy()
        if e == 1:
            p[count - 1], a_bits[count - 1] = 0.0, 0
        none = np.zeros((count, n), dtype=bool)
        experts.append((G.q, G.s, G.gs, G.bias_bits, fold_bits(G, p.astype(np.float32), True, True), none, none))
        a_rows.append(a_bits)
        ps.append(p)
    src, index = gather(np.concatenate(a_rows), k + n, rows[0] + rows[1] - 1)
    return moe_stack(kind, is_bf16, n, k, experts, experts[1][:2], src, index, seed=k), np.transpose(np.concatenate(ps), (1, 0, 2)).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_fold_order_moe_both_forms(pk, kind, is_bf16):
    """Leg X (c), (d): the MoE entry gives the fold bits of every owned row in both forms; the split form's slabs, indexed by grouped row, hold
    p_s of that row under its expert."""
    counts, failures, t0 = new_counts(), [], time.time()
    for n, k in fold_shapes(kind):
        for form, rows in moe_counts().items():
            (P, c_index, c_rows), p = moe_fold_problem(kind, is_bf16, n, k, rows)
            D = MoeInvariantDevice(pk, P, c_index=c_index, c_rows=c_rows)
            assert D.split == (form == "split")
            report = D.run()
            counts[form] += 1
            failures += [report] if report else []
            if D.split:
                failures += slab_report(D, p, f"moe n={n} k={k}")
    moe_finish(f"moe fold {kind} bf16={is_bf16}", counts, failures, t0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_plain_call_rounds_twice_gated_calls_once(pk, kind, is_bf16):
    """rounding_problem: the plain call by bits in both forms (every M of the set); SiLU-mul and SwiGLU-OAI under the band, whose accepted
    values exclude the two-rounding formula's at the chosen outputs (the CPU teeth test)."""
    counts, failures, t0 = new_counts(), [], time.time()
    for m in dense_ms(kind, is_bf16, ROUND_N, 1024):
        D = InvariantDevice(pk, kind, is_bf16, m, ROUND_N, ROUND_K, rounding_problem(kind, is_bf16, m, 0))
        report = D.run()
        counts_for(counts, D)
        failures += [report] if report else []
    for act in (1, 2):
        for m in ROUND_GATED_MS:
            D = InvariantGatedDevice(pk, kind, is_bf16, m, ROUND_N, ROUND_K, rounding_problem(kind, is_bf16, m, act), act)
            report = D.run()
            counts_for(counts, D)
            failures += [f"activation {act}: {report}"] if report else []
    finish(f"rounding {kind} bf16={is_bf16}", counts, failures, t0)

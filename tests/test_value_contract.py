"""The dense GEMMs over their whole value domain, every kernel id, bit for bit: the method and the plumbing of test_exact_contract.py (inputs on
which the 16 output bits are unique in any summation order, caller-owned poisoned and guarded C and scratch, every id and accepted K split through
the C ABI) carried from five block scales and small integers to every scale byte, the ends of the activation types, the fp16 x MXFP4 fallback
body and its switch, and non-finite activations.  Shapes: N = 272 (NVFP4) / 288 (MXFP4), K in KS, M in MS.

Leg 1, truth tables.  Row r of A holds ONE non-zero value a_r at column kappa(r): every partial sum in any kernel is zero plus one product, so
c[r][n] = RNE16(RNE32(a_r w[n][kappa(r)] gs + bias[n])) whatever the order or split.  One W per (family, K) (table_layout): code (n + k) mod 16,
scale byte a function of (16-row tile | 8-row half tile, block class), so that the pairs (code, scale byte) the non-zero activations of a problem
series read cover 16 codes x every scale byte.  The expected value is exact: a w has <= 17 significant bits (asserted), gs <= 24, so a w gs is a
float64; the bias is added with an error-free sum (two_sum_odd) and rounded to odd, which makes the following RNE to float32 the RNE of the exact sum
(53 >= 24 + 2), where the float64 sum is not already exact (the bias is drawn next to the product of ONE row per column; a column's other rows
have products up to 250 binades away).  Then float32 -> the output type by O.f32_to_bf16_bits / numpy's float16 conversion: fp16 overflow to inf
and fp16 subnormal outputs are in scope.  Zeros compare by value, outputs that must be NaN as "a NaN that is not the poison", the rest by bits.
  * the generator's condition, asserted for every non-zero product (c the code value, s the block scale): |a c|, |a c 2^-7|, |a c s| and
    |y| = |a c s gs| in [2^-126, 2^127) -- the bf16 decode kernels form a c 2^-7 and any kernel may form a c before s -- AND |c s| in
    [2^-126, 2^128): most kernels form the weight c s first, in bf16 or fp32, where the oracle's own dequant has a subnormal or inf.  fp32
    subnormals are mode-dependent and no part of the contract.  This excludes bf16 activations below 2^-118 and above 2^127 / 6 (the "largest"
    and "smallest" bf16 activations are those two ends; flushing of bf16 subnormals is out of scope) and the twenty MXFP4 pairs
    (byte 0, |c| <= 1.5), (byte 1, |c| = .5), (byte 253, |c| >= 4), (byte 254, |c| >= 2), whose codes are zeroed in W (an inf weight times the
    zero activations of every other row would make the whole column NaN).
  * e4m3 bytes 0x7F / 0xFF and e8m0 byte 255 sit once each in a column of their own: NaN x 0 = NaN, so that column is NaN in every row, in the
    oracle's reading of byte 255 (2^128 = inf, inf x 0) as in the hardware's.  e8m0 byte 0 is 2^-127 (test_e8m0_zero_scale_divergence_is_pinned).
Leg 2: regimes "F" (every e8m0 byte shifted, gs shifted back) and "S" (zero blocks under a scale byte outside 114..140) of exact_problem, zero
tolerance; the same through the gated machinery (SiLU-mul, its band unchanged).  Leg 3: +-inf and NaN activations on regime B / F / S, the class
(NaN, +inf, -inf) of every output of an injected row derived term by term, without a sum.
"""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_exact_contract import DEV, FAMILIES, FP4, POISON, Device, exact_ids, exact_problem, native_ids, pk, run_ids  # noqa: F401

KS = (256, 1280, 2048)
MS = (1, 2, 3, 4, 5, 8, 16, 17, 40, 128, 129, 257)
TABLE_N = {"nv": 272, "mx": 288}
TABLE_ROWS = {"nv": 256, "mx": 272}              # rows of W that carry the table; behind them plain rows and the NaN-scale rows
INF_BITS = {True: 0x7F80, False: 0x7C00}
LO, HI = 2.0 ** -126, 2.0 ** 127


def values16(bits, is_bf16):
    return (O.bf16_bits_to_f32(bits) if is_bf16 else O.f16_bits_to_f32(bits)).astype(np.float64)


def scale_value(kind, byte):
    """The block scale a byte means, float64: e4m3 by the oracle (sign-bit bytes negative, 0x7F / 0xFF NaN); e8m0 2^(byte - 127) with byte 0 the
    hardware's 2^-127 and byte 255 NaN."""
    byte = np.asarray(byte)
    if kind == "nv":
        return O.e4m3_to_f32(byte.astype(np.uint8)).astype(np.float64)
    return np.where(byte == 255, np.nan, np.ldexp(1.0, byte.astype(np.int64) - 127))


# --- leg 1: the generator ------------------------------------------------------------------------------------------------------------------

class Layout:
    pass


@functools.lru_cache(maxsize=None)
def table_layout(kind, k):
    """The one W of (family, K).  Blocks (16 k NVFP4, 32 k MXFP4) fall into `classes` classes, block b into class b mod classes; G consecutive
    rows (16, or 8 where K has too few blocks for that: MXFP4 at K = 256) share a scale byte per class, G rows x `per_block` columns per block
    (kappa and kappa + 8 mod 16) see all 16 codes of (n + k) mod 16 under it."""
    T = Layout()
    T.kind, T.k, T.n, T.group, rows = kind, k, TABLE_N[kind], 16 if kind == "nv" else 32, TABLE_ROWS[kind]
    T.nb = k // T.group
    T.bytes = np.array(list(range(0, 127)) + list(range(0x80, 0xFF)) if kind == "nv" else list(range(0, 255)))
    for T.per_block in (1, 2):
        T.g = 16 // T.per_block
        per_class = rows // T.g
        T.classes = -(-len(T.bytes) // per_class)
        if T.classes <= T.nb:
            break
    assert T.classes <= T.nb, (kind, k)
    T.types = T.classes * T.per_block                                                # column types a problem series has to read
    cls = np.arange(T.nb) % T.classes
    idx = np.minimum(cls[None, :] * per_class + (np.arange(rows) // T.g)[:, None], len(T.bytes) - 1)       # (the last byte again where the table ends)
    plain = 0x38 if kind == "nv" else 127                                             # scale 1
    T.s = np.full((T.n, T.nb), plain, dtype=np.uint8)
    T.s[:rows] = T.bytes[idx]
    if kind == "mx":
        T.s[rows:] = (121 + np.arange(T.n - rows) % 6)[:, None]                       # (a tile inside 114..140, the fast fp16 body, that bars no activation)
    else:
        T.s[rows:] = T.s[rows - 16:rows - 16 + T.n - rows]                            # (the last table tile's bytes again)
    T.nan_cols = {T.n - 1: (0xFF if kind == "nv" else 255, T.nb - 2)}
    if kind == "nv":
        T.nan_cols[T.n - 2] = (0x7F, 1)
    for col, (byte, blk) in T.nan_cols.items():
        T.s[col, blk] = byte
    code = ((np.arange(T.n)[:, None] + np.arange(k)[None, :]) % 16).astype(np.uint8)
    sval = np.repeat(scale_value(kind, T.s), T.group, axis=1)
    with np.errstate(invalid="ignore"):
        w = FP4[code] * sval
        T.zeroed = (w != 0) & ((np.abs(w) < LO) | (np.abs(w) >= 2.0 ** 128))           # weights that are no normal finite fp32 value
    code[T.zeroed] &= 8
    T.code, T.sval = code, sval
    with np.errstate(invalid="ignore"):
        T.w = FP4[code] * sval
    T.q = (code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8)
    return T


def required_pairs(kind):
    """(code, scale byte) the series of every M must read: every byte of the table x 16 codes, less the pairs whose weight is no normal fp32."""
    byts = list(range(0, 127)) + list(range(0x80, 0xFF)) if kind == "nv" else list(range(0, 255))
    out = set()
    for b in byts:
        s = float(scale_value(kind, b))
        for c in range(16):
            wv = abs(FP4[c] * s)
            if wv == 0 or LO <= wv < 2.0 ** 128:
                out.add((c, b))
    return out


def kappa(T, i):
    """Column of the non-zero activation of global row i (set * M + row): type i mod types -> (class, which of the per_block columns), the
    instance i // types walks the blocks of the class, so that the columns fall in every 256-k span, all eight nibble slots of a word and both
    halves of a 32-block."""
    t, v = i % T.types, i // T.types
    c, u = t % T.classes, t // T.classes
    blocks = np.arange(c, T.nb, T.classes)
    b = int(blocks[(v + c) % len(blocks)])
    off = (c + 8 * u) % 16 if T.per_block == 2 else (c + 3 * v) % 16
    if T.group == 32:
        off += 16 * ((c + v) % 2)
    return b * T.group + off


GS_KINDS = ("pow2", "negfull", "tiny")
GS_VALUES = {
    "pow2": [8.0, 2.0 ** -30, 2.0 ** 30, 1.0, 2.0 ** 60, 2.0 ** -90, 2.0 ** 90],
    "negfull": [-(2.0 - 2.0 ** -23) * 2.0 ** e for e in (0, -20, 20, -1, -70, 70)],
    "tiny": [float(np.float32(4.0 / 3.0)) * 2.0 ** -60],
}


def bf16_ends():
    top = next(b for b in range(0x7F7F, 0, -1) if 6.0 * values16(np.array([b], dtype=np.uint16), True)[0] < HI)
    return top, 9 << 7                                                                # largest a with 6 a < 2^127; 2^-118


def activation_classes(is_bf16, native):
    """name -> bits of |a|, or None where the exponent is chosen per column ("full": every mantissa bit set; native: 1 x and 1.5 x 2^t)."""
    if native:
        return {"1": None, "1.5": None}
    if is_bf16:
        top, bottom = bf16_ends()
        return {"largest": top, "smallest": bottom, "full": None}
    return {"largest": 0x7BFF, "smallest normal": 0x0400, "full": None, "largest subnormal": 0x03FF, "smallest subnormal": 0x0001}


def free_exponent(name, is_bf16, amin, amax):
    """bits of mant x 2^e, e in the middle of what [amin, amax) and the type's normal range leave, or None."""
    mant = {"full": 2.0 - 2.0 ** (-7 if is_bf16 else -10), "1": 1.0, "1.5": 1.5}[name]
    emin, emax = (-126, 127) if is_bf16 else (-14, 15)
    if name != "full":
        emin = max(emin, -119)                                                        # (the quantisers' e8m0 scale 2^(E - 7) stays a byte >= 1)
    lo = max(emin, math.ceil(math.log2(amin / mant)) - 1)
    while mant * 2.0 ** lo < amin:
        lo += 1
    hi = min(emax, math.floor(math.log2(amax / mant)) + 1)
    while mant * 2.0 ** hi >= amax:
        hi -= 1
    if lo > hi:
        return None
    v = np.array([mant * 2.0 ** ((lo + hi) // 2)])
    return int((O.f32_to_bf16_bits(v.astype(np.float32)) if is_bf16 else v.astype(np.float16).view(np.uint16))[0])


def two_sum_odd(p, b):
    """float64 p + b rounded to odd: s = fl(p + b) and the exact error e (Knuth); where e != 0 the exact sum lies strictly between s and its
    neighbour towards e, and of the two the one with the odd last bit is taken.  RNE of the result to float32 is RNE of the exact sum."""
    s = p + b
    bb = s - p
    e = (p - (s - bb)) + (b - bb)
    towards = np.nextafter(s, np.where(e > 0, np.inf, -np.inf))
    even = (s.view(np.int64) & 1) == 0
    return np.where((e != 0) & even, towards, s), e


class Fp32SubnormalSum(Exception):
    pass


def table_expect(P, is_bf16, subnormal_scales_zero=False, ignore_scale_sign=False, flush_fp16_subnormal=False, gs16=False, saturate=False):
    """-> (bits u16 [m, n], must_be_nan, is_zero) of a leg-1 problem by the contract; the keyword arguments are the mutants of the teeth test
    (under a mutant the generator's conditions are not asserted: they are the contract's)."""
    T, m = P.T, P.a_bits.shape[0]
    check = not (subnormal_scales_zero or ignore_scale_sign or flush_fp16_subnormal or gs16 or saturate)
    a = values16(P.a_bits[np.arange(m), P.kappa], is_bf16)
    w = T.w[:, P.kappa].T.copy()                                                      # [m, n]
    if subnormal_scales_zero or ignore_scale_sign:
        assert T.kind == "nv"
        sb = T.s[:, P.kappa // T.group].T
        if subnormal_scales_zero:
            w = np.where((sb & 0x78) == 0, 0.0, w)
        if ignore_scale_sign:
            w = np.where(sb >= 0x80, -w, w)
    if flush_fp16_subnormal:
        a = np.where(np.abs(a) < 2.0 ** -14, 0.0, a)
    gs = P.gs
    if gs16:
        g = np.array([gs], dtype=np.float32)
        gs = float(values16(O.f32_to_bf16_bits(g) if is_bf16 else g.astype(np.float16).view(np.uint16), is_bf16)[0])
    with np.errstate(invalid="ignore", over="ignore"):
        prod = a[:, None] * w
        prod[:, list(T.nan_cols)] = np.nan                                            # (the NaN scale of that column times any row's zeros)
        fin = np.isfinite(prod)
        frac = np.ldexp(np.frexp(np.where(fin, prod, 0.0))[0], 17)
        assert np.array_equal(frac, np.rint(frac)), "a w has at most 17 significant bits"
        assert float(np.float32(gs)) == gs
        y = prod * gs                                                                 # 17 + 24 bits: exact in float64
        nz = fin & (prod != 0)
        assert not check or ((np.abs(y[nz]) >= LO).all() and (np.abs(y[nz]) < HI).all())
        bias = np.zeros(T.n) if P.bias_bits is None else values16(P.bias_bits, is_bf16)
        total, _ = two_sum_odd(y, np.broadcast_to(bias[None, :], y.shape).copy())
        y32 = total.astype(np.float32)
        must_nan = np.isnan(y32)
        assert not check or np.array_equal(must_nan, ~fin)
        tiny = (y32 != 0) & (np.abs(y32) < LO)
        if check and tiny.any():                                                      # (a cancellation against the bias: the generator drops that bias)
            raise Fp32SubnormalSum(np.flatnonzero(tiny.any(axis=0)))
        if is_bf16:
            bits = O.f32_to_bf16_bits(np.where(must_nan, 0, y32))
        else:
            if saturate:
                y32 = np.clip(y32, -65504.0, 65504.0)
            bits = y32.astype(np.float16).view(np.uint16)
    bits = np.where(must_nan, np.uint16(INF_BITS[is_bf16] | 0x40), bits).astype(np.uint16)
    return bits, must_nan, (y32 == 0) & ~must_nan


class TableProblem:
    pass


@functools.lru_cache(maxsize=None)
def table_series(kind, is_bf16, m, k, native=False):
    """The leg-1 problems of (family, M, K): ceil(types / M) activation sets on the one W.  Each row's value is the least used of the classes
    (activation_classes x both signs) that the condition admits in its column; the set's gs is the first of the cycle's kind (then of the other
    kinds) under which every row has an admissible value; every second set has a bias."""
    T = table_layout(kind, k)
    classes = activation_classes(is_bf16, native)
    names = [(nm, sg) for nm in classes for sg in (0, 1)]
    used = dict.fromkeys(names, 0)
    series = []
    nsets = -(-T.types // m)
    seed = [kind == "mx", is_bf16, m, k, native]
    rng = np.random.default_rng(seed)
    for st in range(nsets):
        P = TableProblem()
        P.T, P.q, P.s, P.set = T, T.q, T.s, st
        P.kappa = np.array([kappa(T, st * m + r) for r in range(m)])
        first = (st + MS.index(m) if m in MS else st) + KS.index(k)
        order = [GS_KINDS[(first + j) % 3] for j in range(3)]
        best = None
        for rank, gs_kind in enumerate(order):                                        # the cycle's kind, unless another leaves fewer classes unused
            for gs in GS_VALUES[gs_kind]:
                chosen, trial = [], dict(used)
                for r in range(m):
                    col = T.w[:, P.kappa[r]]
                    cv = np.abs(FP4[T.code[:, P.kappa[r]]])
                    ok = np.isfinite(col) & (col != 0)
                    cv, wv = cv[ok], np.abs(col[ok])
                    x = np.concatenate([cv, cv * 2.0 ** -7, wv, wv * abs(gs)])
                    amin, amax = LO / x.min(), HI / x.max()
                    pick = None
                    # (least used first; among those the fixed values, which few columns admit, before the ones whose exponent is free)
                    for nm, sg in sorted(names, key=lambda c: (trial[c], classes[c[0]] is None, (names.index(c) + st * m + r) % len(names))):
                        bits = classes[nm] if classes[nm] is not None else free_exponent(nm, is_bf16, amin, amax)
                        if bits is not None and amin <= values16(np.array([bits], dtype=np.uint16), is_bf16)[0] < amax:
                            pick = (nm, sg, bits | (sg << 15))
                            break
                    if pick is None:
                        break
                    trial[(pick[0], pick[1])] += 1
                    chosen.append(pick)
                unused = (sum(v == 0 for v in trial.values()), rank)
                if len(chosen) == m and (best is None or unused < best[0]):
                    best = (unused, gs_kind, gs, chosen, trial)
        assert best is not None, f"no gs of the cycle admits an activation in every row: {kind} bf16={is_bf16} m={m} k={k} set {st}"
        _, P.gs_kind, gs, chosen, trial = best
        used, P.gs, P.classes = trial, gs, [(nm, sg) for nm, sg, _ in chosen]
        P.a_bits = np.zeros((m, k), dtype=np.uint16)
        P.a_bits[np.arange(m), P.kappa] = [b for _, _, b in chosen]
        P.bias_bits = None
        if st % 2 == (MS.index(m) if m in MS else 0) % 2:
            # next to the product of ONE row per column (row n mod m), either sign; the exponent kept inside the output type's normal range
            a = values16(P.a_bits[np.arange(m), P.kappa], is_bf16)
            own = np.arange(T.n) % m
            with np.errstate(invalid="ignore"):
                y0 = a[own] * T.w[np.arange(T.n), P.kappa[own]] * P.gs
            e0 = np.where(np.isfinite(y0) & (y0 != 0), np.frexp(np.where(np.isfinite(y0), y0, 1.0))[1] - 1, 0) + rng.integers(-2, 3, T.n)
            e0 = np.clip(e0, -100 if is_bf16 else -14, 100 if is_bf16 else 14)
            mant = 1.0 + rng.integers(0, 128 if is_bf16 else 1024, T.n) / (128.0 if is_bf16 else 1024.0)
            sign = np.where(e0 < -60, np.where(y0 < 0, -1.0, 1.0), rng.choice(np.array([-1.0, 1.0]), T.n))       # (tiny: no cancellation into subnormals)
            bv = (sign * mant * np.exp2(e0)).astype(np.float32)
            P.bias_bits = O.f32_to_bf16_bits(bv) if is_bf16 else bv.astype(np.float16).view(np.uint16)
        for _ in range(3):
            try:
                P.want, P.must_nan, P.is_zero = table_expect(P, is_bf16)
                break
            except Fp32SubnormalSum as exc:                                           # fp32 subnormals are no part of the contract
                P.bias_bits[exc.args[0]] = 0
        assert not (P.want[~P.must_nan] == POISON[is_bf16]).any()
        series.append(P)
    return series


def pairs_read(series):
    out = set()
    for P in series:
        T = P.T
        for kp in P.kappa:
            ok = ~T.zeroed[:, kp] & ~np.isnan(T.w[:, kp])
            ok[list(T.nan_cols)] = False                                              # (those columns' outputs are NaN whatever is read)
            out |= set(zip(T.code[ok, kp].tolist(), T.s[ok, kp // T.group].tolist()))
    return out


@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_table_generator_coverage_and_preconditions(kind, is_bf16):
    """Once per (family, M, K), on A and W alone: the pairs (code, scale byte) the non-zero activations read are all of required_pairs, the NaN
    bytes sit once each, the columns fall in every 256-k span, all eight nibble slots and both halves of a 32-block, both signs of every
    activation class occur, the bytes mean what the oracle says (but e8m0 0 and 255, stated), and over the Ms of a (family, K) gs takes each of
    its three kinds and a bias is there in about half the sets."""
    need = required_pairs(kind)
    assert len(need) == (254 * 16 if kind == "nv" else 255 * 16 - 20), len(need)
    for k in KS:
        T = table_layout(kind, k)
        dq = (O.dequant_nvfp4(T.q, T.s) if kind == "nv" else O.dequant_mxfp4(T.q, T.s)).astype(np.float64)
        same = np.ones_like(T.w, dtype=bool)
        if kind == "mx":
            s_k = np.repeat(T.s, 32, axis=1)
            assert not dq[s_k == 0].any() and (np.abs(T.w[(s_k == 0) & ((T.code & 7) >= 4)]) >= LO).all()        # byte 0: the oracle 0, here c 2^-127
            with np.errstate(invalid="ignore"):
                assert not np.isfinite(dq[s_k == 255]).any()                                                 # byte 255: the oracle c x inf
            same = (s_k != 0) & (s_k != 255)
        assert np.array_equal(dq[same], T.w[same], equal_nan=True), (kind, k)
        for byte in (0x7F, 0xFF) if kind == "nv" else (255,):
            assert (T.s == byte).sum() == 1
        gs_kinds, with_bias, sets = set(), 0, 0
        for m in MS:
            series = table_series(kind, is_bf16, m, k)
            tag = f"{kind} bf16={is_bf16} m={m} k={k}"
            assert pairs_read(series) >= need, (tag, sorted(need - pairs_read(series))[:8])
            kp = np.concatenate([P.kappa for P in series])
            assert set(kp // 256) == set(range(k // 256)), tag
            assert set(kp % 8) == set(range(8)) and set(kp // 16 % 2) == {0, 1}, tag
            seen = {c for P in series for c in P.classes}
            assert seen == {(nm, sg) for nm in activation_classes(is_bf16, False) for sg in (0, 1)}, (tag, seen)
            for P in series:
                assert (P.a_bits != 0).sum(axis=1).tolist() == [1] * m, tag
                gs_kinds.add(P.gs_kind)
                with_bias, sets = with_bias + (P.bias_bits is not None), sets + 1
        assert gs_kinds == set(GS_KINDS), (kind, is_bf16, k, gs_kinds)
        assert 0.3 <= with_bias / sets <= 0.7, (kind, is_bf16, k, with_bias, sets)


@pytest.mark.parametrize("is_bf16", [True, False])
def test_native_table_activations_are_exact_under_the_quantisers(is_bf16):
    """The native class's series: a_r = +-2^t {1, 1.5} on a one-hot block is reproduced by all three activation quantisers, with t such that
    their block scale stays an e8m0 byte."""
    from test_gpu_parity import quantize_act_mxfp4, quantize_act_mxfp6, quantize_act_mxfp8
    for m in NATIVE_MS:
        for P in table_series("mx", is_bf16, m, NATIVE_K, True):
            a = values16(P.a_bits, is_bf16)
            e = np.frexp(a[a != 0])[1] - 1
            assert e.min() - 7 + 127 >= 1 and e.max() - 2 + 127 <= 254
            for quant in (quantize_act_mxfp8, quantize_act_mxfp6, quantize_act_mxfp4):
                assert np.array_equal(quant(a.astype(np.float32)).astype(np.float64), a), (m, quant.__name__)


@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_table_teeth(kind, is_bf16):
    """Each wrong reading the contract excludes changes expected bits in every (family, K) it can occur in (the e4m3 mutants on NVFP4, the fp16
    mutants on fp16): a kernel that had it could not pass."""
    mutants = ["gs16"] + (["subnormal_scales_zero", "ignore_scale_sign"] if kind == "nv" else []) + ([] if is_bf16 else ["flush_fp16_subnormal", "saturate"])
    for k in KS:
        changed = dict.fromkeys(mutants, 0)
        for m in MS:
            for P in table_series(kind, is_bf16, m, k):
                for name in mutants:
                    bits, nan, zero = table_expect(P, is_bf16, **{name: True})
                    differs = (bits != P.want) & ~(zero & P.is_zero) | (nan != P.must_nan)
                    changed[name] += int(differs.sum())
        assert all(changed.values()), (kind, is_bf16, k, changed)


# --- the device side -------------------------------------------------------------------------------------------------------------------------

class ValueDevice(Device):
    """Device judged by P.want where P.must_nan / P.is_zero (optional) do not say otherwise: an output that must be NaN is any NaN but the poison,
    an expected zero is a zero of either sign."""

    def __init__(self, pk, kind, is_bf16, m, n, k, P, activation=0):
        super().__init__(pk, kind, is_bf16, m, n, k, P, activation)
        mask = lambda name: torch.from_numpy(np.ascontiguousarray(getattr(P, name, np.zeros(P.want.shape, dtype=bool)))).to(DEV).reshape(-1)
        self.must_nan, self.is_zero = mask("must_nan"), mask("is_zero")

    def wrong(self):
        got = self.c_out.to(torch.int32) & 0xFFFF
        mag = got & 0x7FFF
        ok = torch.where(self.must_nan, (mag > INF_BITS[self.is_bf16]) & (got != self.poison), self.c_out == self.want)
        return ~(ok | (self.is_zero & (mag == 0)))

    def compare(self) -> list:
        bad = self.wrong()
        if not bool(bad.any()):
            return []
        got = self.c_out.cpu().numpy().view(np.uint16)
        idx = np.flatnonzero(bad.cpu().numpy())
        r, c = divmod(int(idx[0]), self.n_out)
        a_row = self.P.a_bits[r]
        nzc = np.flatnonzero(a_row)[:2]
        extra = f"; row {r} has a = " + ", ".join(f"{a_row[j]:#06x} at k {j}" for j in nzc)
        if hasattr(self.P, "T"):
            T = self.P.T
            extra += f", code {T.code[c, nzc[0]]} scale byte {T.s[c, nzc[0] // T.group]:#04x}, gs {self.P.gs!r}, must be NaN: {bool(self.P.must_nan[r, c])}"
        return [self.describe(got, idx) + extra]


def count_and_assert(tag, counts, failures, k, kinds_of=None):
    print(f"value_contract {tag}: { {key: (sorted(v) if isinstance(v, set) else v) for key, v in counts.items()} }")
    assert k < 1280 or counts["split"] > counts.get("collapsed", 0), "no K-split id ran"
    if kinds_of is not None:
        assert counts["kinds"] >= kinds_of, ("a kind nibble of the enumeration did not run", sorted(kinds_of - counts["kinds"]))
    assert not failures, f"{len(failures)} of {counts['launched']} launches wrong:\n" + "\n".join(failures[:20])


def enumerated_kinds(pk, kind, is_bf16, m, n, k):
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = torch.bfloat16 if is_bf16 else torch.float16
    h.b_type = pk.DataType.float4_e2m1 if kind == "nv" else pk.DataType.mxfloat4_e2m1
    return {(sid >> 48) & 0xF for sid in pk.ops.get_fp4_solutions(h, m, n, k)}


def test_m_list_names_every_kind():
    """The kind nibbles get_fp4_solutions names over MS equal those it names over every M in 1..512, per family and K (no GPU: the enumeration
    is a host query)."""
    import petit_kernel as pk_
    for kind, is_bf16 in FAMILIES:
        for k in sorted(set(KS) | set(SWITCH_KS)):
            every = set().union(*(enumerated_kinds(pk_, kind, is_bf16, m, TABLE_N[kind], k) for m in range(1, 513)))
            ours = set().union(*(enumerated_kinds(pk_, kind, is_bf16, m, TABLE_N[kind], k) for m in MS))
            assert ours == every, (kind, is_bf16, k, sorted(every - ours))


@pytest.mark.gpu
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_truth_tables_every_id_bit_for_bit(pk, kind, is_bf16, k, m):
    """Leg 1: every enumerated kernel, the default pick and every accepted K split on every activation set of the series."""
    counts = {"launched": 0, "split": 0, "refused": 0, "sets": 0}
    failures = []
    for P in table_series(kind, is_bf16, m, k):
        counts["sets"] += 1
        failures += [f"set {P.set}: {f}" for f in run_ids(pk, kind, is_bf16, m, TABLE_N[kind], k, "T", exact_ids, counts, P=P, device=ValueDevice)]
    count_and_assert(f"tables {kind} bf16={is_bf16} k={k} m={m}", counts, failures, k)


NATIVE_MS, NATIVE_K = (1, 33, 257), 2048


@pytest.mark.gpu
@pytest.mark.parametrize("m", NATIVE_MS)
@pytest.mark.parametrize("is_bf16", [True, False])
def test_truth_tables_native_class_mxfp4(pk, is_bf16, m):
    """Leg 1 on the block-scaled-MFMA kernels (kinds 9 and 13, MXFP8 / MXFP6 / MXFP4 activations, K split 1 and 2): the same table under
    activations the three quantisers reproduce."""
    counts = {"launched": 0, "split": 0, "refused": 0, "sets": 0}
    failures = []
    pk.ops.enable_native_fp4(True)
    try:
        for P in table_series("mx", is_bf16, m, NATIVE_K, True):
            counts["sets"] += 1
            failures += [f"set {P.set}: {f}" for f in run_ids(pk, "mx", is_bf16, m, 288, NATIVE_K, "T", native_ids, counts, P=P, device=ValueDevice)]
    finally:
        pk.ops.enable_native_fp4(False)
    count_and_assert(f"tables native mx bf16={is_bf16} m={m}", counts, failures, NATIVE_K)


# --- leg 2: the fp16 x MXFP4 fallback and switch, and far e8m0 ---------------------------------------------------------------------------------

SWITCH_KS = (1280, 2048, 5120)
SHIFTS = {True: (100, -100), False: (-26,)}


def shifted_and_switched(is_bf16, m, n, k, regime="B"):
    """[(name, Problem)] of leg 2: regime F for both types, regime S (both placements) for fp16."""
    out = [(f"F{d:+d}", exact_problem("mx", is_bf16, m, n, k, regime, 0, mx_shift=d)) for d in SHIFTS[is_bf16]]
    if not is_bf16:
        out += [(f"S-{v}", exact_problem("mx", False, m, n, k, regime, 0, switch=v)) for v in ("mid", "last")]
    return out


@pytest.mark.parametrize("is_bf16", [True, False])
def test_shifted_and_switched_preconditions(is_bf16):
    """Regime F: every weight is regime B's times 2^d and gs is regime B's times 2^-d, so acc 2^d is exact wherever acc was (one power of two, no
    partial sum leaves the normal range: the quantum 2^d / 4 stays above 2^-126 and sum |a||w| 2^d below 2^127) and `want` is regime B's.  fp16,
    d = -26: every byte is in 100..103, outside 114..140.  Regime S: B's bytes, every changed block dequantises to zeros under a byte outside
    114..140, the other blocks are B's, and `want` is the exact sum without those blocks."""
    for k in SWITCH_KS:
        for m in (1, 40):
            B = exact_problem("mx", is_bf16, m, 288, k, "B", 0)
            for name, P in shifted_and_switched(is_bf16, m, 288, k):
                dq = O.dequant_mxfp4(P.q, P.s).astype(np.float64)
                assert np.array_equal(P.a_bits, B.a_bits) and np.array_equal(P.bias_bits, B.bias_bits), name
                if name[0] == "F":
                    d = P.mx_shift
                    assert np.array_equal(dq, B.w * 2.0 ** d) and P.gs == B.gs * 2.0 ** -d and np.array_equal(P.want, B.want), name
                    assert float(np.float32(P.gs)) == P.gs and 2.0 ** d / 4 >= LO * 2.0 ** 24 and (np.abs(B.a) @ np.abs(B.w).T).max() * 2.0 ** d < HI
                    assert is_bf16 or (100 <= P.s.min() and P.s.max() <= 103)
                else:
                    assert np.array_equal(dq, P.w) and P.switched and P.gs == B.gs, name
                    changed = np.zeros_like(P.s, dtype=bool)
                    for row, blk, byte, _ in P.switched:
                        changed[row, blk] = True
                        assert not dq[row, 32 * blk:32 * blk + 32].any() and P.s[row, blk] == byte and not 114 <= byte <= 140
                    assert np.array_equal(P.s[~changed], B.s[~changed]) and np.array_equal(P.w[~np.repeat(changed, 32, axis=1)], B.w[~np.repeat(changed, 32, axis=1)])
                    assert (changed.reshape(18, 16, -1).any(axis=(1, 2))[0::2]).all(), "every even 16-row tile switches"
                    if name == "S-last":
                        assert changed[:, :-8].sum() == 0
                    else:
                        assert changed[5, 0]
                    assert not np.array_equal(P.want, B.want)


@pytest.mark.gpu
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("k", SWITCH_KS)
@pytest.mark.parametrize("is_bf16", [True, False])
def test_shifted_and_switched_every_id_bit_for_bit(pk, is_bf16, k, m):
    """Leg 2: regimes F and S through every id and accepted K split, zero tolerance; at least one id of every enumerated kind nibble ran."""
    counts = {"launched": 0, "split": 0, "refused": 0, "kinds": set()}
    failures = []
    for name, P in shifted_and_switched(is_bf16, m, 288, k):
        failures += run_ids(pk, "mx", is_bf16, m, 288, k, name, exact_ids, counts, P=P, device=ValueDevice)
    count_and_assert(f"shifted/switched mx bf16={is_bf16} k={k} m={m}", counts, failures, k, enumerated_kinds(pk, "mx", is_bf16, m, 288, k))


@pytest.mark.gpu
@pytest.mark.parametrize("m", (4, 40, 129))
def test_shifted_and_switched_gated_silu_mul(pk, m):
    """Leg 2 through test_gated_contract's machinery: SiLU-mul on fp16 x MXFP4 at K = 2048, regimes F and S, its band and cap unchanged."""
    from test_gated_contract import CAP, GatedDevice, check_preconditions, gated_problem
    k, counts, failures = 2048, {"launched": 0, "split": 0, "collapsed": 0, "refused": 0, "kinds": set()}, []
    for n in (288, 544):
        for name, opts in (("F-26", {"mx_shift": -26}), ("S-mid", {"switch": "mid"}), ("S-last", {"switch": "last"})):
            P = gated_problem("mx", False, m, n, k, 1, **opts)
            check_preconditions(P, False, (name, m, n))
            assert P.undecided <= CAP[False]
            failures += run_ids(pk, "mx", False, m, n, k, name, exact_ids, counts, activation=1, P=P, device=GatedDevice)
    count_and_assert(f"shifted/switched gated mx fp16 k={k} m={m}", counts, failures, k)


# --- leg 3: non-finite activations ---------------------------------------------------------------------------------------------------------------

NONFINITE_KS, NONFINITE_MS = (1280, 2048), (1, 4, 8, 16, 40, 129, 257)
NAN_BITS = {True: 0x7F81, False: 0x7C01}         # a NaN of the low payload bits: not the poison, and not a NaN any more once truncated to 8 bits


def injections(is_bf16, m, k):
    """-> variants, each a list of (row, [(column, bits)]): +inf in row 0 (span 0), -inf in the last row (last 256 k), a NaN in row 1, two +inf
    in row 2; where M has fewer rows, the injections that would share a row go to variants of their own."""
    pinf, ninf = INF_BITS[is_bf16], INF_BITS[is_bf16] | 0x8000
    wanted = [(0, [(100, pinf)]), (m - 1, [(k - 256 + 7, ninf)]), (min(1, m - 1), [(3 * 256 + 9, NAN_BITS[is_bf16])]), (min(2, m - 1), [(300, pinf), (333, pinf)])]
    variants = []
    for row, what in wanted:
        for v in variants:
            if row not in [r for r, _ in v]:
                v.append((row, what))
                break
        else:
            variants.append([(row, what)])
    return variants


def nonfinite_problem(base, is_bf16, variant, lo_is_nan_in_fallback=False):
    """base (an exact_problem) with the variant's injections: a_bits, want, must_nan.  The class of an output of an injected row from its terms
    a_k w_k alone: NaN if a term is NaN (inf x 0, NaN x anything) or both infinities occur, else the infinity that occurs -- times gs > 0, plus
    a finite bias.  lo_is_nan_in_fallback: the model of split_f16 before its fix (hi = inf, lo = inf - inf) where every wave is in the fallback
    body -- any non-finite fp16 activation makes its whole row NaN."""
    P = type(base)()
    P.__dict__.update(base.__dict__)
    P.a_bits, P.want = base.a_bits.copy(), base.want.copy()
    P.must_nan = np.zeros(P.want.shape, dtype=bool)
    assert P.gs > 0
    for row, what in variant:
        cols = [c for c, _ in what]
        vals = values16(np.array([b for _, b in what], dtype=np.uint16), is_bf16)
        P.a_bits[row, cols] = [b for _, b in what]
        with np.errstate(invalid="ignore"):
            terms = P.w[:, cols] * vals[None, :]                                      # [n, injections]
        nan = np.isnan(terms).any(axis=1) | ((terms == np.inf).any(axis=1) & (terms == -np.inf).any(axis=1))
        if lo_is_nan_in_fallback:
            nan[:] = True
        assert np.isinf(terms[~nan]).any(axis=1).all()
        P.must_nan[row] = nan
        P.want[row] = np.where((terms == -np.inf).any(axis=1), INF_BITS[is_bf16] | 0x8000, INF_BITS[is_bf16])
    P.injected = sorted(r for r, _ in variant)
    return P


def nonfinite_bases(kind, is_bf16, m, k):
    n = TABLE_N[kind]
    out = [("B", exact_problem(kind, is_bf16, m, n, k, "B", 0))]
    if kind == "mx" and not is_bf16:
        out += shifted_and_switched(False, m, n, k)
    return out


@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_nonfinite_generator_preconditions(kind, is_bf16):
    """The +inf of row 0 meets zero and non-zero weight codes, the two +inf of one row meet weights of opposite signs in some columns and of equal
    signs in others, every injection is used at every M, the NaN is not the poison; and the model of split_f16 before its fix (lo = NaN) changes
    expected classes on fp16 x MXFP4 regime F and on no regime B problem (no wave of regime B is in the fallback body: its bytes are 126..129)."""
    assert NAN_BITS[is_bf16] != POISON[is_bf16] and np.isnan(values16(np.array([NAN_BITS[is_bf16]], dtype=np.uint16), is_bf16)[0])
    for k in NONFINITE_KS:
        for m in NONFINITE_MS:
            variants = injections(is_bf16, m, k)
            assert sum(len(v) for v in variants) == 4 and all(len({r for r, _ in v}) == len(v) for v in variants)
            for name, base in nonfinite_bases(kind, is_bf16, m, k):
                w = base.w
                assert (w[:, 100] == 0).any() and (w[:, 100] != 0).any(), name
                assert (w[:, 300] * w[:, 333] < 0).any() and (w[:, 300] * w[:, 333] > 0).any(), name
                kinds_seen = set()
                for v in variants:
                    P = nonfinite_problem(base, is_bf16, v)
                    rows = np.array(P.injected)
                    kinds_seen |= {"nan"} if P.must_nan[rows].any() else set()
                    kinds_seen |= {"+inf"} if (P.want[rows][~P.must_nan[rows]] == INF_BITS[is_bf16]).any() else set()
                    kinds_seen |= {"-inf"} if (P.want[rows][~P.must_nan[rows]] == INF_BITS[is_bf16] | 0x8000).any() else set()
                    others = np.setdiff1d(np.arange(m), rows)
                    assert np.array_equal(P.want[others], base.want[others]) and not P.must_nan[others].any()
                    mutant = nonfinite_problem(base, is_bf16, v, lo_is_nan_in_fallback=name.startswith("F"))
                    differs = not np.array_equal(mutant.must_nan, P.must_nan)
                    has_inf = any(not np.isnan(values16(np.array([b], dtype=np.uint16), is_bf16)[0]) for _, what in v for _, b in what)
                    assert differs == (name.startswith("F") and not is_bf16 and has_inf), (name, m, k)
                assert kinds_seen == {"nan", "+inf", "-inf"}, (name, kinds_seen)


@pytest.mark.gpu
@pytest.mark.parametrize("m", NONFINITE_MS)
@pytest.mark.parametrize("k", NONFINITE_KS)
@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_nonfinite_activations_every_id(pk, kind, is_bf16, k, m):
    """Leg 3: rows without an injection keep their exact bits, injected rows the class and sign of every output, nothing left unwritten."""
    counts = {"launched": 0, "split": 0, "refused": 0, "kinds": set()}
    failures = []
    for name, base in nonfinite_bases(kind, is_bf16, m, k):
        for i, v in enumerate(injections(is_bf16, m, k)):
            P = nonfinite_problem(base, is_bf16, v)
            failures += run_ids(pk, kind, is_bf16, m, TABLE_N[kind], k, f"{name} variant {i}", exact_ids, counts, P=P, device=ValueDevice)
    count_and_assert(f"nonfinite {kind} bf16={is_bf16} k={k} m={m}", counts, failures, k, enumerated_kinds(pk, kind, is_bf16, m, TABLE_N[kind], k))


@pytest.mark.gpu
@pytest.mark.parametrize("m", (33, 257))
@pytest.mark.parametrize("is_bf16", [True, False])
def test_nonfinite_activations_native_class_clean_rows(pk, is_bf16, m):
    """The native class: the rows without an injection keep their exact bits (what the quantisers make of a block that holds +-inf or NaN is
    described in profiles/value_contract.md and not pinned)."""
    k, n = 2048, 288
    base = exact_problem("mx", is_bf16, m, n, k, "B", 0)
    P = nonfinite_problem(base, is_bf16, injections(is_bf16, m, k)[0])
    P.must_nan[:] = False
    P.clean = np.setdiff1d(np.arange(m), P.injected)

    class CleanRows(ValueDevice):
        def wrong(self):
            bad = super().wrong().reshape(self.m, self.n_out)
            bad[torch.as_tensor(self.P.injected, device=DEV)] = False
            return bad.reshape(-1)

    counts = {"launched": 0, "split": 0, "refused": 0}
    pk.ops.enable_native_fp4(True)
    try:
        failures = run_ids(pk, "mx", is_bf16, m, n, k, "B", native_ids, counts, P=P, device=CleanRows)
    finally:
        pk.ops.enable_native_fp4(False)
    count_and_assert(f"nonfinite native mx bf16={is_bf16} m={m}", counts, failures, k)

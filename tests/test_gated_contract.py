"""The gated GEMM epilogues (petit_epilogue.activation 1 SiLU-mul, 2 SwiGLU-OAI) of the dense kernels, bit for bit: the method of
test_exact_contract.py (inputs on which acc is ONE number in any order, caller-owned poisoned and guarded buffers, every id and K split) carried to
c[m][j] = round16(act(y[m][j], y[m][j + n/2])), y = fma(acc, gs, bias).

Inputs, regime "G" of exact_problem: B's weights, block scales and activations (every product and partial sum exact in fp32), gs = 3 * 2^-s with s
from G_SHIFT and a bias of multiples of 2^-4 in [-2, 2] per column.  y is then a multiple of 3 * 2^-(s + 2) below 64: exact in fp32, and so is
clamp(y_up) + 1.  Three conditions pull against each other: each clamp of SwiGLU-OAI must be reached by 1 % of the values (a wide y), in fp16
SwiGLU-OAI's output is SUBNORMAL for every gate below about -7.5 (g sigmoid(1.702 g) < 2^-14 / |u + 1|), which counts as undecided against the 4 %
cap (a narrow y, or a gate that leans positive), and the standard deviation of acc is 1.27 times larger with MXFP4's block scales (.5 .. 4) than
with NVFP4's (.5 .. 3) while s moves it in steps of 2.  So the gate half's bias lies in [1, 2] (the negative tail shrinks, the positive one
grows), the up half's has magnitude in [1.5, 2] with either sign (both of its tails grow), and s is one number per K except at K = 2048, where
sqrt(K) falls half a step between its neighbours and no single s serves both families: s = 8 leaves MXFP4 / fp16 / SwiGLU-OAI at 6 % undecided,
s = 9 leaves NVFP4's up half at 0.3 % beyond either clamp.  |y_gate| <= 40 everywhere.

Expected value: float64, the header's statement (silu_mul / swiglu_oai below, alpha = float32(1.702)), rounded once.  The only slack is the distance
of the device's fp32 arithmetic from the float64 value.  The generated code of silu_mul4 (device_common.hpp; gfx950, -O3, no fast-math) is, per
output, with x = alpha * g * log2(e):
    v_mul_f32 t = alpha * -g           one rounding (none for SiLU-mul: alpha = 1)        |error of t * log2 e| <= |x| 2^-24
    v_mul_f32 t' = 0x3fb8aa3b * t      one rounding, and the constant is log2 e (1 - 2^-26.2)               <= |x| (2^-24 + 2^-26)
    v_exp_f32 e = 2^t'                 1 ulp (the ISA manual's statement, taken on trust: not measured here) relative 2^-23
    v_add_f32 d = 1 + e                one rounding                                                         relative 2^-24
    v_div_scale / v_rcp / v_fma ... v_div_fmas / v_div_fixup: the IEEE division g / d, correctly rounded    relative 2^-24
    v_mul_f32 (g / d) * u              one rounding                                                         relative 2^-24
An absolute error eps of the exponent enters e as the relative error 2^eps - 1 <= 0.7 eps, and e enters d with weight e / (1 + e) <= 1, so the
result is within 2^-23 (2.5 + 0.8 |x|) of the float64 value, relatively.  The band used is delta = 2^-23 (8 + 2 |x|): three times that, nothing
fitted.  An output whose whole band ref (1 +- delta) rounds to one 16-bit value must be that value; otherwise ("undecided") it may be either of the
two neighbours the band reaches and nothing else.  A reference below the smallest normal of the output type (fp16: gates below about -8 / -13) is
compared at one quantum of the subnormal range, absolutely, and counts as undecided.  Undecided outputs are capped per problem (CAP): 4 % fp16, 1 %
bf16; the generator takes the first seed that keeps a problem within the cap (tiny problems: one undecided output of 16 is 6 %).
Independently of the band every launch of a problem (every id, every K split) must give the bits of the problem's first launch.

The quantising form (out_format 8 / 6 / 4) takes the same float64 reference through the numpy quantisers of test_gpu_parity.py: the scale byte of a
32-column block is the rule on the reference's block maximum unless the band around that maximum crosses a power of two (such blocks are left out,
at most 2 %), and an element's code is the quantiser's code of the reference, or of either end of its band where they differ.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_exact_contract import DEV, FAMILIES, GUARD, POISON, Device, exact_ids, exact_problem, native_ids, pk, round16, run_ids  # noqa: F401

G_SHIFT = {256: (7, 7), 1280: (8, 8), 2048: (8, 9), 5120: (9, 9)}    # K -> s for (NVFP4, MXFP4) weights, gs = 3 * 2^-s; why 2048 has two: docstring
KS = tuple(G_SHIFT)
MS = (1, 4, 5, 16, 17, 40, 129, 257)
NS = (32, 288, 544)                              # n / 2 = 16 (one tile per half), 144 (nine tiles), 272
ACTS = (1, 2)
ALPHA = float(np.float32(1.702))
LIMIT = 7.0
LOG2E = 1.4426950408889634
CAP = {True: 0.01, False: 0.04}                  # undecided outputs per problem, bf16 / fp16
SMALLEST_NORMAL = {True: 2.0 ** -126, False: 2.0 ** -14}
QUANTUM = {True: 2.0 ** -133, False: 2.0 ** -24}
SEEDS_TRIED = 8


# --- 1. the float64 model -------------------------------------------------------------------------------------------------------------------

def gated64(yg, yu, act, alpha=ALPHA, lower_clamp=True, gate_lower_clamp=False, one_first=False, round_silu=None):
    """The header's statement in float64; the keyword arguments are the mutants of the teeth test (none of them touches SiLU-mul, act 1)."""
    if act == 1:
        g, u, a = yg, yu, 1.0
    else:
        g = np.minimum(yg, LIMIT)
        if gate_lower_clamp:
            g = np.maximum(g, -LIMIT)
        u = np.clip(yu + 1.0, -LIMIT if lower_clamp else -np.inf, LIMIT) if one_first else np.clip(yu, -LIMIT if lower_clamp else -np.inf, LIMIT) + 1.0
        a = alpha
    silu = g / (1.0 + np.exp(-a * g))
    if round_silu is not None:
        silu = round16(silu, round_silu)
    return silu * u


def band(yg, act):
    g, a = (yg, 1.0) if act == 1 else (np.minimum(yg, LIMIT), ALPHA)
    return 2.0 ** -23 * (8.0 + 2.0 * np.abs(a * g * LOG2E))


def bits16(v, is_bf16):
    """to_bits for values of the output type that may be subnormal or zero (to_bits asserts the normal range's round trip only for fp16 values)."""
    if is_bf16:
        return (v.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    return v.astype(np.float16).view(np.uint16)


def values16(b, is_bf16):
    with np.errstate(invalid="ignore"):
        return ((b.astype(np.uint32) << 16).view(np.float32) if is_bf16 else b.view(np.float16)).astype(np.float64)


def expect(P, is_bf16, act):
    """Adds to a regime-G problem what the gated epilogue `act` must write: ref (float64 [m, n/2]), delta, want / alt (u16: the nearest value and,
    where the band reaches a second one, that; else want again), decided, subnormal, and wrong(got bits) -> mask of outputs outside what is accepted."""
    nh = P.y.shape[1] // 2
    yg, yu = P.y[:, :nh], P.y[:, nh:]
    P.act, P.ref, P.delta = act, gated64(yg, yu, act), band(yg, act)
    P.subnormal = np.abs(P.ref) < SMALLEST_NORMAL[is_bf16]
    safe = np.where(P.subnormal, 1.0, P.ref)
    lo, mid, hi = (round16(safe * f, is_bf16) for f in (1.0 - P.delta, 1.0, 1.0 + P.delta))
    P.decided = (lo == hi) & ~P.subnormal
    q = QUANTUM[is_bf16]
    mid = np.where(P.subnormal, np.rint(P.ref / q) * q, mid)
    other = np.where(P.subnormal | P.decided, mid, np.where(mid == lo, hi, lo))
    P.want, P.alt = bits16(mid, is_bf16), bits16(other, is_bf16)
    P.undecided = float((~P.decided).mean())

    def wrong(got):
        got = got.reshape(P.want.shape)
        ok = (got == P.want) | (got == P.alt)
        with np.errstate(invalid="ignore"):
            ok |= P.subnormal & (np.abs(values16(got, is_bf16) - P.ref) <= q)       # (a NaN, the poison included, compares false)
        return ~ok.reshape(-1)
    P.wrong = wrong
    return P


@functools.lru_cache(maxsize=4)
def inputs(kind, is_bf16, m, n, k, seed, mx_shift=0, switch=None):
    return exact_problem(kind, is_bf16, m, n, k, "G", seed, shift=G_SHIFT[k][kind == "mx"], mx_shift=mx_shift, switch=switch)


def gated_problem(kind, is_bf16, m, n, k, act, first_seed=0, mx_shift=0, switch=None):
    """The problem of a GPU case: regime G at the first seed whose undecided share is within the cap (the inputs are shared by both activations).
    mx_shift / switch: exact_problem's two options for test_value_contract.py, under the same cap and the same band."""
    for seed in range(first_seed, first_seed + SEEDS_TRIED):
        base = inputs(kind, is_bf16, m, n, k, seed, mx_shift, switch)
        P = type(base)()
        P.__dict__.update(base.__dict__)
        P.seed = seed
        if expect(P, is_bf16, act).undecided <= CAP[is_bf16]:
            return P
    raise AssertionError(f"no seed in {first_seed}..{seed} keeps {kind} bf16={is_bf16} m={m} n={n} k={k} act={act} within the cap")


# --- 2. CPU: the preconditions, the cap, the teeth -----------------------------------------------------------------------------------------

EVAL_M, EVAL_N, SEEDS = 64, 288, tuple(range(SEEDS_TRIED))     # (every seed a GPU problem may end up at)


def check_preconditions(P, is_bf16, tag):
    """What holds for EVERY regime-G problem, the GPU cases' included."""
    n = P.y.shape[1]
    nh = n // 2
    yg, yu = P.y[:, :nh], P.y[:, nh:]
    assert np.array_equal(P.y.astype(np.float32).astype(np.float64), P.y), tag                        # y survives float32: the fma is exact
    assert np.array_equal((yu + 1.0).astype(np.float32).astype(np.float64), yu + 1.0), tag            # and so is u + 1
    assert (np.abs(P.a) @ np.abs(P.w).T).max() / P.quantum < 2 ** 24, tag                             # any partial sum, any order: exact
    assert np.abs(yg).max() <= 40.0, (tag, np.abs(yg).max())
    assert not np.array_equal(P.bias[:nh], P.bias[nh:]) or nh < 32, tag
    assert np.array_equal(np.rint(P.bias * 16), P.bias * 16) and np.abs(P.bias).max() <= 2.0 and np.unique(P.bias).size >= min(8, nh // 2), tag
    assert not np.any(P.want == POISON[is_bf16]) and not np.any(P.alt == POISON[is_bf16]), tag
    assert P.undecided <= CAP[is_bf16], (tag, P.undecided)
    # an undecided output's two accepted values are neighbours (the band is far narrower than a quantum of the type)
    und = ~P.decided & ~P.subnormal
    assert (np.abs(P.want[und].astype(np.int32) - P.alt[und].astype(np.int32)) == 1).all(), tag
    assert np.array_equal(P.want[P.decided], P.alt[P.decided]), tag


@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_generator_preconditions_and_teeth(kind, is_bf16):
    """Regime G keeps what makes acc one number, lands y where the activations curve and clamp, keeps the undecided share within the cap, and each
    wrong epilogue the contract excludes changes expected bits among the DECIDED outputs (so a kernel that had it could not pass).  Two named
    exceptions, both arithmetic: the four SwiGLU-OAI-only mutants are the identity on SiLU-mul, and in fp16 a lower clamp on the gate shows only on
    outputs that are normal fp16 values although their gate is below -7 (stated at the assertion).  The clamp shares and the curved range are
    properties of (family, K, s): shown here at the 64 x 288 shape for every seed a GPU problem may take, not per GPU problem."""
    from oracle import oracle as O
    from test_gpu_parity import quantize_act_mxfp4, quantize_act_mxfp6, quantize_act_mxfp8
    m, n, nh = EVAL_M, EVAL_N, EVAL_N // 2
    worst = 0.0
    for k in KS:
        for seed in SEEDS:
            base = inputs(kind, is_bf16, m, n, k, seed)
            tag = f"{kind} bf16={is_bf16} G K={k} seed={seed}"
            dq = O.dequant_nvfp4(base.q, base.s) if kind == "nv" else O.dequant_mxfp4(base.q, base.s)
            assert np.array_equal(dq.astype(np.float64), base.w), tag
            assert base.gs == 3.0 * 2.0 ** -G_SHIFT[k][kind == "mx"] and np.array_equal(base.y, base.acc * base.gs + base.bias[None, :]), tag
            assert np.array_equal(np.rint(base.a), base.a) and np.array_equal(np.rint(base.w / base.quantum), base.w / base.quantum), tag
            if kind == "mx":       # the native class: the preconditions of test_exact_contract.py, which depend on a and w alone
                def spread(x):
                    g = np.abs(x).reshape(x.shape[0], -1, 8)
                    lo = np.where(g > 0, g, np.inf).min(axis=2)
                    return np.where(np.isfinite(lo), g.max(axis=2) / np.where(np.isfinite(lo), lo, 1.0), 1.0).max()
                assert spread(base.a) * spread(base.w) < 2 ** 13, tag
                for quant in (quantize_act_mxfp8, quantize_act_mxfp6, quantize_act_mxfp4):
                    assert np.array_equal(quant(base.a.astype(np.float32)).astype(np.float64), base.a), (tag, quant.__name__)
            yg, yu = base.y[:, :nh], base.y[:, nh:]
            assert (np.abs(yg) < 4).mean() >= 0.40, (tag, (np.abs(yg) < 4).mean())
            for name, share in (("gate > 7", (yg > 7).mean()), ("up > 7", (yu > 7).mean()), ("up < -7", (yu < -7).mean())):
                assert share >= 0.01, (tag, name, share)
            for act in ACTS:
                P = gated_problem(kind, is_bf16, m, n, k, act, seed)
                assert P.seed == seed, (tag, act, "the evaluation problems are within the cap as drawn")
                check_preconditions(P, is_bf16, (tag, act))
                worst = max(worst, P.undecided)
                want = values16(P.want, is_bf16)
                acc_g, acc_u = P.acc[:, :nh] * P.gs, P.acc[:, nh:] * P.gs
                r16 = lambda v: round16(v, is_bf16)
                oai_only = {
                    "alpha = 1.7": gated64(yg, yu, act, alpha=1.7),
                    "no lower clamp on up": gated64(yg, yu, act, lower_clamp=False),
                    "gate clamped from below as well": gated64(yg, yu, act, gate_lower_clamp=True),
                    "+ 1 before the clamp": gated64(yg, yu, act, one_first=True),
                }
                mutants = {
                    "y rounded to 16 bits before the activation": gated64(r16(yg), r16(yu), act),
                    "silu(g) rounded to 16 bits before the multiply": gated64(yg, yu, act, round_silu=is_bf16),
                    "truncation instead of RNE": None,
                    "up bias taken from the gate half": gated64(yg, acc_u + P.bias[None, :nh], act),
                    "gate and up swapped": gated64(yu, yg, act),
                    "up taken one 16-column tile to the right": gated64(yg, np.roll(yu, -16, axis=1), act),
                }
                for name, v in {**oai_only, **mutants}.items():
                    with np.errstate(invalid="ignore", divide="ignore"):
                        got = round16(P.ref, is_bf16, "trunc") if v is None else round16(v, is_bf16)
                    differs = (got != want)[P.decided].any()
                    if act == 1 and name in oai_only:
                        # SiLU-mul has no alpha, no clamp and no + 1: gated64 takes none of these arguments on its act == 1 path, the mutant IS the
                        # contract and there is nothing to tell apart
                        assert not differs, (tag, act, name)
                    elif name == "gate clamped from below as well" and not is_bf16:
                        # fp16: g sigmoid(1.702 g) is below 4.7e-5 for g < -7, so such an output is a normal fp16 value (and can be decided) only
                        # where |u + 1| > 1.3; a narrow draw (K = 2048 on MXFP4: s = 9) may have no decided output with a gate below -7, and
                        # then the mutant has nothing to change -- it must change bits wherever there is one
                        assert differs or not (P.decided & (yg < -LIMIT)).any(), (tag, act, name)
                    else:
                        assert differs, (tag, act, name)
                # C written at row stride n instead of n / 2: row r lands at r * n, every second row of the buffer stays poison
                flat = np.full(m * nh + m * n, POISON[is_bf16], dtype=np.uint16)
                for r in range(m):
                    flat[r * n: r * n + nh] = P.want[r]
                assert (flat[:m * nh].reshape(m, nh) != P.want)[P.decided].any(), (tag, act, "row stride n")
    print(f"gated_contract {kind} bf16={is_bf16}: largest undecided share of the evaluation problems {worst:.4f} (cap {CAP[is_bf16]})")


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_every_gpu_problem_is_within_the_cap(kind, is_bf16, k):
    """The problems the GPU tests launch (every M, N, activation; the native class's and the Python route's are among or next to them): the
    preconditions and the cap hold on the reference alone, at a seed below SEEDS_TRIED."""
    worst, reseeded = 0.0, 0
    for m in sorted(set(MS) | set(NATIVE_MS) | {ROUTE_M}):
        for n in NS:
            for act in ACTS:
                P = gated_problem(kind, is_bf16, m, n, k, act)
                check_preconditions(P, is_bf16, f"{kind} bf16={is_bf16} m={m} n={n} k={k} act={act} seed={P.seed}")
                worst, reseeded = max(worst, P.undecided), reseeded + (P.seed != 0)
    print(f"gated_contract {kind} bf16={is_bf16} k={k}: largest undecided share {worst:.4f} (cap {CAP[is_bf16]}), {reseeded} problems not at seed 0")


# --- 3. GPU: every id and K split into poisoned, guarded buffers ----------------------------------------------------------------------------

NATIVE_MS, NATIVE_KS, NATIVE_NS = (1, 33, 130, 257), (1280, 2048), (288, 544)
ROUTE_M, ROUTE_K, ROUTE_N = 40, 1280, 544


class GatedDevice(Device):
    """Device whose outputs are judged by the band: P.want or P.alt per output (P.wrong for the subnormal ones), and every launch the bits of the
    problem's first launch."""

    def __init__(self, pk, kind, is_bf16, m, n, k, P, activation):
        super().__init__(pk, kind, is_bf16, m, n, k, P, activation)
        self.alt = torch.from_numpy(P.alt.view(np.int16).copy()).to(DEV).reshape(-1)
        self.first = None

    def compare(self) -> list:
        if self.first is None:
            self.first = self.c_out.clone()
        elif torch.equal(self.c_out, self.first):
            return []                                                                 # (the bits that were judged at the first launch)
        what = []
        if not bool(((self.c_out == self.want) | (self.c_out == self.alt)).all()):
            got = self.c_out.cpu().numpy().view(np.uint16)
            bad = np.flatnonzero(self.P.wrong(got))
            if bad.size:
                what.append(self.describe(got, bad))
        differ = torch.nonzero(self.c_out != self.first).reshape(-1)
        if differ.numel():
            what.append(f"{differ.numel()} outputs differ from the first launch of this problem, first at (row {int(differ[0]) // self.n_out}, "
                        f"col {int(differ[0]) % self.n_out})")
        return what


def run_gated(pk, kind, is_bf16, m, k, ns, ids_of, counts):
    failures = []
    for n in ns:
        for act in ACTS:
            P = gated_problem(kind, is_bf16, m, n, k, act)
            counts["undecided"] = max(counts["undecided"], P.undecided)
            failures += [f"activation {act}: {f}" for f in run_ids(pk, kind, is_bf16, m, n, k, "G", ids_of, counts, activation=act, P=P, device=GatedDevice)]
    return failures


@pytest.mark.gpu
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_exact_class_gated_every_id_bit_for_bit(pk, kind, is_bf16, k, m):
    """SiLU-mul and SwiGLU-OAI through every enumerated kernel, the default pick and every id with K split 2 / 4 / 8 that
    petit_gemm_resolve_solution accepts WITH this epilogue (the rest is counted as refused: odd n-tiles per wave unsplit, the LDS-shared kernel):
    rc 0, the expected bits (module docstring), every launch the bits of the first, no output unwritten, the guards and the scratch guard untouched.
    At K = 256 the split ids of the kinds that drop empty K slices (k_slices: all but the streaming kernels, whose reduce pass applies the
    activation whatever K) run as ONE slice, so the kernel's own epilogue applies it: at least one such launch per case."""
    counts = {"launched": 0, "split": 0, "collapsed": 0, "refused": 0, "undecided": 0.0}
    failures = run_gated(pk, kind, is_bf16, m, k, NS, exact_ids, counts)
    print(f"gated_contract {kind} bf16={is_bf16} k={k} m={m}: {counts}")
    assert k < 1280 or counts["split"] > counts["collapsed"], "no K-split id ran"
    assert k != 256 or counts["collapsed"] > 0, "no collapsed K split ran"
    assert counts["undecided"] <= CAP[is_bf16]
    assert not failures, f"{len(failures)} of {counts['launched']} launches wrong:\n" + "\n".join(failures[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("m", NATIVE_MS)
@pytest.mark.parametrize("k", NATIVE_KS)
@pytest.mark.parametrize("is_bf16", [True, False])
def test_native_class_mxfp4_gated_every_id_bit_for_bit(pk, is_bf16, k, m):
    """The block-scaled-MFMA kernels on MXFP4 weights, K split 1 and 2: acc is the exact class's (the preconditions carry over, they depend on
    the weights and activations alone), so the expected bits are too."""
    counts = {"launched": 0, "split": 0, "refused": 0, "undecided": 0.0}
    pk.ops.enable_native_fp4(True)
    try:
        failures = run_gated(pk, "mx", is_bf16, m, k, NATIVE_NS, native_ids, counts)
    finally:
        pk.ops.enable_native_fp4(False)
    print(f"gated_contract native mx bf16={is_bf16} k={k} m={m}: {counts}")
    assert counts["split"] > 0, "no K-split id ran"
    assert not failures, f"{len(failures)} of {counts['launched']} launches wrong:\n" + "\n".join(failures[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_python_route_writes_every_gated_output(pk, kind, is_bf16, act):
    """mul_*_a16(..., activation=...) and, on MXFP4 weights, mul_mxfp4_native(..., activation=...): torch.empty for C and scratch, the allocator's
    cache emptied and a poisoned block of C's size freed before every call (test_python_route_writes_every_output); the default pick and one id each
    of three kinds write the expected bits."""
    m, n, k = ROUTE_M, ROUTE_N, ROUTE_K
    name = {1: "silu_mul", 2: "swiglu_oai"}[act]
    dtype = torch.bfloat16 if is_bf16 else torch.float16
    P = gated_problem(kind, is_bf16, m, n, k, act)
    D = Device(pk, kind, is_bf16, m, n, k, P, act)
    by_kind = {}
    for sid in pk.ops.get_fp4_solutions(D.h, m, n, k):
        if pk.ops.resolve_solution(D.h, m, n, k, sid, activation=name):
            by_kind.setdefault((sid >> 48) & 0xF, sid)
    assert len(by_kind) >= 3, by_kind
    mul = pk.mul_nvfp4_a16 if kind == "nv" else pk.mul_mxfp4_a16
    calls = [(mul, sid) for sid in [-1] + list(by_kind.values())[:3]]
    if kind == "mx":
        calls += [(pk.mul_mxfp4_native, sid) for sid in (pk.SOLUTION_AUTO_NATIVE_MXFP8, pk.SOLUTION_AUTO_NATIVE_MXFP6, pk.SOLUTION_AUTO_NATIVE_MXFP4)]
    first = None
    for fn, sid in calls:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        poison = torch.full((m, n // 2), POISON[is_bf16], dtype=torch.int16, device=DEV)
        del poison
        c = fn(D.a.view(dtype).reshape(m, k), D.b, D.sp, D.gs, m, n, k, sid, bias=D.bias.view(dtype), activation=name)
        assert c.shape == (m, n // 2) and c.dtype == dtype
        got = c.view(torch.int16).reshape(-1).cpu().numpy().view(np.uint16)
        bad = np.flatnonzero(P.wrong(got))
        assert bad.size == 0, (f"{fn.__name__} {sid:#x}: {bad.size} outputs wrong, {int((got[bad] == POISON[is_bf16]).sum())} unwritten, first at "
                               f"{divmod(int(bad[0]), n // 2)}")
        first = got if first is None else first
        assert np.array_equal(got, first), f"{fn.__name__} {sid:#x}: not the bits of the first call"


# --- 4. the quantising form: out_format 8 / 6 / 4 ---------------------------------------------------------------------------------------------

QUANT_MS, QUANT_K, QUANT_NS, QUANT_FORMATS = (5, 130), 1280, (512, 1024), ("mxfp8", "mxfp6", "mxfp4")
QUANT_BLOCK_CAP = 0.02                           # blocks whose scale byte the band leaves open


def quant_expect(P, fmt):
    """What the quantising epilogue may write for the problem P (after expect): sbyte [m, n/2 / 32] and keep (the blocks whose scale byte the
    band around the block maximum does not leave open), q_lo / q_hi [m, n/2] (the dequantised codes of the two ends of each element's band: the
    quantisers are monotone, so a device value inside the band has one of the two)."""
    from test_gpu_parity import quantize_act_mxfp4, quantize_act_mxfp6, quantize_act_mxfp8
    quant = {"mxfp8": quantize_act_mxfp8, "mxfp6": quantize_act_mxfp6, "mxfp4": quantize_act_mxfp4}[fmt]
    m, nh = P.ref.shape
    mag = np.abs(P.ref)
    ebits = lambda amax: ((amax.astype(np.float32).view(np.uint32) >> 23) & 0xFF).astype(np.int64)
    blocks = lambda x: x.reshape(m, nh // 32, 32).max(axis=2)
    e_lo, e_mid, e_hi = ebits(blocks(mag * (1 - P.delta))), ebits(blocks(mag)), ebits(blocks(mag * (1 + P.delta)))
    keep = (e_lo == e_hi) & (blocks(mag) > 0)
    sbyte = np.clip(e_mid - (7 if fmt == "mxfp8" else 2), 1, 254)
    lo, hi = P.ref - mag * P.delta, P.ref + mag * P.delta
    return sbyte, keep, quant(lo).astype(np.float64), quant(hi).astype(np.float64)


@pytest.mark.parametrize("is_bf16", [True, False])
def test_quantising_form_blocks_left_open_are_within_the_cap(is_bf16):
    """On the reference alone: at most 2 % of the 32-column blocks of a quantising case have a maximum whose band crosses a power of two."""
    for m in QUANT_MS:
        for n in QUANT_NS:
            for act in ACTS:
                P = gated_problem("mx", is_bf16, m, n, QUANT_K, act)
                check_preconditions(P, is_bf16, f"mx bf16={is_bf16} m={m} n={n} act={act}")
                _, keep, q_lo, q_hi = quant_expect(P, "mxfp4")
                assert (~keep).mean() <= QUANT_BLOCK_CAP, (m, n, act, (~keep).mean())
                assert (q_lo != q_hi).mean() <= 0.01, "the codes are all but decided"


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", QUANT_FORMATS)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("is_bf16", [True, False])
def test_quantising_gated_epilogue_codes_and_scales(pk, is_bf16, act, fmt):
    """petit_gemm_mxfp4_native with out_format: the class's default pick writes, into a poisoned buffer of exactly the layout's bytes between two
    guards, the scale byte the quantiser's rule gives on the reference's block maximum and the quantiser's code of the reference for every element
    (module docstring for the two exceptions); every byte is written (two launches over two different poisons agree) and nothing past them."""
    from petit_kernel import _lib
    from test_gpu_parity import decode_qact
    L = _lib.lib
    code = {"mxfp8": 8, "mxfp6": 6, "mxfp4": 4}[fmt]
    sid = {"mxfp8": _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP8, "mxfp6": _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP6, "mxfp4": _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP4}[fmt]
    k, failures = QUANT_K, []
    for m in QUANT_MS:
        for n in QUANT_NS:
            nh = n // 2
            P = gated_problem("mx", is_bf16, m, n, k, act)
            D = Device(pk, "mx", is_bf16, m, n, k, P, act)
            sbyte, keep, q_lo, q_hi = quant_expect(P, fmt)
            na = _lib.NativeArgs(C.sizeof(_lib.NativeArgs), 0, code, 0)
            nbytes = int(L.petit_quantized_activation_bytes(m, nh, code))
            assert nbytes == m * (nh // 8 * code) + m * (nh // 32)                    # native32_ws_bytes of the half-width matrix
            need = int(L.petit_gemm_native_workspace_bytes(C.byref(D.hints), m, n, k, C.c_uint64(sid), D.epi, C.byref(na)))
            assert int(L.petit_gemm_resolve_solution(C.byref(D.hints), m, n, k, C.c_uint64(sid), D.epi, C.c_uint64(need))) != 0
            out_all = torch.empty(GUARD + nbytes + GUARD, dtype=torch.uint8, device=DEV)
            ws_all = torch.empty(need + GUARD, dtype=torch.uint8, device=DEV)
            tag = f"m={m} n={n}"
            raws = []
            for poison in (0xC1, 0x3E):
                out_all.fill_(poison)
                ws_all.fill_(poison)
                out = out_all[GUARD:GUARD + nbytes]
                rc = L.petit_gemm_mxfp4_native(C.c_void_p(out.data_ptr()), C.c_void_p(D.a.data_ptr()), C.c_void_p(D.b.data_ptr()),
                                               C.c_void_p(D.sp.data_ptr()), C.c_void_p(D.gs.data_ptr()), m, n, k, C.byref(D.hints), C.c_uint64(sid),
                                               D.epi, C.byref(na), C.c_void_p(ws_all.data_ptr()), C.c_uint64(need),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
                assert rc == 0, (tag, rc, _lib.error_string(rc))
                whole = out_all.cpu().numpy()
                if (whole[:GUARD] != poison).any() or (whole[GUARD + nbytes:] != poison).any():
                    failures.append(f"{tag}: a guard of the output was written")
                if (ws_all[need:] != poison).any():
                    failures.append(f"{tag}: scratch written past the {need} declared bytes")
                raws.append(whole[GUARD:GUARD + nbytes].copy())
            unwritten = int((raws[0] != raws[1]).sum())
            if unwritten:
                failures.append(f"{tag}: {unwritten} of {nbytes} output bytes were not written (they keep the poison of each launch)")
                continue
            raw = raws[0]
            got_s = raw[m * (nh // 8 * code):].reshape(nh // 128, m, 4).transpose(1, 0, 2).reshape(m, nh // 32).astype(np.int64)
            bad_s = keep & (got_s != sbyte)
            if bad_s.any():
                r, b = np.argwhere(bad_s)[0]
                failures.append(f"{tag}: {int(bad_s.sum())} scale bytes wrong, first at (row {r}, block {b}): got {got_s[r, b]} want {sbyte[r, b]}")
            got = decode_qact(raw, m, nh, fmt).astype(np.float64)
            bad = np.repeat(keep & ~bad_s, 32, axis=1) & (got != q_lo) & (got != q_hi)
            if bad.any():
                r, c = np.argwhere(bad)[0]
                failures.append(f"{tag}: {int(bad.sum())} codes wrong, first at (row {r}, col {c}): got {got[r, c]!r} want {q_lo[r, c]!r} / "
                                f"{q_hi[r, c]!r} (reference {P.ref[r, c]!r})")
            print(f"gated_contract quantising bf16={is_bf16} act={act} {fmt} {tag}: {int((~keep).sum())} of {keep.size} blocks left open, "
                  f"{int((q_lo != q_hi).sum())} of {q_lo.size} codes undecided")
    assert not failures, "\n".join(failures)

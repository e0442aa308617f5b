"""The epilogue and write contract of the dense GEMMs, bit for bit: c = RNE16(fma(acc, gs, bias)), ONE rounding, every output written, nothing
written outside C or past the scratch petit_gemm_workspace_bytes_ex declares.

Method: inputs on which every product and every partial sum, in ANY order, is exactly representable in fp32 (exact_problem).  acc is then the same
number in every kernel, tile shape and K split, y = acc * gs + bias survives fp32, and the 16 output bits are determined uniquely: they are computed
here in float64 (exact on these inputs) and rounded once.  Tolerance: none.
  * regime "A" (representable): |w| in {0, .5, 1}, block scales {1, 2}, activations +-1 at density 1/4, gs = 2, no bias -- nearly every output is
    exactly representable in the output type, so one dropped or doubled k term changes bits.
  * regime "B" (rounding): all 16 codes, block scales {.5, 1, 1.5, 2, 3} (NV) / e8m0 126..129 (MX), activations from {+-1, +-2, +-3} at density
    1/2, gs = 0.75, bias multiples of .25 in [-8, 8] -- several per cent of the outputs are exact ties of the output type, so truncation, round
    half away, a rounding before the bias or a 16-bit rounding of a K part each change bits (test_generator_preconditions_and_teeth shows it;
    one mutant is the identity by arithmetic: in fp16 at K = 256, one span that no launch splits, the sums of a K half are fp16 values).
The CPU tests state the preconditions that make this true; the GPU tests launch through the C ABI into caller-owned buffers: C sits between two
guards, a K split's scratch is exactly the declared bytes followed by a guard, and everything is filled with a NaN pattern before EVERY launch, so
an output nobody wrote, a write outside C and a write past the declared scratch all show.

Native class (block-scaled MFMA): MXFP4 weights only.  On these inputs the activation quantisers are exact, every 8-k group of e4m3 products spans
less than 2^13, and the accumulator alignment of the instruction (test_gpu_parity.native_exact_bound) truncates below the quantum of the sums, so
the expected bits are the exact class's.  The NVFP4 native image is left out: its e2m3 x e8m0-per-32 re-encoding is not the exact dequant of
regime B's weights (two 16-k groups with scales 0.5 and 3 share one e8m0 scale; test_nvfp4_native_image_is_not_exact_on_regime_b pins that), and
test_native_nvfp4_every_kernel already judges that path against the image's own weights.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as O

DEV = "cuda"
FAMILIES = [("nv", True), ("nv", False), ("mx", True), ("mx", False)]
KS = (256, 1280, 2048, 2560, 5120)
MS = (1, 3, 4, 5, 16, 17, 40, 128, 129, 257)
NS = {"nv": (16, 272), "mx": (32, 288)}
REGIMES = ("A", "B")
REGIMES_ALL = ("A", "B", "G")                   # (the position seeds the generator: A and B keep the streams they always had)
POISON = {True: 0x7FC1, False: 0x7E01}          # a NaN of the output type: no expected value is one
GUARD = 4096                                    # bytes on either side of C and behind the scratch
E4M3_BYTE = {0.5: 0x30, 1.0: 0x38, 1.5: 0x3C, 2.0: 0x40, 3.0: 0x44}
FP4 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0])


@pytest.fixture(scope="module")
def pk():
    import petit_kernel
    assert torch.cuda.is_available()
    name = torch.cuda.get_device_properties(0).gcnArchName
    assert name.startswith("gfx950"), f"these kernels are gfx950 code objects, device is {name}"
    return petit_kernel


# --- 1. the generator and the CPU model (plain numpy) ------------------------------------------------------------------------------------

def round16(y: np.ndarray, is_bf16: bool, mode: str = "rne") -> np.ndarray:
    """float64 -> the nearest value of the output type as float64 (normal range: the callers assert it), mode "rne" / "trunc" / "away"."""
    p = 8 if is_bf16 else 11
    mant, exp = np.frexp(y)
    x = np.ldexp(mant, p)                          # |x| in [2^(p-1), 2^p): integers are the type's values
    r = {"rne": np.rint, "trunc": np.trunc, "away": lambda v: np.trunc(v + np.copysign(0.5, v))}[mode](x)
    return np.ldexp(r, exp - p)


def to_bits(v: np.ndarray, is_bf16: bool) -> np.ndarray:
    """Values ALREADY of the output type (float64) -> their 16 bits."""
    if is_bf16:
        f = v.astype(np.float32)
        assert np.array_equal(f.astype(np.float64), v) and not (f.view(np.uint32) & 0xFFFF).any()
        return (f.view(np.uint32) >> 16).astype(np.uint16)
    h = v.astype(np.float16)
    assert np.array_equal(h.astype(np.float64), v)
    return h.view(np.uint16)


def rne_bits(y: np.ndarray, is_bf16: bool) -> np.ndarray:
    """The contract's rounding by the project's own statements of it: O.f32_to_bf16_bits / IEEE float16 conversion."""
    y32 = y.astype(np.float32)
    assert np.array_equal(y32.astype(np.float64), y), "y must survive float32: then the kernel's fma is exact"
    return O.f32_to_bf16_bits(y32) if is_bf16 else y.astype(np.float16).view(np.uint16)


class Problem:
    pass


def exact_problem(kind, is_bf16, m, n, k, regime, seed, shift=None, mx_shift=0, switch=None):
    """-> Problem with the launch operands (a_bits u16 [m, k], q u8 [n, k/2], s u8 block scale bytes, gs, bias bits u16 [n] or None), the expected
    output bits `want` u16 [m, n], and the float64 model behind them (a [m, k], w [n, k] = code value x block scale, acc, y, quantum).
    Regime "G" (the gated epilogues, test_gated_contract.py): B's weights and activations, gs = 3 * 2^-shift, a bias of multiples of 2^-4 drawn for
    every column, for the gate half from [1, 2], for the up half with magnitude in [1.5, 2] and either sign (the gated module says why); `want` is
    then the PLAIN epilogue's, the gated module derives its own.
    Two options of test_value_contract.py on MXFP4 weights, applied after every draw (the streams of A, B and G stay what they were):
    mx_shift = d moves every e8m0 byte by d and multiplies the launched gs by 2^-d (P.gs; the model keeps w, acc, y and `want` of the unshifted
    problem: every weight moved by one power of two); switch = "mid" / "last" zeroes chosen 32-blocks (codes 0 or 8) under a scale byte outside
    114..140 (switch_blocks), which the model's w, acc, y and `want` follow."""
    rng = np.random.default_rng([seed, kind == "mx", is_bf16, m, n, k, REGIMES_ALL.index(regime)])
    group = 16 if kind == "nv" else 32
    P = Problem()
    if regime == "A":
        code = rng.choice(np.array([0, 1, 2, 8, 9, 10], dtype=np.uint8), (n, k))
        scales = np.array([1.0, 2.0])
        a = rng.choice(np.array([-1.0, 1.0]), (m, k)) * (rng.random((m, k)) < 0.25)
        P.gs, bias, P.quantum = 2.0, None, 0.5
    else:
        code = rng.integers(0, 16, (n, k), dtype=np.uint8)
        scales = np.array([0.5, 1.0, 1.5, 2.0, 3.0] if kind == "nv" else [0.5, 1.0, 2.0, 4.0])
        a = rng.choice(np.array([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0]), (m, k)) * (rng.random((m, k)) < 0.5)
        if regime == "B":
            P.gs, bias, P.quantum = 0.75, rng.integers(-32, 33, n) * 0.25, 0.25
        else:
            gate, up = rng.integers(16, 33, n // 2), rng.integers(24, 33, n // 2) * rng.choice(np.array([-1, 1]), n // 2)
            P.gs, bias, P.quantum = 3.0 * 2.0 ** -shift, np.concatenate([gate, up]) * 2.0 ** -4, 0.25
    a = a + 0.0                                                                       # (no -0.0 activations)
    P.q = (code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8)
    sidx = rng.integers(0, len(scales), (n, k // group))
    sval = scales[sidx]
    sbyte = [E4M3_BYTE[v] for v in scales] if kind == "nv" else [127 + int(np.log2(v)) for v in scales]      # e4m3 bytes / e8m0 126..129
    P.s = np.array(sbyte, dtype=np.uint8)[sidx]
    keep = np.ones((n, k), dtype=bool)
    if switch is not None:
        assert kind == "mx"
        P.switched = switch_blocks(n, k, seed, switch)
        for row, blk, byte, negative in P.switched:
            code[row, 32 * blk:32 * blk + 32], P.s[row, blk], keep[row, 32 * blk:32 * blk + 32] = 8 * negative, byte, False
        P.q = (code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8)
    if mx_shift:
        assert kind == "mx" and 1 <= int(P.s.min()) + mx_shift and int(P.s.max()) + mx_shift <= 254
        P.s = (P.s.astype(np.int64) + mx_shift).astype(np.uint8)
    P.a, P.w = a, FP4[code] * np.repeat(sval, group, axis=1) * keep
    P.a_bits = to_bits(a, is_bf16)
    P.bias = bias
    P.bias_bits = None if bias is None else to_bits(bias, is_bf16)
    P.acc = a @ P.w.T                                                                 # float64: exact, see the preconditions
    P.y = P.acc * P.gs + (0.0 if bias is None else bias[None, :])                     # (+ 0.0: the kernel's fma adds a +0 bias, -0 becomes +0)
    P.want = rne_bits(P.y, is_bf16)
    P.mx_shift, P.gs = mx_shift, P.gs * 2.0 ** -mx_shift                              # (the launched gs; y above is the unshifted problem's)
    return P


def switch_blocks(n, k, seed, variant):
    """[(row, 32-block, scale byte, negative zeros)] of regime "S": the placement of test_gpu_parity.mx_f16_scale_profiles' switch profile -- every
    even 16-row tile gets one block in the second half of K, a few tiles one anywhere, row 5 the very first block -- or, variant "last", every
    even tile one block in the last 256 k, so that the fp16 x MXFP4 kernels switch bodies right before their accumulators join."""
    rng = np.random.default_rng([seed, n, k, variant == "last", 0x53])
    kb, out = k // 32, {}
    for t in range(0, n // 16, 2):
        blk = kb - 8 + int(rng.integers(0, 8)) if variant == "last" else kb // 2 + int(rng.integers(0, kb - kb // 2))
        out[(16 * t + int(rng.integers(0, 16)), blk)] = int(rng.choice([100, 113, 141, 143]))
    if variant != "last":
        for t in rng.integers(0, n // 16, max(1, n // 64)):
            out[(16 * int(t) + int(rng.integers(0, 16)), int(rng.integers(0, kb)))] = int(rng.choice([100, 113, 141, 143]))
        out[(5 % n, 0)] = 141
    return [(row, blk, byte, int(rng.integers(0, 2))) for (row, blk), byte in sorted(out.items())]


def shares(P, is_bf16):
    """(share of outputs exactly representable in the output type, share that are exact ties between two of its neighbours)."""
    mant, _ = np.frexp(P.y)
    frac = np.abs(np.ldexp(mant, 8 if is_bf16 else 11)) % 1.0
    return float((frac == 0).mean()), float((frac == 0.5).mean())


EVAL_M, EVAL_N, SEEDS = 64, 288, (0, 1, 2)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_generator_preconditions_and_teeth(kind, is_bf16, regime):
    """What makes "any order gives the same bits" true on these inputs, what keeps the cases from going soft, and that each wrong epilogue the
    contract excludes changes expected bits (so a kernel that had it could not pass)."""
    from test_gpu_parity import quantize_act_mxfp4, quantize_act_mxfp6, quantize_act_mxfp8
    for k in KS:
        for seed in SEEDS:
            P = exact_problem(kind, is_bf16, EVAL_M, EVAL_N, k, regime, seed)
            tag = f"{kind} bf16={is_bf16} {regime} K={k} seed={seed}"
            # the bytes mean what the model says (the oracle's dequant), and the activations are the 16-bit values
            dq = O.dequant_nvfp4(P.q, P.s) if kind == "nv" else O.dequant_mxfp4(P.q, P.s)
            assert np.array_equal(dq.astype(np.float64), P.w), tag
            a16 = O.bf16_bits_to_f32(P.a_bits) if is_bf16 else O.f16_bits_to_f32(P.a_bits)
            assert np.array_equal(a16.astype(np.float64), P.a), tag
            # every product is a multiple of the quantum and sum |a||w| stays below 2^24 quanta: any partial sum in any association is exact in fp32
            assert np.array_equal(np.rint(P.a / 1.0), P.a) and np.array_equal(np.rint(P.w / P.quantum), P.w / P.quantum), tag
            assert (np.abs(P.a) @ np.abs(P.w).T).max() / P.quantum < 2 ** 24, tag
            # y survives float32 (rne_bits asserted it): fma(acc, gs, bias) is exact; finite and in the normal range of the output type
            assert np.abs(P.y).max() < (3e38 if is_bf16 else 65504.0), tag
            assert (P.y == 0).all() or np.abs(P.y[P.y != 0]).min() >= 2.0 ** -14, tag
            assert np.array_equal(to_bits(round16(P.y, is_bf16), is_bf16), P.want), tag       # the model's RNE is the project's
            assert not np.any(P.want == POISON[is_bf16]), tag
            if kind == "mx":       # the native class (MXFP4 weights)
                # e4m3 activations: inside every group of 8 consecutive k, largest |product| / smallest non-zero |product| < 2^13 -- bounded by
                # (largest / smallest non-zero |a| of the group) x (largest / smallest non-zero |w| of the group)
                def spread(x):
                    g = np.abs(x).reshape(x.shape[0], -1, 8)
                    lo = np.where(g > 0, g, np.inf).min(axis=2)
                    return np.where(np.isfinite(lo), g.max(axis=2) / np.where(np.isfinite(lo), lo, 1.0), 1.0).max()
                assert spread(P.a) * spread(P.w) < 2 ** 13, tag
                # the activation quantisers reproduce these activations exactly
                for quant in (quantize_act_mxfp8, quantize_act_mxfp6, quantize_act_mxfp4):
                    assert np.array_equal(quant(P.a.astype(np.float32)).astype(np.float64), P.a), (tag, quant.__name__)
            rep, tie = shares(P, is_bf16)
            if regime == "A":
                assert rep >= 0.99, (tag, rep)
                # dropping or doubling one k index changes at least one bit in every row that has a non-zero activation there
                for k0 in np.random.default_rng(seed).integers(0, k, 8):
                    delta = P.gs * np.outer(P.a[:, k0], P.w[:, k0])
                    rows = P.a[:, k0] != 0
                    assert rows.any() and (P.w[:, k0] != 0).any(), tag
                    for mutant in (P.y - delta, P.y + delta):
                        changed = (rne_bits(mutant, is_bf16) != P.want).any(axis=1)
                        assert changed[rows].all(), (tag, int(k0))
            else:
                assert tie >= 0.04, (tag, tie)
                h = k // 2
                acc_lo, acc_hi = P.a[:, :h] @ P.w[:, :h].T, P.a[:, h:] @ P.w[:, h:].T
                mutants = {
                    "truncate": round16(P.y, is_bf16, "trunc"),
                    "round half away from zero": round16(P.y, is_bf16, "away"),
                    "round acc * gs before the bias": round16(round16(P.acc * P.gs, is_bf16) + P.bias[None, :], is_bf16),
                    "round one K half to 16 bit": round16((round16(acc_lo, is_bf16) + acc_hi) * P.gs + P.bias[None, :], is_bf16),
                }
                for name, v in mutants.items():
                    differs = (to_bits(v, is_bf16) != P.want).any()
                    if k == 256 and not is_bf16 and name == "round one K half to 16 bit":
                        # one 256-span, which no launch splits: in fp16 the sums of 128 terms (multiples of 1/4 below 512) are fp16 values
                        # themselves, the mutant is then the contract and there is nothing to tell apart
                        assert differs or np.array_equal(round16(acc_lo, is_bf16), acc_lo), (tag, name)
                    else:
                        assert differs, (tag, name)


def test_nvfp4_native_image_is_not_exact_on_regime_b():
    """Why the NVFP4 native image path is not in this module: petit_nvfp4_native_image_dequant_host of the image is the exact dequant of regime A's
    weights but not of regime B's (e2m3 elements under one e8m0 scale per 32 k cannot hold 6 x 3 next to 0.5 x 0.5)."""
    from petit_kernel import offline
    n, k = 272, 1280
    exact = {}
    for regime in REGIMES:
        P = exact_problem("nv", True, 1, n, k, regime, 0)
        b = offline.repack_nvfp4_cpu(torch.from_numpy(P.q).view(torch.int32), n, k)
        sp = offline.process_nvfp4_scales_cpu(torch.from_numpy(P.s).view(torch.float8_e4m3fn), n, k)
        image = offline.nvfp4_native_image_cpu(b, sp, n, k)
        dq = offline.nvfp4_native_image_dequant_cpu(image, n, k).numpy().astype(np.float64)
        exact[regime] = bool(np.array_equal(dq, P.w))
    assert exact == {"A": True, "B": False}, exact


# --- 2. the GPU side: through the C ABI into caller-owned, poisoned, guarded buffers -------------------------------------------------------

def with_split(sid: int, split: int) -> int:
    return (sid & ~(0xF << 60)) | (split << 60)


def k_slices(sid: int, k: int) -> int:
    """The K slices (grid z) the launch of an explicit id makes: launch_geometry of csrc/solution.h restated on the id's fields.  nspans spans of
    ks k-tiles go to `split` slices of kparts in-workgroup parts each, spans_per_part = ceil(nspans / (split kparts)), and the slices that then own no
    span are dropped -- except by the streaming kinds (gemm_stream.hpp), whose grid z is the split the id names whatever K.  One slice: no slabs, no
    reduce pass, the kernel's own epilogue writes C (and applies a gated activation)."""
    split, ks = max(1, (sid >> 60) & 0xF), ((sid >> 16) & 0x1F) // 2
    code, wm, wk = (sid >> 48) & 0xF, (sid >> 36) & 0xF, (sid >> 44) & 0xF
    if code in (0, 1, 2, 3, 5, 6, 7, 10, 11) and wm == 1:                             # shape_is_stream: even_split
        return split
    if code in (4, 14, 15) or (code in (1, 2, 3, 10, 11) and wm == 2):               # decode / mid: one_slice (they refuse a split)
        return 1
    kparts = (2 if code in (12, 13) and wm == 3 else 1) if code in (8, 9, 12, 13) else wk
    nspans = k // (128 * ks)
    spp = -(-nspans // (split * kparts))
    return -(-nspans // (spp * kparts)) if spp else 1


ACTIVATION_NAMES = {0: None, 1: "silu_mul", 2: "swiglu_oai"}


class Device:
    """One problem's operands on the device, its guarded C and scratch, and the launch + check of one solution id.  activation 1 / 2 (the gated
    epilogues): C is the m * n / 2 outputs between its guards, the Epilogue carries the activation and P.want is [m, n / 2].  `compare` judges
    the outputs of a launch: here by equality with P.want; a subclass may judge otherwise (test_gated_contract.GatedDevice)."""

    def __init__(self, pk, kind, is_bf16, m, n, k, P, activation=0):
        from petit_kernel import _lib
        self.pk, self.L, self.kind, self.is_bf16, self.m, self.n, self.k = pk, _lib, kind, is_bf16, m, n, k
        self.activation, self.n_out, self.P = activation, n // 2 if activation else n, P
        self.dtype = torch.bfloat16 if is_bf16 else torch.float16
        dev16 = lambda b: torch.from_numpy(b.view(np.int16).copy()).to(DEV)
        self.a = dev16(P.a_bits)
        qd = torch.from_numpy(P.q).to(DEV).view(torch.int32)
        if kind == "nv":
            self.b = pk.repack_nvfp4(qd, n, k)
            self.sp = pk.process_nvfp4_scales(torch.from_numpy(P.s).to(DEV).view(torch.float8_e4m3fn), n, k)
            self.fn = _lib.lib.petit_gemm_fp4_fp16_grid_ws
        else:
            self.b = pk.repack_mxfp4(qd, n, k)
            self.sp = pk.process_mxfp4_scales(torch.from_numpy(P.s).to(DEV), n, k)
            self.fn = _lib.lib.petit_gemm_mxfp4_fp16_grid_ws
        self.gs = torch.tensor([P.gs], dtype=torch.float32, device=DEV)
        self.bias = None if P.bias_bits is None else dev16(P.bias_bits)
        self.want = dev16(P.want).reshape(-1)
        a_type = _lib.CXX_DTYPE_BF16 if is_bf16 else _lib.CXX_DTYPE_FP16
        self.hints = _lib.SolutionHints(a_type, _lib.CXX_DTYPE_FP4_E2M1 if kind == "nv" else _lib.CXX_DTYPE_MXFP4_E2M1, a_type, 0)
        with_epilogue = self.bias is not None or activation
        self.epilogue = _lib.Epilogue(None if self.bias is None else self.bias.data_ptr(), activation, 0) if with_epilogue else None
        self.epi = C.byref(self.epilogue) if with_epilogue else None
        self.h = pk.PetitSolutionHints()
        self.h.a_type = self.h.c_type = self.dtype
        self.h.b_type = pk.DataType.float4_e2m1 if kind == "nv" else pk.DataType.mxfloat4_e2m1
        self.poison = POISON[is_bf16]
        g = GUARD // 2
        mn = m * self.n_out
        assert self.want.numel() == mn
        self.c_all = torch.empty(g + mn + g, dtype=torch.int16, device=DEV)          # [guard | m * n_out outputs | guard]
        self.c_lo, self.c_out, self.c_hi = self.c_all[:g], self.c_all[g:g + mn], self.c_all[g + mn:]
        self.guard = torch.full((g,), self.poison, dtype=torch.int16, device=DEV)
        self.ws_all = self.ws_ref = None

    def need(self, sid: int) -> int:
        return int(self.L.lib.petit_gemm_workspace_bytes_ex(C.byref(self.hints), self.m, self.n, self.k, C.c_uint64(sid & (2 ** 64 - 1)),
                                                            self.epi if self.activation else None))

    def reserve_scratch(self, most: int) -> None:
        """One allocation that serves every id of the problem: an id is handed its declared bytes, all that follows is guard."""
        total = (most + GUARD + 511) // 512 * 512
        self.ws_all = torch.empty(total // 2, dtype=torch.int16, device=DEV)
        self.ws_ref = torch.full((total // 2,), self.poison, dtype=torch.int16, device=DEV).view(torch.uint8)

    def compare(self) -> list:
        """What is wrong with the outputs the launch just made left in C: none, or one line of the report."""
        if torch.equal(self.c_out, self.want):
            return []
        got = self.c_out.cpu().numpy().view(np.uint16)
        return [self.describe(got, np.flatnonzero(got != self.P.want.reshape(-1)))]

    def describe(self, got, bad) -> str:
        want = self.P.want.reshape(-1)
        rows, cols = bad // self.n_out, bad % self.n_out
        return (f"{bad.size} of {got.size} outputs differ, {int((got[bad] == self.poison).sum())} of them unwritten (still poison); first at "
                f"(row {rows[0]}, col {cols[0]}): got {got[bad[0]]:#06x} want {want[bad[0]]:#06x}; rows {rows.min()}..{rows.max()}, "
                f"cols {cols.min()}..{cols.max()}")

    def run(self, sid: int):
        """Poison, launch, compare on the device -> None, or the report of what is wrong."""
        sid &= 2 ** 64 - 1
        need = self.need(sid)
        self.c_all.fill_(self.poison)
        self.ws_all.fill_(self.poison)
        rc = self.fn(C.c_void_p(self.c_out.data_ptr()), C.c_void_p(self.a.data_ptr()), C.c_void_p(self.b.data_ptr()), C.c_void_p(self.sp.data_ptr()),
                     C.c_void_p(self.gs.data_ptr()), self.m, self.n, self.k, C.byref(self.hints), C.c_uint64(sid), self.epi,
                     C.c_void_p(self.ws_all.data_ptr()) if need else None, C.c_uint64(need),
                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
        what = []
        if rc != 0:
            what.append(f"the queries accept the call, the launch returns {rc} ({self.L.error_string(rc)})")
        else:
            what += self.compare()
        if not torch.equal(self.c_lo, self.guard):
            what.append("the guard in front of C was written")
        if not torch.equal(self.c_hi, self.guard):
            what.append("the guard behind C was written")
        ws8 = self.ws_all.view(torch.uint8)
        if not torch.equal(ws8[need:], self.ws_ref[need:]):
            first = int(torch.nonzero(ws8[need:] != self.ws_ref[need:])[0])
            what.append(f"scratch written {first} bytes past the {need} bytes petit_gemm_workspace_bytes_ex declares")
        if not what:
            return None
        return f"m={self.m} n={self.n} k={self.k} id {sid:#x} [{self.L.describe_solution(sid)}]: " + "; ".join(what)


def run_ids(pk, kind, is_bf16, m, n, k, regime, ids_of, counts, activation=0, P=None, device=Device):
    """Every id `ids_of(D)` names for the problem: launched when the library resolves it, counted when it refuses.  -> the reports of what failed.
    activation 1 / 2: the gated epilogues on the problem P of the caller (regime "G" with its [m, n / 2] expectation), judged by `device`.
    counts["collapsed"]: the launched ids that name a K split and run as ONE slice (k_slices); counts["kinds"], where the caller put a set there:
    the kind nibbles of the launched ids."""
    P = P or exact_problem(kind, is_bf16, m, n, k, regime, 0)
    D = device(pk, kind, is_bf16, m, n, k, P, activation)
    enumerated, ids = ids_of(D)
    runnable = []
    for sid in ids:
        if pk.ops.resolve_solution(D.h, m, n, k, sid, activation=ACTIVATION_NAMES[activation]) != 0:
            runnable.append(sid)
        else:
            counts["refused"] += 1
    # (a gated epilogue is refused by the kernels that cannot pair the halves: odd n-tiles per wave unsplit, the LDS-shared kernel)
    assert (runnable if activation else len(runnable) >= len(enumerated) > 0), "every enumerated id runs"
    D.reserve_scratch(max(D.need(sid) for sid in runnable))
    failures = []
    for sid in runnable:
        report = D.run(sid)
        counts["launched"] += 1
        counts["split"] += sid >= 0 and (sid >> 60) & 0xF > 1
        counts["collapsed"] = counts.get("collapsed", 0) + (sid >= 0 and (sid >> 60) & 0xF > 1 and k_slices(sid, k) == 1)
        if "kinds" in counts and sid >= 0:
            counts["kinds"].add((sid >> 48) & 0xF)                                    # (the kind nibbles that ran: test_value_contract.py)
        if report:
            failures.append(f"regime {regime}: {report}")
    return failures


def exact_ids(D):
    sols = list(D.pk.ops.get_fp4_solutions(D.h, D.m, D.n, D.k))
    ids = [-1] + sols + [with_split(sid, sp) for sid in sols for sp in (2, 4, 8)]
    return sols, list(dict.fromkeys(ids))


@pytest.mark.gpu
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_exact_class_every_id_bit_for_bit(pk, kind, is_bf16, k, m):
    """Every enumerated kernel, the default pick and every id with K split 2 / 4 / 8 that the library accepts: the expected bits, no output left
    unwritten, both C guards and the scratch guard untouched."""
    counts = {"launched": 0, "split": 0, "refused": 0}
    failures = []
    for n in NS[kind]:
        for regime in REGIMES:
            failures += run_ids(pk, kind, is_bf16, m, n, k, regime, exact_ids, counts)
    print(f"exact_contract {kind} bf16={is_bf16} k={k} m={m}: {counts}")
    assert k < 1280 or counts["split"] > 0, "no K-split id ran"
    assert not failures, f"{len(failures)} of {counts['launched']} launches wrong:\n" + "\n".join(failures[:20])


def native_ids(D):
    sols = [sid for sid in D.pk.ops.get_fp4_solutions(D.h, D.m, D.n, D.k) if (sid >> 48) & 0xF in (9, 13)]
    return sols, list(dict.fromkeys(with_split(sid, sp) for sid in sols for sp in (1, 2)))


@pytest.mark.gpu
@pytest.mark.parametrize("m", (1, 33, 130, 257))
@pytest.mark.parametrize("k", (1280, 2048))
@pytest.mark.parametrize("is_bf16", [True, False])
def test_native_class_mxfp4_every_id_bit_for_bit(pk, is_bf16, k, m):
    """The block-scaled-MFMA kernels on MXFP4 weights (16x16x128 and 32x32x64, MXFP8 / MXFP6 / MXFP4 activations), K split 1 and 2: the exact
    class's bits (module docstring), the same guards; the scratch holds the quantised activations in front of the slabs."""
    counts = {"launched": 0, "split": 0, "refused": 0}
    failures = []
    pk.ops.enable_native_fp4(True)
    try:
        for regime in REGIMES:
            failures += run_ids(pk, "mx", is_bf16, m, 288, k, regime, native_ids, counts)
    finally:
        pk.ops.enable_native_fp4(False)
    print(f"exact_contract native mx bf16={is_bf16} k={k} m={m}: {counts}")
    assert counts["split"] > 0, "no K-split id ran"
    assert not failures, f"{len(failures)} of {counts['launched']} launches wrong:\n" + "\n".join(failures[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,is_bf16", FAMILIES)
def test_python_route_writes_every_output(pk, kind, is_bf16):
    """mul_*_a16 (torch.empty for C and scratch): the allocator's cache is emptied and a block of C's size is filled with poison and freed before
    every call, so the block the call's torch.empty gets holds poison, not an earlier kernel's answer; the default pick and one id each of three
    different kinds give the expected bits."""
    m, k = 40, 1280
    n = NS[kind][1]
    dtype = torch.bfloat16 if is_bf16 else torch.float16
    P = exact_problem(kind, is_bf16, m, n, k, "B", 1)
    D = Device(pk, kind, is_bf16, m, n, k, P)
    by_kind = {}
    for sid in pk.ops.get_fp4_solutions(D.h, m, n, k):
        by_kind.setdefault((sid >> 48) & 0xF, sid)
    assert len(by_kind) >= 3, by_kind
    mul = pk.mul_nvfp4_a16 if kind == "nv" else pk.mul_mxfp4_a16
    for sid in [-1] + list(by_kind.values())[:3]:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        poison = torch.full((m, n), POISON[is_bf16], dtype=torch.int16, device=DEV)
        del poison
        c = mul(D.a.view(dtype).reshape(m, k), D.b, D.sp, D.gs, m, n, k, sid, bias=D.bias.view(dtype))
        assert torch.equal(c.view(torch.int16).reshape(-1), D.want), f"{sid:#x} [{D.L.describe_solution(sid)}]"

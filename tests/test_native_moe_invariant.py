"""The batch-invariant MoE launch on the native class (include/petit_amd.h "Batch-invariant MoE launch on the native class") on the GPU: every
written row is the dense native-invariant entry's row on that row alone; neighbours, position, the expert's offset and the launch form do not
reach a row; both forms equal the definition (float64 through the stated epilogue, and the host twin) bit for bit on inputs whose quantisation
and partial sums are exact; the fold is the ascending one and the split form's slabs are the p_s; the write contract on poisoned, guarded,
caller-owned buffers; graph replay follows new offsets; the layer switch fp4_moe_native(invariant=True).
Shapes (n, k): (64, 1024): S = 4, L = 256; (64, 4352): S = 9, L = 512, last slice 256; (128, 256): S = 1; (96, 512): three pairs of n-tiles
(the whole form has a wave with one dead pair, the split form a ragged last workgroup); gated: (128, 1024) and (192, 512) (three gate pairs in
a four-slot workgroup).  E in {3, 65, 130}: the slot map crosses the 64-expert chunks of moe_locate."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from petit_kernel import _lib
from test_gated_contract import expect as gated_expect
from test_gpu_parity import DEV, decode_qact, pk  # noqa: F401
from test_moe_invariant import OFFSETS, _Guarded, _offsets, _same
from test_native_invariant import dev16, fold32, fold_problem, out_bits
from test_native_invariant_abi import BF16, FMTS, FP16, OK, dt, exact_activations, expect_plain, from16, geometry, host_quantize, to16
from test_native_moe_invariant_abi import CASES, EXPERTS, GATED_SHAPES, IDS, SHAPES, HostExperts, moe_twin, row_owner

pytestmark = pytest.mark.gpu
L = _lib.lib
A_ROWS = 8                                                                                # distinct activation rows of the equality test
SPECIAL = (70, 1, 32, 33, 64)                                                             # more than a whole-form tile; 1; a split-form tile, and a row; a whole-form tile


class Experts:
    """E experts' [n, k] weights quantised to MXFP4 on the device (the stacked packed tensors the MoE launch reads), one global scale and one
    bias row per expert, and expert e's own packed tensors as the dense entry takes them: byte ranges of the stacked ones."""

    def __init__(self, pk, dtype, E, n, k, seed):
        g = torch.Generator().manual_seed(seed)
        w = (torch.randn(E, n, k, generator=g) * 0.5).to(torch.bfloat16).to(DEV)
        self.b, self.s, _ = pk.quantize_mxfp4(w)
        self.gs = (torch.rand(E, generator=g) * 0.5 + 0.5).to(DEV)                        # distinct per expert
        self.bias = torch.randn(E, n, generator=g).to(dtype).to(DEV)
        self.E, self.n, self.k, self.wb, self.sb = E, n, k, n * k // 2, n * k // 32

    def expert(self, e):
        b = self.b.view(torch.uint8).reshape(-1)[e * self.wb:(e + 1) * self.wb]
        s = self.s.view(torch.uint8).reshape(-1)[e * self.sb:(e + 1) * self.sb]
        return b, s, self.gs[e:e + 1], self.bias[e]


@functools.lru_cache(maxsize=None)
def experts(E, n, k, is_bf16):
    import petit_kernel
    return Experts(petit_kernel, dt(is_bf16), E, n, k, 100 * E + n + k)


def m_of_form(pk, E, split, start):
    """The largest m <= start of the split form, or the smallest m >= start of the whole form."""
    m = start
    while pk.native_moe_invariant_form(m, E) != int(split):
        m += -1 if split else 1
        assert 0 < m < 1 << 16
    return m


def routings(pk, E, split):
    """Per-expert row counts on the wanted side of the form switch, found through the form query.  whole: one expert with more than 64 rows and
    one with exactly 1, 32, 33 and 64 (E = 3: over two routings), next to the 64-expert chunk boundaries of the slot map, the first and the
    last expert empty where E allows.  split: rows dealt one at a time to the experts next to the chunk boundaries while the query says split."""
    if not split:
        if E == 3:
            out = [[70, 0, 33], [1, 32, 64]]
        else:
            c = [0] * E
            for e, v in zip((1, 62, 63, 64, 66 if E > 66 else 3), SPECIAL):
                c[e] = v
            if E > 129:
                c[127], c[128] = 5, 7
            out = [c]
    else:
        c = [0] * E
        seats = list(dict.fromkeys(e for e in (1, 62, 64, 65, 128, E - 2) if 0 < e < E)) or [0]
        i = 0
        while pk.native_moe_invariant_form(sum(c) + 1, E) == 1 and sum(c) < 64:
            c[seats[i % len(seats)]] += 1
            i += 1
        out = [c]
    assert any(0 in c for c in out)                                                       # empty experts included
    for c in out:
        assert sum(c) > 0 and pk.native_moe_invariant_form(sum(c), E) == int(split), (E, split, c)
    return out


def layers():
    from petit_kernel import compiled, ops
    assert compiled.available(), compiled.why_unavailable()
    return {"ctypes": ops, "compiled": compiled}


# --- 1. every row is the dense entry's -------------------------------------------------------------------------------------------------------

EPILOGUES = ((False, None), (True, None), (True, "silu_mul"), (True, "swiglu_oai"))      # (bias, activation)


@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
@pytest.mark.parametrize("E", EXPERTS)
def test_every_row_equals_the_dense_native_invariant_entry_on_that_row(pk, E, fmt, is_bf16):
    """Grouped row r of expert e equals mul_mxfp4_native_invariant(size_m=1) on that row with expert e's tensors, gs[e] and bias[e]: both forms,
    plain / bias / silu_mul / swiglu_oai, with and without row indices, 16-bit and quantised input, both operator layers."""
    dtype = dt(is_bf16)
    shapes = [(n, k, (0, 1)) for n, k in (SHAPES if E == 3 else [SHAPES[0], SHAPES[3]])] + [(n, k, (2, 3)) for n, k in (GATED_SHAPES if E == 3 else GATED_SHAPES[1:])]
    lay = layers()
    g = torch.Generator().manual_seed(E)
    forms = set()
    for n, k, eis in shapes:
        X = experts(E, n, k, is_bf16)
        a = torch.randn(A_ROWS, k, generator=g).to(dtype).to(DEV)
        ref = {}

        def want_row(ei, e, ar):
            if (ei, e, ar) not in ref:
                use_bias, act = EPILOGUES[ei]
                b, s, gs, bias = X.expert(e)
                ref[(ei, e, ar)] = pk.mul_mxfp4_native_invariant(a[ar:ar + 1], b, s, gs, 1, n, k, fmt, bias if use_bias else None, act)[0]
            return ref[(ei, e, ar)]

        for split in (True, False):
            for counts in routings(pk, E, split):
                m = sum(counts)
                forms.add(pk.native_moe_invariant_form(m, E))
                owner = np.repeat(np.arange(E), counts)
                a_idx = torch.tensor([(5 * int(owner[r]) + 3 * r) % A_ROWS for r in range(m)], dtype=torch.int32)
                c_idx = torch.randperm(m, generator=g).to(torch.int32)
                grouped = a[a_idx.long().to(DEV)].contiguous()
                off = _offsets(counts)
                for ei in eis:
                    use_bias, act = EPILOGUES[ei]
                    kw = dict(fmt=fmt, bias=X.bias if use_bias else None, activation=act)
                    want = torch.stack([want_row(ei, int(owner[r]), int(a_idx[r])) for r in range(m)])
                    mul = lay[("ctypes", "compiled")[(ei + int(split)) % 2]].mul_mxfp4_native_moe_invariant
                    # 16-bit input gathered and scattered through the indices
                    out = mul(a, X.b, X.s, X.gs, off, m, n, k, E, a_row_index=a_idx.to(DEV), c_row_index=c_idx.to(DEV), **kw)
                    assert out.shape == (m, n // 2 if act else n) and out.dtype == dtype
                    assert _same(out[c_idx.long().to(DEV)], want), (E, n, k, split, ei, "indexed")
                    # 16-bit grouped rows, no index
                    assert _same(mul(grouped, X.b, X.s, X.gs, off, m, n, k, E, **kw), want), (E, n, k, split, ei, "plain")
                    # quantised grouped rows from the gathering quantiser
                    qa = pk.quantize_activation_rows(a, fmt, a_idx.to(DEV))
                    out = mul(qa, X.b, X.s, X.gs, off, m, n, k, E, c_row_index=c_idx.to(DEV), **kw)
                    assert _same(out[c_idx.long().to(DEV)], want), (E, n, k, split, ei, "quantised")
    assert forms == {0, 1}


# --- 2. neighbours and routing do not reach a row --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("activation", (None, "swiglu_oai"))
@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
def test_neighbours_and_routing_do_not_reach_a_row(pk, fmt, is_bf16, activation):
    """Three probe rows of expert 1 of 3: alone; among NaN / +-inf / huge rows of the same and of the neighbouring experts, at the first, the
    middle and the last position of the expert; with the expert's offset moved; in both forms."""
    E, n, k, e = 3, 128, 1024, 1
    X = experts(E, n, k, is_bf16)
    kw = dict(fmt=fmt, bias=X.bias, activation=activation)
    probes = to16(np.random.default_rng(41).standard_normal((3, k)), is_bf16, exact=False)
    alone = out_bits(pk.mul_mxfp4_native_moe_invariant(dev16(probes, is_bf16), X.b, X.s, X.gs, _offsets([0, 3, 0]), 3, n, k, E, **kw))
    assert not np.isnan(from16(alone, is_bf16)).any()
    big = 2.0 ** 120 if is_bf16 else 65504.0
    hostile = [np.nan, np.inf, -np.inf, big, -big, 0.0]
    forms = {pk.native_moe_invariant_form(3, E)}
    split_m = m_of_form(pk, E, True, 64)
    assert split_m >= 5
    for counts in ([1, split_m - 2, 1], [0, split_m - 1, 1], [20, 23, 20], [40, 70, 3], [64, 33, 0], [65, 3, 64]):
        m = sum(counts)
        forms.add(pk.native_moe_invariant_form(m, E))
        v = np.empty((m, k))
        for r in range(m):
            v[r] = hostile[r % len(hostile)]
        bits = to16(v, is_bf16, exact=False)
        lo, cnt = counts[0], counts[1]
        places = [lo, lo + cnt // 2, lo + cnt - 1]                                        # first / middle / last row of the expert
        for p, i in zip(places, range(3)):
            bits[p] = probes[i]
        got = out_bits(pk.mul_mxfp4_native_moe_invariant(dev16(bits, is_bf16), X.b, X.s, X.gs, _offsets(counts), m, n, k, E, **kw))
        for p, i in zip(places, range(3)):
            assert np.array_equal(got[p], alone[i]), (counts, p, i)
    assert forms == {0, 1}


# --- 3. the definition on exact inputs -------------------------------------------------------------------------------------------------------

def exact_case(pk, E, n, k, is_bf16, fmt, counts, gs, seed):
    X = HostExperts(E, n, k, is_bf16, seed, exact=True, gs=gs)
    m = sum(counts)
    a = exact_activations(m, k, seed)
    bits = to16(a, is_bf16)
    owner = np.repeat(np.arange(E), counts)
    fold = np.stack([a[r] @ X.w[owner[r]].T for r in range(m)])
    assert max((np.abs(a[r]) @ np.abs(X.w[owner[r]]).T).max() for r in range(m)) < 2 ** 22           # every partial sum is exact, in any order
    assert np.array_equal(fold.astype(np.float32).astype(np.float64), fold)
    qa_host = host_quantize(bits, is_bf16, fmt)
    assert np.array_equal(decode_qact(qa_host, m, k, fmt).astype(np.float64), a)                      # the quantiser is exact
    return X, m, a, bits, owner, fold, qa_host


@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
@pytest.mark.parametrize("n,k", SHAPES)
def test_both_forms_equal_the_definition_and_the_twin_on_exact_inputs(pk, n, k, fmt, is_bf16):
    """Quantiser exact, every partial sum exact: both forms equal expect_plain of the float64 fold of each row with its expert's weights, and the
    MoE twin, bit for bit.  Each expert meets gs 0.25, 1/3 and none in turn (the entry always multiplies by gs[e]: "none" is gs[e] = 1.0, which
    changes no bit, and the expectation then skips the multiply), with and without a bias."""
    E = 3
    forms = set()
    for split in (True, False):
        counts = [1, m_of_form(pk, E, True, 64) - 1, 0] if split else [2, 0, m_of_form(pk, E, False, 66) - 2]
        for gs in ([0.25, 1.0 / 3.0, 1.0], [1.0 / 3.0, 1.0, 0.25], [1.0, 0.25, 1.0 / 3.0]):       # (1.0: the multiply changes nothing -- "none")
            X, m, a, bits, owner, fold, qa_host = exact_case(pk, E, n, k, is_bf16, fmt, counts, gs, 3)
            forms.add(pk.native_moe_invariant_form(m, E))
            b, s, gsd, biasd = X.b.to(DEV), X.s.to(DEV), torch.from_numpy(X.gs).to(DEV), dev16(X.bias_bits, is_bf16)
            for use_bias in (True, False):
                got = out_bits(pk.mul_mxfp4_native_moe_invariant(dev16(bits, is_bf16), b, s, gsd, _offsets(counts), m, n, k, E, fmt=fmt,
                                                                 bias=biasd if use_bias else None))
                want = np.stack([expect_plain(fold[r:r + 1].astype(np.float32), None if X.gs[owner[r]] == 1.0 else float(X.gs[owner[r]]),
                                              X.bias64[owner[r]] if use_bias else None, is_bf16)[0] for r in range(m)])
                assert np.array_equal(got, want), (split, gs, use_bias, int((got != want).sum()))
                tw = moe_twin(qa_host, X, np.concatenate([[0], np.cumsum(counts)]), m, None, m, fmt, use_bias)
                assert np.array_equal(got, tw), (split, gs, use_bias)
    assert forms == {0, 1}


@pytest.mark.parametrize("act,name", [(1, "silu_mul"), (2, "swiglu_oai")])
@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
@pytest.mark.parametrize("n,k", GATED_SHAPES)
def test_gated_epilogues_on_exact_inputs(pk, n, k, fmt, is_bf16, act, name):
    """y = fma(fold, gs[e], bias[e]) with an exact fold, through the gated epilogue every gated kernel calls: held to the gated contract's band
    (tests/test_gated_contract.py), and the two forms to each other bit for bit on the rows they share."""
    E, gs = 3, [2.0 ** -7, 2.0 ** -6, 2.0 ** -7]                                          # (gate values of a few units)
    per_form = {}
    for split in (True, False):
        rows = m_of_form(pk, E, True, 64) - 1
        counts = [1, rows, 0] if split else [1, 70, 2]
        X, m, a, bits, owner, fold, _ = exact_case(pk, E, n, k, is_bf16, fmt, counts, gs, 9)
        X.bias64 = X.bias64 * 0.25
        X.bias_bits = to16(X.bias64, is_bf16)
        y = np.stack([fold[r] * float(X.gs[owner[r]]) + X.bias64[owner[r]] for r in range(m)]).astype(np.float32).astype(np.float64)   # one rounding: the fma
        P = gated_expect(types.SimpleNamespace(y=y), is_bf16, act)
        got = out_bits(pk.mul_mxfp4_native_moe_invariant(dev16(bits, is_bf16), X.b.to(DEV), X.s.to(DEV), torch.from_numpy(X.gs).to(DEV),
                                                         _offsets(counts), m, n, k, E, fmt=fmt, bias=dev16(X.bias_bits, is_bf16), activation=name))
        assert got.shape == (m, n // 2)
        assert not P.wrong(got).any(), (split, int(P.wrong(got).sum()))
        per_form[split] = got[1:1 + rows]                                                 # exact_activations(m, ...)'s rows differ with m: compare through one call below
    # the same rows of expert 1 in both forms: the split routing's rows placed first in the whole routing's expert 1
    rows = m_of_form(pk, E, True, 64) - 1
    X, m, a, bits, owner, fold, _ = exact_case(pk, E, n, k, is_bf16, fmt, [1, rows, 0], gs, 9)
    big_counts = [1, 70, 2]
    mb = sum(big_counts)
    more = to16(exact_activations(mb, k, 10), is_bf16)
    more[1:1 + rows] = bits[1:1 + rows]
    kw = dict(fmt=fmt, bias=dev16(to16(X.bias64 * 0.25, is_bf16), is_bf16), activation=name)
    args = (X.b.to(DEV), X.s.to(DEV), torch.from_numpy(X.gs).to(DEV))
    small = out_bits(pk.mul_mxfp4_native_moe_invariant(dev16(bits, is_bf16), *args, _offsets([1, rows, 0]), m, n, k, E, **kw))
    large = out_bits(pk.mul_mxfp4_native_moe_invariant(dev16(more, is_bf16), *args, _offsets(big_counts), mb, n, k, E, **kw))
    assert np.array_equal(small[1:1 + rows], large[1:1 + rows]) and np.array_equal(small[1:1 + rows], per_form[True])


# --- 4. fold order ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
@pytest.mark.parametrize("n,k", SHAPES[:2])
def test_the_fold_is_ascending_and_the_slabs_are_the_partial_sums(pk, n, k, fmt, is_bf16):
    """test_native_invariant.py's fold_problem on expert 1 of a 3-expert routing in the split form, through the C ABI on quantised bytes; the
    slabs are read back from the caller-owned workspace."""
    E = 3
    S, Lk = geometry(n, k)
    a_type = BF16 if is_bf16 else FP16
    m = m_of_form(pk, E, True, 64)
    assert m >= 3
    counts = [1, m - 2, 1]
    rows = m - 2
    bh, sh, a, parts = fold_problem(n, k, rows, is_bf16)
    want = expect_plain(fold32(parts, list(range(S))), None, None, is_bf16)
    others = expect_plain(fold32(parts, list(range(S))[::-1]), None, None, is_bf16)
    assert (want != others).mean() > 0.25                                                  # the inputs tell the orders apart
    X = HostExperts(E, n, k, is_bf16, 5, gs=[0.5, 1.0, 0.5])
    wb, sb = n * k // 2, n * k // 32
    X.b[wb:2 * wb] = bh.contiguous().view(torch.uint8).reshape(-1)
    X.s[sb:2 * sb] = sh.contiguous().view(torch.uint8).reshape(-1)
    bits = np.concatenate([to16(a[:1], is_bf16), to16(a, is_bf16), to16(a[-1:], is_bf16)])
    qa = pk.quantize_activation_rows(dev16(bits, is_bf16), fmt)
    nbytes = int(L.petit_gemm_native_moe_invariant_workspace_bytes(E, m, n, k, a_type, FMTS[fmt], 1))
    assert nbytes == (S * m * n * 4 + 255) // 256 * 256
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    c = torch.empty(m, n, dtype=dt(is_bf16), device=DEV)
    hints = _lib.SolutionHints(a_type, _lib.CXX_DTYPE_MXFP4_E2M1, a_type, 0)
    b, s, gsd, off = X.b.to(DEV), X.s.to(DEV), torch.from_numpy(X.gs).to(DEV), _offsets(counts)
    rc = L.petit_gemm_mxfp4_native_moe_invariant(c.data_ptr(), qa.data.data_ptr(), b.data_ptr(), s.data_ptr(), gsd.data_ptr(), off.data_ptr(), E, m, n,
                                                 k, None, m, None, m, C.byref(hints), FMTS[fmt], 1, None, ws.data_ptr(), None)
    assert rc == OK
    torch.cuda.synchronize()
    slabs = ws[: S * m * n * 4].view(torch.float32).reshape(S, m, n).cpu().numpy()
    for sl in range(S):
        assert np.array_equal(slabs[sl, 1:1 + rows].astype(np.float64), parts[sl]), sl
    assert np.array_equal(out_bits(c)[1:1 + rows], want)
    assert np.array_equal(out_bits(pk.mul_mxfp4_native_moe_invariant(dev16(bits, is_bf16), b, s, gsd, off, m, n, k, E, fmt=fmt))[1:1 + rows], want)


# --- 5. the write contract, through the C ABI ------------------------------------------------------------------------------------------------

def abi_call(X, dtype, fmt, a, quantized, offsets, m, a_idx, a_rows, c_idx, c_rows, c, ws):
    from petit_kernel import ops
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    hints = ops._hints("mx", dtype)
    epi = _lib.Epilogue(X.bias.data_ptr(), 0, 0)
    rc = L.petit_gemm_mxfp4_native_moe_invariant(c.ptr, ptr(a), ptr(X.b), ptr(X.s), ptr(X.gs), ptr(offsets), X.E, m, X.n, X.k, ptr(a_idx), a_rows,
                                                 ptr(c_idx), c_rows, C.byref(hints), FMTS[fmt], quantized, C.byref(epi), ws.ptr,
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == OK


@pytest.mark.parametrize("form", ("split", "whole"))
@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
def test_write_contract_on_poisoned_guarded_buffers(pk, fmt, is_bf16, form):
    """E = 4, every offsets kind, 16-bit input through an A index with out-of-range entries (a zero row: round16(bias)) and quantised input:
    every row some expert owns is written with the dense entry's bits, nothing else is; a C index out of range is skipped; nothing lands
    outside c or past the queried workspace bytes."""
    from petit_kernel import ops
    dtype = dt(is_bf16)
    E, n, k = 4, 96, 512
    split = form == "split"
    m = m_of_form(pk, E, split, 64 if split else 150)
    assert m >= 8 and (pk.native_moe_invariant_form(m, E) == 1) == split
    X = experts(E, n, k, is_bf16)
    g = torch.Generator().manual_seed(m)
    a_rows, c_rows = max(m // 2, 4), m + 5
    a = torch.randn(a_rows, k, generator=g).to(dtype).to(DEV)
    a_idx = torch.randint(0, a_rows, (m,), generator=g).to(torch.int32)
    a_idx[3::11] = a_rows                                                                 # outside [0, a_rows): a zero row
    a_idx[5::13] = -1
    c_idx = torch.randperm(c_rows, generator=g)[:m].to(torch.int32)
    c_idx[2::9] = c_rows + 1                                                              # outside [0, c_rows): skipped
    c_idx[4::17] = -3
    zero = torch.zeros(1, k, dtype=dtype, device=DEV)
    grouped = torch.cat([a[int(i)][None] if 0 <= int(i) < a_rows else zero for i in a_idx])
    for quantized in (0, 1):
        need = ops.native_moe_invariant_workspace_bytes(E, m, n, k, dtype, fmt, bool(quantized))
        assert need % 256 == 0 and (need > 0) == (split or not quantized)
        src = pk.quantize_activation_rows(a, fmt, a_idx.to(DEV)).data if quantized else a
        for name, fractions in OFFSETS.items():
            offsets = np.array([int(round(f * m)) for f in fractions], dtype=np.int32)
            owner = row_owner(offsets, m)
            assert (owner >= 0).sum() > m // 2
            c, ws = _Guarded(c_rows * n // 2), _Guarded(max(need // 4, 64))
            assert ws.ptr.value % 256 == 0 and c.ptr.value % 16 == 0
            abi_call(X, dtype, fmt, src, quantized, torch.from_numpy(offsets).to(DEV), m, None if quantized else a_idx.to(DEV), a_rows,
                     c_idx.to(DEV), c_rows, c, ws)
            assert c.guards_intact() and ws.guards_intact(), name
            if not need:
                assert bool((ws.inside() == ws.POISON).all()), "a call without workspace wrote it"
            elif need // 4 < ws.count:
                assert bool((ws.inside()[need // 4:] == ws.POISON).all())
            got = c.inside().view(dtype).reshape(c_rows, n)
            want = torch.full((c_rows, n // 2), _Guarded.POISON, dtype=torch.int32, device=DEV).view(dtype).reshape(c_rows, n).clone()
            for e in range(E):
                rows = [r for r in range(m) if owner[r] == e]
                if not rows:
                    continue
                b, s, gs, bias = X.expert(e)
                y = pk.mul_mxfp4_native_invariant(grouped[rows].contiguous(), b, s, gs, len(rows), n, k, fmt, bias)
                for i, r in enumerate(rows):
                    if not 0 <= int(a_idx[r]) < a_rows:
                        assert _same(y[i], bias), "an A index out of range must give round16(bias)"
                    if 0 <= int(c_idx[r]) < c_rows:
                        want[int(c_idx[r])] = y[i]
            assert _same(got, want), (form, quantized, name)                              # written rows: the dense bits; all others: the poison


@pytest.mark.parametrize("form", ("split", "whole"))
@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
def test_all_rows_on_one_expert_of_130_equal_the_dense_call(pk, fmt, is_bf16, form):
    """The largest split-form m up to 64, and 300 rows (5 m-tiles of the whole form) on expert 77 of 130."""
    E, k, e = 130, 512, 77
    m = m_of_form(pk, E, form == "split", 64 if form == "split" else 300)
    a = torch.randn(m, k, generator=torch.Generator().manual_seed(m)).to(dt(is_bf16)).to(DEV)
    counts = [0] * E
    counts[e] = m
    for act, n in ((None, 96), ("silu_mul", 192)):
        X = experts(E, n, k, is_bf16)
        out = pk.mul_mxfp4_native_moe_invariant(a, X.b, X.s, X.gs, _offsets(counts), m, n, k, E, fmt=fmt, bias=X.bias, activation=act)
        b, s, gs, bias = X.expert(e)
        assert _same(out, pk.mul_mxfp4_native_invariant(a, b, s, gs, m, n, k, fmt, bias, act)), (m, act)


# --- 6. graph capture ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
def test_graph_capture_replays_and_follows_new_offsets_and_index(pk, fmt, is_bf16):
    dtype = dt(is_bf16)
    E, n, k = 8, 192, 512
    X = experts(E, n, k, is_bf16)
    mul = pk.mul_mxfp4_native_moe_invariant
    g = torch.Generator().manual_seed(1)
    forms = set()
    small = m_of_form(pk, E, True, 64)
    for counts, counts2 in (([1] * (small - 1) + [0] * (E - small + 1) if small <= E else [small - 7, 1, 1, 1, 1, 1, 1, 1],
                             [0, small - 1] + [0] * (E - 2)),
                            ([65, 64, 0, 33, 32, 65, 1, 64], [100, 0, 90, 7, 0, 67, 40, 20])):
        m, m2 = sum(counts), sum(counts2)
        assert m2 <= m
        forms.add(pk.native_moe_invariant_form(m, E))
        pool, pool2 = (torch.randn(m + 3, k, generator=g).to(dtype).to(DEV) for _ in range(2))
        a_idx, a_idx2 = (torch.randint(0, m + 3, (m,), generator=g).to(torch.int32).to(DEV) for _ in range(2))
        c_idx, c_idx2 = (torch.randperm(m, generator=g).to(torch.int32).to(DEV) for _ in range(2))
        off = _offsets(counts)
        kw = dict(fmt=fmt, bias=X.bias, activation="silu_mul")
        eager = mul(pool, X.b, X.s, X.gs, off, m, n, k, E, a_row_index=a_idx, c_row_index=c_idx, **kw)
        for _ in range(3):                                                                # repeated launches are identical
            assert _same(mul(pool, X.b, X.s, X.gs, off, m, n, k, E, a_row_index=a_idx, c_row_index=c_idx, **kw), eager)
        eager2 = mul(pool2, X.b, X.s, X.gs, _offsets(counts2), m, n, k, E, a_row_index=a_idx2, c_row_index=c_idx2, **kw)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = mul(pool, X.b, X.s, X.gs, off, m, n, k, E, a_row_index=a_idx, c_row_index=c_idx, **kw)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same(out, eager), m
        off.copy_(_offsets(counts2))                                                      # in place: the replay reads the new routing
        pool.copy_(pool2)
        a_idx.copy_(a_idx2)
        c_idx.copy_(c_idx2)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        written = c_idx2[:m2].long()                                                      # (rows of no expert keep the zeros)
        assert _same(out[written], eager2[written]) and not _same(eager[written], eager2[written]), m
        rest = c_idx2[m2:].long()
        assert bool((out[rest].view(torch.int16) == 0).all())
    assert forms == {0, 1}


# --- 7. the layer ----------------------------------------------------------------------------------------------------------------------------

def synth_gptoss(E, H, I, seed):
    """The six expert tensors of one MoE block as a gpt-oss checkpoint stores them, from random codes, scales and biases."""
    rng = np.random.default_rng(seed)
    t = torch.from_numpy
    return dict(gate_up_blocks=t(rng.integers(0, 256, (E, 2 * I, H // 32, 16), dtype=np.uint8)),
                gate_up_scales=t(rng.integers(120, 124, (E, 2 * I, H // 32), dtype=np.uint8)),
                gate_up_bias=t(rng.standard_normal((E, 2 * I)).astype(np.float32) * 0.5).bfloat16(),
                down_blocks=t(rng.integers(0, 256, (E, H, I // 32, 16), dtype=np.uint8)),
                down_scales=t(rng.integers(120, 124, (E, H, I // 32), dtype=np.uint8)),
                down_bias=t(rng.standard_normal((E, H)).astype(np.float32) * 0.5).bfloat16())


@pytest.fixture(scope="module")
def layer_weights(pk):
    """H = 256, I = 256, 8 experts, top-2: a randomly quantised MXFP4 layer and a gpt-oss block (biases, swiglu_oai) through prepare_gptoss_experts."""
    H, I, E = 256, 256, 8
    g = torch.Generator().manual_seed(2025)
    w13 = (torch.randn(E, 2 * I, H, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
    w2 = (torch.randn(E, H, I, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
    ex = pk.prepare_gptoss_experts(**{k: v.to(DEV) for k, v in synth_gptoss(E, H, I, 7).items()})
    logits = torch.randn(300, E, generator=g)
    topk_w, topk_ids = torch.topk(torch.softmax(logits, dim=1), 2, dim=1)
    return {"plain": (pk.quantize_mxfp4(w13) + pk.quantize_mxfp4(w2), dict(activation="silu_mul")),
            "gptoss": ((ex.w13, ex.s13, ex.gs13, ex.w2, ex.s2, ex.gs2), dict(bias13=ex.bias13, bias2=ex.bias2, activation="swiglu_oai")), "experts": ex,
            "hidden": torch.randn(300, H, generator=g).to(torch.bfloat16).to(DEV), "norm": (torch.rand(H, generator=g) + 0.5).to(torch.bfloat16).to(DEV),
            "w": topk_w.contiguous().to(DEV), "ids": topk_ids.to(torch.int32).contiguous().to(DEV)}


@pytest.mark.parametrize("variant", ("plain", "norm", "gptoss"))
@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
def test_a_tokens_layer_output_is_the_same_in_any_batch(pk, layer_weights, variant, fmt, is_bf16):
    """fp4_moe_native(..., invariant=True): a token's output row -- with norm_weight both returned rows -- is identical on T = 37 tokens, on
    each of three of them alone, in a T = 3 batch that holds them at other positions, and in a T = 300 batch; the launches run in both forms."""
    dtype = dt(is_bf16)
    wts, kw = layer_weights["gptoss" if variant == "gptoss" else "plain"]
    kw = {key: (v.to(dtype) if torch.is_tensor(v) else v) for key, v in kw.items()}
    if variant == "norm":
        kw["norm_weight"] = layer_weights["norm"].to(dtype)
    hidden, w, ids = layer_weights["hidden"].to(dtype), layer_weights["w"], layer_weights["ids"]
    E, topk, tokens = 8, 2, (0, 18, 36)
    assert {pk.native_moe_invariant_form(T * topk, E) for T in (1, 3, 37, 300)} == {0, 1}

    def run(x, rows):
        out = pk.fp4_moe_native(x.contiguous(), *wts, w[rows].contiguous(), ids[rows].contiguous(), "mxfp4", fmt, invariant=True, **kw)
        return out if isinstance(out, tuple) else (out,)

    every = torch.arange(300, device=DEV)
    full = run(hidden[:37], every[:37])
    assert len(full) == (2 if variant == "norm" else 1) and all(t.shape == (37, 256) for t in full)
    three = torch.tensor([36, 0, 18], device=DEV)                                         # the three tokens alone together, at other positions
    out3 = run(hidden[three], three)
    order = every.clone()                                                                 # T = 300; tokens 0 / 18 / 36 moved to 250 / 7 / 299
    moved = {0: 250, 18: 7, 36: 299}
    for t, p in moved.items():
        order[p] = t
    out300 = run(hidden[order], order)
    for t in tokens:
        one = torch.tensor([t], device=DEV)
        alone = run(hidden[one], one)
        for i in range(len(full)):
            assert _same(alone[i][0], full[i][t]), (variant, t, i, "alone")
            assert _same(out3[i][[36, 0, 18].index(t)], full[i][t]), (variant, t, i, "T = 3")
            assert _same(out300[i][moved[t]], full[i][t]), (variant, t, i, "T = 300")
    # the default native layer is free to move with the batch: computed, compared, not asserted equal
    loose = pk.fp4_moe_native(hidden[:37].contiguous(), *wts, w[:37].contiguous(), ids[:37].contiguous(), "mxfp4", fmt, **kw)
    loose = loose if isinstance(loose, tuple) else (loose,)
    assert loose[0].shape == full[0].shape


@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
def test_the_layer_is_the_chain_built_by_hand(pk, layer_weights, fmt, is_bf16):
    """moe_align_device, quantize_activation_rows, the two batch-invariant launches (gate_up on the quantised grouped rows, down scattered
    through sorted_pos), moe_combine -- and the gpt-oss block's forward(..., path='native', invariant=True) is that layer."""
    dtype = dt(is_bf16)
    T, H, I, E, topk = 37, 256, 256, 8, 2
    x, w, ids = layer_weights["hidden"][:T].to(dtype).contiguous(), layer_weights["w"][:T].contiguous(), layer_weights["ids"][:T].contiguous()
    for variant in ("plain", "gptoss"):
        (b13, s13, gs13, b2, s2, gs2), kw = layer_weights[variant]
        kw = {key: (v.to(dtype) if torch.is_tensor(v) else v) for key, v in kw.items()}
        got = pk.fp4_moe_native(x, b13, s13, gs13, b2, s2, gs2, w, ids, "mxfp4", fmt, invariant=True, **kw)
        sorted_pos, offsets, token_index = pk.moe_align_device(ids, E)
        m = T * topk
        qa = pk.quantize_activation_rows(x, fmt, token_index)
        h = pk.mul_mxfp4_native_moe_invariant(qa, b13, s13, gs13, offsets, m, 2 * I, H, E, fmt=fmt, bias=kw.get("bias13"), activation=kw["activation"])
        assert h.shape == (m, I) and h.dtype == dtype
        y = pk.mul_mxfp4_native_moe_invariant(h, b2, s2, gs2, offsets, m, H, I, E, c_row_index=sorted_pos, c_rows=m, fmt=fmt, bias=kw.get("bias2"))
        assert _same(got, pk.moe_combine(y, w, ids, E)), variant
    if is_bf16:
        ex = layer_weights["experts"]
        assert _same(ex.forward(x, w, ids, path="native", activations=fmt, invariant=True), got)

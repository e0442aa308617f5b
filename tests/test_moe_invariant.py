"""The batch-invariant MoE launch (include/petit_amd.h "Batch-invariant MoE launch") and the batch-invariant MoE layer on the GPU.

The reference bits are the dense batch-invariant entry's: every grouped row is compared, with torch.equal on the bits, with
mul_*_a16_invariant(size_m=1) on its A row and its expert's tensors -- no tolerance anywhere in this module.  Shapes are the smallest that reach
every path: expert counts that cross the slot map's chunks of 64, per-expert row counts on the tile edges (16 and 64), an N of one n-block
and a ragged one, K of two slices, three, and nine with a short last one, and both sides of the form switch.  Which side a batch falls on is
read from moe_invariant_form, never assumed: the whole form takes the full set of row counts, the split form the counts of that set the
switch admits (it serves a decode step's few rows: profiles/moe_invariant.md)."""
import ctypes as C

import numpy as np
import pytest
import torch

DEV = "cuda"
PAIRS = {"bf16-nv": (torch.bfloat16, "nv"), "bf16-mx": (torch.bfloat16, "mx"), "f16-nv": (torch.float16, "nv")}
EPILOGUES = ((False, None), (True, None), (True, "silu_mul"), (True, "swiglu_oai"))      # (bias, activation)
COUNT_SET = (0, 1, 15, 16, 17, 63, 64, 65)
A_ROWS = 8                                                                                # distinct activation rows of the equality test


@pytest.fixture(scope="module")
def pk():
    import petit_kernel
    assert torch.cuda.is_available()
    assert torch.cuda.get_device_properties(0).gcnArchName.startswith("gfx950")
    return petit_kernel


def _layers():
    from petit_kernel import compiled, ops
    assert compiled.available(), compiled.why_unavailable()
    return {"ctypes": ops, "compiled": compiled}


def _moe(layer, kind):
    return layer.mul_nvfp4_a16_moe_invariant if kind == "nv" else layer.mul_mxfp4_a16_moe_invariant


def _dense(pk, kind):
    return pk.mul_nvfp4_a16_invariant if kind == "nv" else pk.mul_mxfp4_a16_invariant


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


class _Experts:
    """E experts' [n, k] weights quantised on the device (the stacked packed tensors the MoE launches read), one global scale and one bias row
    per expert, and expert e's own packed tensors as the dense entry takes them: byte ranges of the stacked ones."""

    def __init__(self, pk, kind, dtype, E, n, k, seed):
        g = torch.Generator().manual_seed(seed)
        w = (torch.randn(E, n, k, generator=g) * 0.5).to(dtype).to(DEV)
        self.b, self.s, self.gs = pk.quantize_nvfp4(w) if kind == "nv" else pk.quantize_mxfp4(w)
        if kind == "mx":
            self.gs = (torch.rand(E, generator=g) * 0.5 + 0.5).to(DEV)                    # (MXFP4 has none of its own: any float32 [E] does)
        self.bias = torch.randn(E, n, generator=g).to(dtype).to(DEV)
        self.kind, self.E, self.n, self.k = kind, E, n, k
        self.wb, self.sb = n * k // 2, n * k // (16 if kind == "nv" else 32)

    def expert(self, e):
        b = self.b.view(torch.uint8).reshape(-1)[e * self.wb:(e + 1) * self.wb]
        s = self.s.view(torch.uint8).reshape(-1)[e * self.sb:(e + 1) * self.sb]
        return b, s, self.gs[e:e + 1], self.bias[e]


def _offsets(counts):
    return torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=DEV)


def _counts(pk, E, split):
    """Per-expert row counts from COUNT_SET on the wanted side of the form switch, empty experts at the chunk boundaries of the slot map.
    whole: the set in a cycle, small counts raised inside the set until the switch says whole.  split: every other expert empty; the experts
    next to the chunk boundaries first, each gets the largest count of the set that keeps the batch in the split form."""
    if split:
        c = [0] * E
        first = [e for e in (0, 62, 65, 126, 129, E - 1) if e < E]
        for e in dict.fromkeys(first + list(range(2, E, 2))):
            fits = [v for v in sorted(COUNT_SET, reverse=True) if v and pk.moe_invariant_form(sum(c) + v, E) == 1]
            if not fits:
                break
            c[e] = fits[0]
    else:
        base = (17, 0, 65, 16, 1, 64, 15, 63)
        c = [base[e % 8] for e in range(E)]
        for e in (63, 64, 127, 128):
            if e < E:
                c[e] = 0
        grow, e, i = (65, 64, 63), 0, 0
        while pk.moe_invariant_form(sum(c), E) != 0:
            assert e < E, "no counts of COUNT_SET reach the whole form"
            if c[e] in (17, 16, 15, 1):
                c[e], i = grow[i % 3], i + 1
            e += 1
    assert set(c) <= set(COUNT_SET) and 0 in c and sum(c) > 0 and pk.moe_invariant_form(sum(c), E) == int(split)
    return c


# --- 1. bit equality with the dense invariant entry ------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("E", (3, 65, 130))
@pytest.mark.parametrize("pair", list(PAIRS))
def test_every_row_equals_the_dense_invariant_entry_on_that_row(pk, pair, E):
    """Grouped row r of expert e, reading A row a_row_index[r] and written to c_row_index[r], equals mul_*_a16_invariant(size_m=1) on that A row
    with expert e's tensors, global scale and bias: both forms, plain / bias / silu_mul / swiglu_oai, both operator layers."""
    from petit_kernel import ops
    dtype, kind = PAIRS[pair]
    every = (0, 1, 2, 3)
    # (a gated call needs n % 32 == 0: NVFP4's ragged n-block is 208 for the plain epilogues and 224, MXFP4's, for the gated ones)
    wide = [(224, every)] if kind == "mx" else [(208, (0, 1)), (224, (2, 3))]
    shapes = [(32, 512, 2, every)] + [(n, 768, 3, eis) for n, eis in wide]
    if E == 3:
        shapes += [(32, 768, 3, every), (32, 4352, 9, every)] + [(n, 512, 2, eis) for n, eis in wide]
    layers = _layers()
    dense = _dense(pk, kind)
    g = torch.Generator().manual_seed(E)
    for n, k, want_S, eis in shapes:
        S, L = ops.invariant_geometry(n, k, dtype, kind)
        assert S == want_S and (k != 4352 or k % L != 0)                                  # 4352: a short last slice
        X = _Experts(pk, kind, dtype, E, n, k, 100 * E + n + k)
        a = torch.randn(A_ROWS, k, generator=g).to(dtype).to(DEV)
        ref = {}                                                                          # (epilogue, expert, A row) -> the dense entry's row

        def want_row(ei, e, ar):
            key = (ei, e, ar)
            if key not in ref:
                use_bias, act = EPILOGUES[ei]
                b, s, gs, bias = X.expert(e)
                ref[key] = dense(a[ar:ar + 1], b, s, gs, 1, n, k, bias if use_bias else None, act)[0]
            return ref[key]

        for split in (True, False):
            counts = _counts(pk, E, split)
            m = sum(counts)
            assert pk.moe_invariant_form(m, E) == int(split)
            owner = np.repeat(np.arange(E), counts)
            a_idx = torch.tensor([(5 * int(owner[r]) + 3 * r) % A_ROWS for r in range(m)], dtype=torch.int32)
            c_idx = torch.randperm(m, generator=g).to(torch.int32)
            for ei in eis:
                use_bias, act = EPILOGUES[ei]
                name = ("ctypes", "compiled")[(ei + int(split)) % 2]                      # every epilogue x form through one layer, both layers used
                out = _moe(layers[name], kind)(a, X.b, X.s, X.gs, _offsets(counts), m, n, k, E, a_row_index=a_idx.to(DEV),
                                               c_row_index=c_idx.to(DEV), bias=X.bias if use_bias else None, activation=act)
                assert out.shape == (m, n // 2 if act else n) and out.dtype == dtype
                want = torch.stack([want_row(ei, int(owner[r]), int(a_idx[r])) for r in range(m)])
                assert _same(out[c_idx.long().to(DEV)], want), (pair, E, n, k, split, use_bias, act, name)


# --- 2. a row's bits do not depend on its neighbours -----------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("activation", (None, "silu_mul", "swiglu_oai"))
@pytest.mark.parametrize("pair", list(PAIRS))
def test_a_rows_bits_do_not_depend_on_its_neighbours(pk, pair, activation):
    """The same A row on the same expert: alone (m = 1), in the middle of a full batch with the other experts busy, and at another grouped
    position -- through a different a_row_index and a c_row_index permutation -- of a batch of the other form."""
    dtype, kind = PAIRS[pair]
    E, n, k, e = 8, 208 if kind == "nv" and not activation else 224, 768, 5      # (gated: n % 32 == 0)
    X = _Experts(pk, kind, dtype, E, n, k, 77)
    mul = _moe(pk, kind)
    g = torch.Generator().manual_seed(5)
    row = torch.randn(1, k, generator=g).to(dtype).to(DEV)
    act = {"activation": activation, "bias": X.bias}
    ones = [0] * E
    ones[e] = 1
    forms = {pk.moe_invariant_form(1, E)}
    alone = mul(row, X.b, X.s, X.gs, _offsets(ones), 1, n, k, E, **act)[0]
    for counts in ([1] * E, [17] * E, [65] * E):                                          # every expert busy: a decode step, a tile and a row, a whole-form tile and a row
        m = sum(counts)
        forms.add(pk.moe_invariant_form(m, E))
        a = torch.randn(m, k, generator=g).to(dtype).to(DEV)
        r = sum(counts[:e]) + counts[e] // 2                                              # the middle of expert e's rows
        a[r] = row[0]
        full = mul(a, X.b, X.s, X.gs, _offsets(counts), m, n, k, E, **act)
        assert _same(full[r], alone), (pair, activation, m)
    for counts in ([1, 0, 2, 0, 1, 3, 0, 1], [16] * E, [64, 65, 63, 64, 1, 64, 65, 64]):  # other positions, through both forms again
        m = sum(counts)
        forms.add(pk.moe_invariant_form(m, E))
        pool = torch.randn(m + 3, k, generator=g).to(dtype).to(DEV)
        pool[m + 1] = row[0]
        r = sum(counts[:e]) + counts[e] - 1                                               # the last of expert e's rows
        a_idx = torch.randperm(m, generator=g).to(torch.int32)
        a_idx[r] = m + 1
        c_idx = torch.randperm(m, generator=g).to(torch.int32)
        out = mul(pool, X.b, X.s, X.gs, _offsets(counts), m, n, k, E, a_row_index=a_idx.to(DEV), c_row_index=c_idx.to(DEV), **act)
        assert _same(out[int(c_idx[r])], alone), (pair, activation, m)
    assert forms == {0, 1}                                                                # the row met both forms


# --- 3. the write contract, through the C ABI ------------------------------------------------------------------------------------------------

class _Guarded:
    """A caller buffer of `count` 4-byte elements between two guard zones, everything poisoned."""
    GUARD = 1024
    POISON = 0x7FC5FFC5  # (a NaN as float32, two NaNs as bf16 / fp16: no output is one)

    def __init__(self, count):
        self.count = count
        self.buf = torch.full((count + 2 * self.GUARD,), self.POISON, dtype=torch.int32, device=DEV)

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + 4 * self.GUARD)

    def inside(self):
        return self.buf[self.GUARD:self.GUARD + self.count]

    def guards_intact(self):
        g = self.GUARD
        return bool((self.buf[:g] == self.POISON).all()) and bool((self.buf[g + self.count:] == self.POISON).all())


def row_ownership(offsets, m):
    """owner[r] = the expert whose clamped range holds grouped row r, or -1: each offset clamped into [its predecessor, m] (a running maximum)."""
    hi = np.minimum(np.maximum.accumulate(np.clip(np.asarray(offsets, dtype=np.int64), 0, None)), m)
    owner = np.searchsorted(hi[1:], np.arange(m), side="right")
    return np.where((np.arange(m) >= hi[0]) & (owner < len(hi) - 1), owner, -1)


def _abi_call(kind, dtype, X, a, offsets, m, a_idx, c_idx, c_rows, use_bias, act, c, ws):
    from petit_kernel import _lib, ops
    fn = _lib.lib.petit_gemm_fp4_fp16_moe_invariant if kind == "nv" else _lib.lib.petit_gemm_mxfp4_fp16_moe_invariant
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    hints = ops._hints(kind, dtype)
    epi = _lib.Epilogue(X.bias.data_ptr() if use_bias else None, ops._ACTIVATIONS[act], 0)
    rc = fn(c.ptr, ptr(a), ptr(X.b), ptr(X.s), ptr(X.gs), ptr(offsets), X.E, m, X.n, X.k, ptr(a_idx), a.shape[0], ptr(c_idx), c_rows,
            C.byref(hints), C.byref(epi), ws.ptr, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == _lib.PETIT_OK
    return rc


OFFSETS = {   # (as fractions of m, scaled in the test) E = 4
    "well formed": (0, 0.3, 0.3, 0.7, 1),
    "rows before the first and after the last": (0.1, 0.3, 0.5, 0.5, 0.93),
    "descending": (0, 0.6, 0.2, 0.8, 1),
    "negative": (-0.05, 0.4, -0.01, 0.9, 1),
    "beyond m": (0.1, 0.5, 10, 0.7, 2),
}


@pytest.mark.gpu
def _m_of_form(pk, E, split, start):
    """The largest m <= start of the split form, or the smallest m >= start of the whole form."""
    m = start
    while pk.moe_invariant_form(m, E) != int(split):
        m += -1 if split else 1
        assert 0 < m < 1 << 16
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("split", "whole"))
@pytest.mark.parametrize("pair", list(PAIRS))
def test_write_contract_on_poisoned_guarded_buffers(pk, pair, form):
    """E = 4, the largest split-form m up to 100 and the whole form at 200 rows, every offsets kind: every row some expert owns is written with the dense entry's bits, nothing
    else is; a C index out of range is skipped; an A index out of range gives round16(bias); nothing lands outside c or past the queried
    workspace bytes, and the whole form writes no workspace byte."""
    from petit_kernel import ops
    dtype, kind = PAIRS[pair]
    E, n, k = 4, 208 if kind == "nv" else 224, 512
    split = int(form == "split")
    m = _m_of_form(pk, E, split, 100 if split else 200)
    assert m >= 8
    X = _Experts(pk, kind, dtype, E, n, k, m)
    g = torch.Generator().manual_seed(m)
    a_rows, c_rows = m // 2, m + 5
    a = torch.randn(a_rows, k, generator=g).to(dtype).to(DEV)
    a_idx = torch.randint(0, a_rows, (m,), generator=g).to(torch.int32)
    a_idx[3::11] = a_rows                                                                 # outside [0, a_rows): a zero row
    a_idx[5::13] = -1
    c_idx = torch.randperm(c_rows, generator=g)[:m].to(torch.int32)
    c_idx[2::9] = c_rows + 1                                                              # outside [0, c_rows): skipped
    c_idx[4::17] = -3                                                                     # (at m = 8: rows 3, 5 read zeros, rows 2, 4 are skipped)
    need = ops.moe_invariant_workspace_bytes(E, m, n, k, dtype, kind)
    assert (need > 0) == bool(split) and need % 4 == 0
    dense = _dense(pk, kind)
    zero = torch.zeros(1, k, dtype=dtype, device=DEV)
    for name, fractions in OFFSETS.items():
        offsets = np.array([int(round(f * m)) for f in fractions], dtype=np.int32)
        owner = row_ownership(offsets, m)
        assert (owner >= 0).sum() > m // 2 and ((owner < 0).any() or name in ("well formed", "descending", "negative"))
        c, ws = _Guarded(c_rows * n // 2), _Guarded(max(need // 4, 64))
        _abi_call(kind, dtype, X, a, torch.from_numpy(offsets).to(DEV), m, a_idx.to(DEV), c_idx.to(DEV), c_rows, True, None, c, ws)
        assert c.guards_intact() and ws.guards_intact(), name
        if not split:
            assert bool((ws.inside() == ws.POISON).all()), "the whole form wrote its workspace"
        got = c.inside().view(dtype).reshape(c_rows, n)
        want = torch.full((c_rows, n // 2), _Guarded.POISON, dtype=torch.int32, device=DEV).view(dtype).reshape(c_rows, n).clone()
        for e in range(E):
            rows = [r for r in range(m) if owner[r] == e]
            if not rows:
                continue
            src = torch.cat([a[int(a_idx[r])][None] if 0 <= int(a_idx[r]) < a_rows else zero for r in rows])
            b, s, gs, bias = X.expert(e)
            y = dense(src, b, s, gs, len(rows), n, k, bias)
            for i, r in enumerate(rows):
                if not 0 <= int(a_idx[r]) < a_rows:
                    assert _same(y[i], bias), "an A index out of range must give round16(bias)"
                if 0 <= int(c_idx[r]) < c_rows:
                    want[int(c_idx[r])] = y[i]
        assert _same(got, want), (pair, form, m, name)                                    # written rows: the dense bits; all others: the poison


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("split", "whole"))
@pytest.mark.parametrize("pair", list(PAIRS))
def test_all_rows_on_one_expert_of_130_equal_the_dense_call(pk, pair, form):
    """The largest split-form m up to 100, and 2100 rows (33 m-tiles of the whole form) on expert 77 of 130."""
    dtype, kind = PAIRS[pair]
    E, k, e = 130, 512, 77
    m = _m_of_form(pk, E, form == "split", 100 if form == "split" else 2100)
    a = torch.randn(m, k, generator=torch.Generator().manual_seed(m)).to(dtype).to(DEV)
    counts = [0] * E
    counts[e] = m
    for act in (None, "silu_mul"):
        n = 208 if kind == "nv" and not act else 224                                      # (gated: n % 32 == 0)
        X = _Experts(pk, kind, dtype, E, n, k, 3)
        out = _moe(pk, kind)(a, X.b, X.s, X.gs, _offsets(counts), m, n, k, E, bias=X.bias, activation=act)
        b, s, gs, bias = X.expert(e)
        assert _same(out, _dense(pk, kind)(a, b, s, gs, m, n, k, bias, act)), (pair, m, act)


# --- 4. graph capture ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("pair", list(PAIRS))
def test_graph_capture_replays_and_follows_new_offsets(pk, pair):
    dtype, kind = PAIRS[pair]
    E, n, k = 8, 224, 768                                                                 # (gated: n % 32 == 0; 224 = one n-block + a ragged one)
    X = _Experts(pk, kind, dtype, E, n, k, 9)
    mul = _moe(pk, kind)
    g = torch.Generator().manual_seed(1)
    forms = set()
    for counts, counts2 in (([1, 0, 2, 1, 0, 2, 1, 1], [0, 3, 0, 0, 4, 1, 0, 0]),                          # m = 8
                            ([17, 0, 16, 1, 15, 17, 16, 16], [0, 30, 5, 0, 40, 1, 6, 16]),                 # m = 98
                            ([65, 64, 0, 63, 64, 65, 1, 64], [100, 0, 90, 7, 0, 129, 40, 20])):            # m = 386
        m = sum(counts)
        assert sum(counts2) == m
        forms.add(pk.moe_invariant_form(m, E))
        a, a2 = (torch.randn(m, k, generator=g).to(dtype).to(DEV) for _ in range(2))
        off = _offsets(counts)
        kw = dict(bias=X.bias, activation="silu_mul")
        eager = mul(a, X.b, X.s, X.gs, off, m, n, k, E, **kw)
        eager2 = mul(a2, X.b, X.s, X.gs, _offsets(counts2), m, n, k, E, **kw)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = mul(a, X.b, X.s, X.gs, off, m, n, k, E, **kw)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same(out, eager), (pair, m)
        off.copy_(_offsets(counts2))                                                      # in place: the replay reads the new routing
        a.copy_(a2)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same(out, eager2) and not _same(eager, eager2), (pair, m)
    assert forms == {0, 1}                                                                # one split call at least, one whole call at least


# --- 5. the layer ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def layer_weights(pk):
    """H = 512, I = 512, 8 routed experts and one shared, NVFP4 and MXFP4, quantised once for the module."""
    H, I, E = 512, 512, 9
    g = torch.Generator().manual_seed(2024)
    w13 = (torch.randn(E, 2 * I, H, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
    w2 = (torch.randn(E, H, I, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
    out = {"router": (torch.randn(E - 1, H, generator=g) * 0.2).to(torch.bfloat16).to(DEV),
           "hidden": torch.randn(300, H, generator=g).to(torch.bfloat16).to(DEV),
           "norm": (torch.rand(H, generator=g) + 0.5).to(torch.bfloat16).to(DEV)}
    for kind, q in (("nvfp4", pk.quantize_nvfp4), ("mxfp4", pk.quantize_mxfp4)):
        out[kind] = q(w13) + q(w2)                                                        # (b13, s13, gs13, b2, s2, gs2), 9 experts
        out[kind + "-routed"] = q(w13[:8].contiguous()) + q(w2[:8].contiguous())          # the 8 routed experts alone
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ("plain", "norm", "shared"))
@pytest.mark.parametrize("kind", ("nvfp4", "mxfp4"))
def test_a_tokens_layer_output_is_the_same_in_any_batch(pk, layer_weights, kind, variant):
    """fp4_moe_routed(hidden, None, ..., router_weight=W, invariant=True): a token's output row -- with norm_weight both returned rows -- is
    identical on T = 37 tokens, on each of three of them alone, in a T = 5 batch that holds them at other positions, and in a T = 300 batch;
    the launches of these batches run in both forms."""
    topk, tokens = 2, (0, 18, 36)
    W, hidden, norm_w = layer_weights["router"], layer_weights["hidden"], layer_weights["norm"]
    wts = layer_weights[kind if variant == "shared" else kind + "-routed"]
    kw = dict(router_weight=W, invariant=True)
    if variant == "norm":
        kw.update(norm_weight=norm_w)
    if variant == "shared":
        kw.update(num_shared=1)
    slots = topk + (variant == "shared")
    assert {pk.moe_invariant_form(T * slots, len(wts[2])) for T in (1, 5, 37, 300)} == {0, 1}

    def run(x):
        out = pk.fp4_moe_routed(x.contiguous(), None, *wts, topk, kind, **kw)
        return out if isinstance(out, tuple) else (out,)

    full = run(hidden[:37])
    assert len(full) == (2 if variant == "norm" else 1) and all(t.shape == (37, 512) for t in full)
    five = hidden[100:105].clone()
    places = {0: 4, 18: 0, 36: 2}
    for t, p in places.items():
        five[p] = hidden[t]
    out5 = run(five)
    big = hidden.clone()                                                                  # T = 300; tokens 0 / 18 / 36 moved to 250 / 7 / 299
    moved = {0: 250, 18: 7, 36: 299}
    for t, p in moved.items():
        big[p] = hidden[t]
    out300 = run(big)
    for t in tokens:
        alone = run(hidden[t:t + 1])
        for i in range(len(full)):
            assert _same(alone[i][0], full[i][t]), (kind, variant, t, i, "alone")
            assert _same(out5[i][places[t]], full[i][t]), (kind, variant, t, i, "T = 5")
            assert _same(out300[i][moved[t]], full[i][t]), (kind, variant, t, i, "T = 300")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("nvfp4", "mxfp4"))
def test_the_layer_is_the_chain_built_by_hand(pk, layer_weights, kind):
    """moe_route_hidden, the two batch-invariant launches (gate_up gathered through token_index, down scattered through sorted_pos), moe_combine."""
    topk, T, H, I, E = 2, 37, 512, 512, 8
    W, x = layer_weights["router"], layer_weights["hidden"][:T].contiguous()
    b13, s13, gs13, b2, s2, gs2 = layer_weights[kind + "-routed"]
    got = pk.fp4_moe_routed(x, None, b13, s13, gs13, b2, s2, gs2, topk, kind, router_weight=W, invariant=True)
    w, ids, sorted_pos, offsets, token_index = pk.moe_route_hidden(x, W, topk)
    mul = pk.mul_nvfp4_a16_moe_invariant if kind == "nvfp4" else pk.mul_mxfp4_a16_moe_invariant
    m = T * topk
    h = mul(x, b13, s13, gs13, offsets, m, 2 * I, H, E, a_row_index=token_index, activation="silu_mul")
    y = mul(h, b2, s2, gs2, offsets, m, H, I, E, c_row_index=sorted_pos, c_rows=m)
    want = pk.moe_combine(y, w, ids, E)
    assert _same(got, want)

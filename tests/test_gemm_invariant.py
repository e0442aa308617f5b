"""The batch-invariant dense GEMM (include/petit_amd.h "Batch-invariant GEMM") on the GPU: exact on small numbers, inside the derived error
bound on random inputs, a row's bits independent of its batch, its position and the launch form (gated epilogues included), the gated outputs
equal to the existing entry's on exact inputs, the write contract through the C ABI on guarded buffers, and graph capture.

Shapes are the smallest that reach every path.  K is a multiple of 256 -- the packed scale layout exists for nothing else (csrc/layout.h), so
256 is the smallest K -- and the K set is {L (one slice), L + 256 (two), 3 L (S > 2), 4352 at n = 16 (L = 512, nine slices, the last one half as
long)}.  N covers one n-tile, less than an n-block of four tiles, and several n-blocks with a ragged last one; MXFP4 scales come in rows of 32,
so its N are multiples of 32.  M covers one row, a ragged tile, a whole tile, two tiles, a ragged fifth, and both sides of the form switch."""
import ctypes as C

import pytest
import torch

DEV = "cuda"
U = 2.0 ** -24
PAIRS = {"bf16-nv": (torch.bfloat16, "nv"), "bf16-mx": (torch.bfloat16, "mx"), "f16-nv": (torch.float16, "nv")}
NS = {"nv": (16, 48, 208), "mx": (32, 96, 224)}      # 208 = 3 n-blocks + 1 tile, 224 = 3 n-blocks + 2 tiles
GATED_NS = (32, 224)                                 # n % 32 == 0; 224: 7 gate / up pairs = one n-block + a ragged one
ACTS = ("silu_mul", "swiglu_oai")
FP4 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0], dtype=torch.float64)
E4M3_POW2 = {1.0: 0x38, 2.0: 0x40, 4.0: 0x48}        # e4m3 bytes of the powers of two the exact inputs use


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


def _mul(layer, kind):
    return layer.mul_nvfp4_a16_invariant if kind == "nv" else layer.mul_mxfp4_a16_invariant


def _k_set(n, dtype, kind):
    from petit_kernel import ops
    L = ops.invariant_geometry(n, 256, dtype, kind)[1]
    assert ops.invariant_geometry(n, L, dtype, kind) == (1, L) and ops.invariant_geometry(n, L + 256, dtype, kind) == (2, L)
    assert ops.invariant_geometry(n, 3 * L, dtype, kind)[0] > 2
    ks = [L, L + 256, 3 * L]
    if n == 16:
        S, L2 = ops.invariant_geometry(n, 4352, dtype, kind)
        assert S > 2 and 4352 % L2 != 0                                  # a last slice shorter than L
        ks.append(4352)
    return tuple(ks)


def _switch(n, k, dtype, kind):
    """(largest M of the split form, smallest M of the whole form) for a K of several slices."""
    from petit_kernel import ops
    S = ops.invariant_geometry(n, k, dtype, kind)[0]
    assert S > 1 and ops.invariant_slabs(1, n, k, dtype, kind) == S
    m = 1
    while ops.invariant_slabs(m + 1, n, k, dtype, kind) == S:
        m += 1
        assert m < 1 << 12
    assert ops.invariant_slabs(m + 1, n, k, dtype, kind) == 1
    return m, m + 1


def _m_set(n, dtype, kind):
    return sorted({1, 7, 16, 17, 65, *_switch(n, 512, dtype, kind)})


class _Weights:
    """Packed weights and scales of an [n, k] matrix on the GPU, and what the library says they hold: dequant_packed's float32, as float64."""

    def __init__(self, pk, kind, n, k, code, sbyte):
        from petit_kernel import ops
        q = (code[:, 0::2] | (code[:, 1::2] << 4)).to(torch.uint8).contiguous().to(DEV).view(torch.int32)
        if kind == "nv":
            self.b = pk.repack_nvfp4(q, n, k)
            self.s = pk.process_nvfp4_scales(sbyte.to(torch.uint8).to(DEV).view(torch.float8_e4m3fn), n, k)
        else:
            self.b = pk.repack_mxfp4(q, n, k)
            self.s = pk.process_mxfp4_scales(sbyte.to(torch.uint8).to(DEV), n, k)
        self.w64 = ops.dequant_packed(self.b, self.s, n, k, kind + "fp4", torch.float32).cpu().double()


def _exact_problem(pk, kind, dtype, m, n, k, seed, gated=False):
    """FP4 codes from the format's values, power-of-two group scales, integer activations with many zeros, gs a power of two, an integer bias:
    every product and partial sum is a multiple of 1/2 below 2^22, exact in fp32 in any order."""
    g = torch.Generator().manual_seed(seed)
    group = 16 if kind == "nv" else 32
    code = torch.randint(0, 16, (n, k), generator=g)
    sval = torch.tensor([1.0, 2.0, 4.0])[torch.randint(0, 3, (n, k // group), generator=g)]
    sbyte = sval.clone().apply_(lambda v: E4M3_POW2[v]) if kind == "nv" else 127 + torch.log2(sval)
    W = _Weights(pk, kind, n, k, code, sbyte.long())
    assert torch.equal(W.w64, FP4[code] * sval.double().repeat_interleave(group, dim=1))          # the library reads what was written
    a = torch.randint(-3, 4, (m, k), generator=g) * (torch.rand(m, k, generator=g) < 0.5)
    bias = torch.randint(-8, 9, (n,), generator=g)
    gs = 2.0 ** -7 if gated else 0.25                                                               # (gated: y of a few units, inside exp's range)
    a64 = a.double()
    assert float((a64.abs() @ W.w64.abs().T).max()) < 2 ** 22
    acc = a64 @ W.w64.T
    return W, a.to(dtype).to(DEV), bias.to(dtype).to(DEV), torch.tensor([gs], dtype=torch.float32, device=DEV), acc, bias.double(), gs


def _random_problem(pk, kind, dtype, m, n, k, seed):
    g = torch.Generator().manual_seed(seed)
    group = 16 if kind == "nv" else 32
    code = torch.randint(0, 16, (n, k), generator=g)
    if kind == "nv":
        sbyte = torch.randint(0x28, 0x48, (n, k // group), generator=g)                           # e4m3 0.25 .. 3.75
    else:
        sbyte = torch.randint(124, 131, (n, k // group), generator=g)                             # 2^-3 .. 2^3
    W = _Weights(pk, kind, n, k, code, sbyte)
    a = torch.randn(m, k, generator=g).to(dtype)
    bias = torch.randn(n, generator=g).to(dtype)
    gs = torch.tensor([0.0123], dtype=torch.float32)
    return W, a.to(DEV), bias.to(DEV), gs.to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _round16(y64, dtype):
    """float64 -> the 16-bit type through float32; both roundings are monotonic, and exact inputs survive the first."""
    return y64.to(torch.float32).to(dtype)


# --- 1. exact ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("ni", (0, 1, 2))
@pytest.mark.parametrize("pair", list(PAIRS))
def test_exact_on_small_numbers(pk, pair, ni):
    """c equals the float64 result rounded once, with torch.equal: every (K, M) of the module's sets, both forms, both operator layers, with
    and without the bias and the global scale."""
    dtype, kind = PAIRS[pair]
    n = NS[kind][ni]
    ms = _m_set(n, dtype, kind)
    for k in _k_set(n, dtype, kind):
        W, a, bias, gs, acc, bias64, gsv = _exact_problem(pk, kind, dtype, max(ms), n, k, 1000 * n + k)
        for m in ms:
            for name, layer in _layers().items():
                for use_gs in (True, False):
                    for use_bias in (True, False):
                        out = _mul(layer, kind)(a[:m].contiguous(), W.b, W.s, gs if use_gs else None, m, n, k, bias if use_bias else None)
                        y = acc[:m] * (gsv if use_gs else 1.0) + (bias64 if use_bias else 0.0)
                        assert torch.equal(y.float().double(), y)                                   # exact in fp32: one rounding is left
                        assert out.dtype == dtype and out.shape == (m, n)
                        assert torch.equal(out.cpu(), _round16(y, dtype)), (name, pair, n, k, m, use_gs, use_bias)


# --- 2. the bound on random inputs -------------------------------------------------------------------------------------------------------

def _slab_y(pk, kind, dtype, W, a, bias, gs, m, n, k):
    """The split form through the C ABI into a workspace of the test's own: (c, y) with y the definition's fp32 value folded from the slabs
    the GEMM launch left there -- ((p_0 + p_1) + ...) * gs + bias, one fp32 operation at a time."""
    from petit_kernel import _lib, ops
    hints = ops._hints(kind, dtype)
    S = ops.invariant_slabs(m, n, k, dtype, kind)
    need = ops.invariant_workspace_bytes(m, n, k, dtype, kind)
    assert need == (S * m * n * 4 + 255) // 256 * 256 and need > 0
    ws = torch.zeros(need // 4, dtype=torch.float32, device=DEV)
    c = torch.empty((m, n), dtype=dtype, device=DEV)
    epi = _lib.Epilogue(bias.data_ptr(), 0, 0)
    fn = _lib.lib.petit_gemm_fp4_fp16_invariant if kind == "nv" else _lib.lib.petit_gemm_mxfp4_fp16_invariant
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = fn(ptr(c), ptr(a), ptr(W.b), ptr(W.s), ptr(gs), m, n, k, C.byref(hints), C.byref(epi), ptr(ws),
            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == _lib.PETIT_OK
    slabs = ws[:S * m * n].reshape(S, m, n)
    y = slabs[0].clone()
    for s in range(1, S):
        y = y + slabs[s]
    y = y * gs
    y = y + bias.float()
    return c, y


@pytest.mark.gpu
@pytest.mark.parametrize("ni", (0, 1, 2))
@pytest.mark.parametrize("pair", list(PAIRS))
def test_error_bound_on_random_inputs(pk, pair, ni):
    """round16(y64 - d) <= c <= round16(y64 + d) with d = 2 u (K + S + 2) (|gs| sum |a w| + |bias|), for every element of every (K, M) of the
    sets, both forms.  In the split form the fp32 y itself is read back from the slabs: |y - y64| <= d, round16(y) == c, and the largest
    |y - y64| in units of u |gs| sum |a w| is printed (profiles/gemm_invariant.md records it)."""
    from petit_kernel import ops
    dtype, kind = PAIRS[pair]
    n = NS[kind][ni]
    ms = _m_set(n, dtype, kind)
    split_max = _switch(n, 512, dtype, kind)[0]
    worst = 0.0
    for k in _k_set(n, dtype, kind):
        S = ops.invariant_geometry(n, k, dtype, kind)[0]
        W, a, bias, gs = _random_problem(pk, kind, dtype, max(ms), n, k, 7 * n + k)
        a64, b64, g64 = a.cpu().double(), bias.cpu().double(), float(gs.cpu().double())
        y64 = a64 @ W.w64.T * g64 + b64
        mag = abs(g64) * (a64.abs() @ W.w64.abs().T)
        delta = 2 * U * (k + S + 2) * (mag + b64.abs())
        lo, hi = _round16(y64 - delta, dtype).double(), _round16(y64 + delta, dtype).double()
        for m in ms:
            c = _mul(pk, kind)(a[:m].contiguous(), W.b, W.s, gs, m, n, k, bias).cpu().double()
            assert bool(((lo[:m] <= c) & (c <= hi[:m])).all()), (pair, n, k, m)
            if m <= split_max:
                c2, y = _slab_y(pk, kind, dtype, W, a[:m].contiguous(), bias, gs, m, n, k)
                err = (y.cpu().double() - y64[:m]).abs()
                assert bool((err <= delta[:m]).all()), (pair, n, k, m, float((err / delta[:m]).max()))
                assert _same(y.to(dtype), c2) and torch.equal(c2.cpu().double(), c)
                worst = max(worst, float((err / (U * mag[:m])).max()))
    print(f"invariant error {pair} n {n}: max |y - y64| = {worst:.3f} u |gs| sum|a w|")


# --- 3. invariance -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("activation", (None,) + ACTS)
@pytest.mark.parametrize("pair", list(PAIRS))
def test_a_rows_result_does_not_depend_on_its_batch(pk, pair, activation):
    """Row r of the batch's result, the row run alone (M = 1, the split form) and the same row at another position of a different batch are
    identical bit for bit -- for a batch in the split form and for one in the whole form, so the two forms meet on random data."""
    dtype, kind = PAIRS[pair]
    n, k = 224, 768
    split_m, whole_m = _switch(n, k, dtype, kind)
    act = {} if activation is None else {"activation": activation}
    mul = _mul(pk, kind)
    for m in (split_m, whole_m + 37):
        W, a, bias, gs = _random_problem(pk, kind, dtype, m, n, k, m + n)
        full = mul(a, W.b, W.s, gs, m, n, k, bias, **act)
        g = torch.Generator().manual_seed(m)
        for other_m in (whole_m + 9, 19):                                                           # a different batch of either form
            other = torch.randn(other_m, k, generator=g).to(dtype).to(DEV)
            for r in (0, 15, 16, m - 1):
                alone = mul(a[r:r + 1].contiguous(), W.b, W.s, gs, 1, n, k, bias, **act)
                assert _same(alone[0], full[r]), (pair, activation, m, r)
                pos = (r + 5) % other_m
                other[pos] = a[r]
                moved = mul(other, W.b, W.s, gs, other_m, n, k, bias, **act)
                assert _same(moved[pos], full[r]), (pair, activation, m, r, other_m, pos)


# --- 4. the gated formula ----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("activation", ACTS)
@pytest.mark.parametrize("n", GATED_NS)
@pytest.mark.parametrize("pair", list(PAIRS))
def test_gated_outputs_equal_the_existing_entrys_on_exact_inputs(pk, pair, n, activation):
    """On exact inputs the new entry and mul_*_a16(..., activation=...) see the same exact y and call the same epilogue function: their gated
    outputs are equal bit for bit, in both forms and both operator layers."""
    dtype, kind = PAIRS[pair]
    old = pk.mul_nvfp4_a16 if kind == "nv" else pk.mul_mxfp4_a16
    ms = _m_set(n, dtype, kind)
    for k in (256, 768):
        W, a, bias, gs, _, _, _ = _exact_problem(pk, kind, dtype, max(ms), n, k, 31 * n + k, gated=True)
        for m in ms:
            want = old(a[:m].contiguous(), W.b, W.s, gs, m, n, k, -1, bias=bias, activation=activation)
            for name, layer in _layers().items():
                got = _mul(layer, kind)(a[:m].contiguous(), W.b, W.s, gs, m, n, k, bias, activation)
                assert got.shape == (m, n // 2) and _same(got, want), (name, pair, n, k, m, activation)


# --- 5. the write contract, through the C ABI --------------------------------------------------------------------------------------------

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

    def check(self, what, all_written=True):
        g = self.GUARD
        assert bool((self.buf[:g] == self.POISON).all()) and bool((self.buf[g + self.count:] == self.POISON).all()), f"{what}: a write outside"
        if all_written:
            halves = self.inside().view(torch.int16)
            assert bool((halves != (self.POISON & 0xFFFF) - 0x10000).all()) and bool((halves != self.POISON >> 16).all()), \
                f"{what}: an element was not written"


@pytest.mark.gpu
@pytest.mark.parametrize("activation", (None, "silu_mul"))
@pytest.mark.parametrize("pair", list(PAIRS))
def test_write_contract_through_the_c_abi(pk, pair, activation):
    """M = 17 (split) and the first whole-form M on a ragged N, poisoned and guarded buffers: every element of c is written, nothing lands
    outside c, nothing past the bytes the workspace query declares, and the whole form writes no workspace at all."""
    from petit_kernel import _lib, ops
    dtype, kind = PAIRS[pair]
    n, k = 224, 512
    act = ops._ACTIVATIONS[activation]
    n_out = n // 2 if act else n
    hints = ops._hints(kind, dtype)
    fn = _lib.lib.petit_gemm_fp4_fp16_invariant if kind == "nv" else _lib.lib.petit_gemm_mxfp4_fp16_invariant
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for m in (17, _switch(n, k, dtype, kind)[1]):
        W, a, bias, gs = _random_problem(pk, kind, dtype, m, n, k, m)
        need = ops.invariant_workspace_bytes(m, n, k, dtype, kind)
        whole = ops.invariant_slabs(m, n, k, dtype, kind) == 1
        assert (need == 0) == whole and need % 4 == 0
        c, ws = _Guarded(m * n_out // 2), _Guarded(max(need // 4, 64))
        epi = _lib.Epilogue(bias.data_ptr(), act, 0)
        rc = fn(c.ptr, ptr(a), ptr(W.b), ptr(W.s), ptr(gs), m, n, k, C.byref(hints), C.byref(epi), ws.ptr, stream)
        torch.cuda.synchronize()
        assert rc == _lib.PETIT_OK
        c.check(f"c at m = {m}")
        ws.check(f"workspace at m = {m}", all_written=False)
        if whole:
            assert bool((ws.inside() == ws.POISON).all()), "the whole form wrote its workspace"
        want = _mul(pk, kind)(a, W.b, W.s, gs, m, n, k, bias, activation)
        assert _same(c.inside().view(dtype).reshape(m, n_out), want)


# --- 6. graph capture --------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("pair", list(PAIRS))
def test_graph_capture_replays_the_eager_bits(pk, pair):
    dtype, kind = PAIRS[pair]
    n, k = 208 if kind == "nv" else 224, 768
    mul = _mul(pk, kind)
    for m in _switch(n, k, dtype, kind):                                                            # one split-form call, one whole-form call
        W, a, bias, gs = _random_problem(pk, kind, dtype, m, n, k, 11 * m)
        eager = mul(a, W.b, W.s, gs, m, n, k, bias)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = mul(a, W.b, W.s, gs, m, n, k, bias)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same(out, eager), (pair, m)

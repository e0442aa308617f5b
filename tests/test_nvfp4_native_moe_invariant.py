"""The batch-invariant MoE launch on NVFP4 images (include/petit_amd.h "Batch-invariant native-class GEMM and MoE launch on NVFP4 images") on the
GPU: every written row is the dense entry's row 0 of an m = 1 call on that row and its expert's image, in both forms, through every epilogue,
16-bit and quantised input, with and without row indices; malformed offsets and out-of-range C indices leave rows untouched (poisoned,
guarded buffers through the C ABI); a captured graph follows new offsets; and the layer examples/nvfp4_native_invariant.py composes gives a
token the same row alone and in a batch.  E in {1, 4, 16} at (n, k) = (64, 1024) and (128, 1536)."""
import ctypes as C
import functools
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

from petit_kernel import _lib
from test_gpu_parity import DEV, pk  # noqa: F401
from test_moe_invariant import OFFSETS, _Guarded, _offsets, _same, row_ownership
from test_native_invariant_abi import BF16, FMTS, FP16, OK, dt
from test_nvfp4_native_invariant_abi import NV, image_bytes

pytestmark = pytest.mark.gpu
L = _lib.lib
ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(64, 1024), (128, 1536)]
EXPERTS = (1, 4, 16)
CASES = [(fmt, is_bf16) for fmt in FMTS for is_bf16 in (True, False)]
IDS = [f"{fmt}-{'bf16' if b else 'fp16'}" for fmt, b in CASES]
A_ROWS = 8
EPILOGUES = ((False, None), (True, None), (True, "silu_mul"), (True, "swiglu_oai"))      # (bias, activation), the bias per expert


class Experts:
    """E experts' [n, k] weights quantised to NVFP4 on the device and re-encoded into their images back to back; the NVFP4 global scale and one
    bias row per expert; expert e's own image as the dense entry takes it: a byte range of the stacked ones."""

    def __init__(self, pk, dtype, E, n, k, seed):
        g = torch.Generator().manual_seed(seed)
        w = (torch.randn(E, n, k, generator=g) * (0.25 + torch.rand(E, 1, 1, generator=g))).to(torch.bfloat16).to(DEV)
        b, s, self.gs = pk.quantize_nvfp4(w)
        self.images = pk.nvfp4_native_images(b, s, E, n, k)
        self.bias = torch.randn(E, n, generator=g).to(dtype).to(DEV)
        self.E, self.n, self.k, self.per = E, n, k, image_bytes(n, k)
        assert self.images.numel() == E * self.per and self.per % 256 == 0 and self.gs.numel() == E

    def expert(self, e):
        return self.images[e * self.per:(e + 1) * self.per], self.gs[e:e + 1], self.bias[e]


@functools.lru_cache(maxsize=None)
def experts(E, n, k, is_bf16):
    import petit_kernel
    return Experts(petit_kernel, dt(is_bf16), E, n, k, 100 * E + n + k)


def routings(E):
    """(split, counts): the split form at m = 8 over (at most) 4 experts, the whole form at m = 70 with one expert holding 65 rows; empty
    experts wherever E allows, and every row on the last expert."""
    if E == 1:
        return [(True, [8]), (False, [70])]
    if E == 4:
        return [(True, [3, 0, 4, 1]), (True, [2, 2, 2, 2]), (False, [65, 0, 4, 1]), (True, [0, 0, 0, 8]), (False, [0, 0, 0, 70])]
    c1, c2, c3, c4 = [0] * E, [0] * E, [0] * E, [0] * E
    c1[1], c1[6], c1[7], c1[14] = 3, 1, 2, 2
    c2[2], c2[3], c2[9], c2[15] = 65, 1, 3, 1
    c3[E - 1], c4[E - 1] = 8, 70
    return [(True, c1), (False, c2), (True, c3), (False, c4)]


def layers():
    from petit_kernel import compiled, ops
    assert compiled.available(), compiled.why_unavailable()
    return {"ctypes": ops, "compiled": compiled}


# --- 1. every row is the dense entry's -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
@pytest.mark.parametrize("E", EXPERTS)
@pytest.mark.parametrize("n,k", SHAPES)
def test_every_row_equals_the_dense_entry_on_that_row_and_its_experts_image(pk, n, k, E, fmt, is_bf16):
    """Grouped row r of expert e equals row 0 of mul_nvfp4_native_invariant(size_m=1) on that row with expert e's image, &gs[e] and bias[e]: both
    forms, plain / bias / silu_mul / swiglu_oai, 16-bit input gathered through a_row_index against quantised grouped input, C scattered
    through c_row_index, both operator layers."""
    dtype = dt(is_bf16)
    lay = layers()
    g = torch.Generator().manual_seed(E + n)
    X = experts(E, n, k, is_bf16)
    a = torch.randn(A_ROWS, k, generator=g).to(dtype).to(DEV)
    ref, forms = {}, set()

    def want_row(ei, e, ar):
        if (ei, e, ar) not in ref:
            use_bias, act = EPILOGUES[ei]
            image, gs, bias = X.expert(e)
            ref[(ei, e, ar)] = pk.mul_nvfp4_native_invariant(a[ar:ar + 1], image, gs, 1, n, k, fmt, bias if use_bias else None, act)[0]
        return ref[(ei, e, ar)]

    for i, (split, counts) in enumerate(routings(E)):
        m = sum(counts)
        assert pk.native_moe_invariant_form(m, E) == int(split) and m == (8 if split else 70)
        forms.add(split)
        owner = np.repeat(np.arange(E), counts)
        a_idx = torch.tensor([(5 * int(owner[r]) + 3 * r) % A_ROWS for r in range(m)], dtype=torch.int32)
        c_idx = torch.randperm(m, generator=g).to(torch.int32)
        grouped = a[a_idx.long().to(DEV)].contiguous()
        off = _offsets(counts)
        for ei, (use_bias, act) in enumerate(EPILOGUES):
            kw = dict(fmt=fmt, bias=X.bias if use_bias else None, activation=act)
            want = torch.stack([want_row(ei, int(owner[r]), int(a_idx[r])) for r in range(m)])
            mul = lay[("ctypes", "compiled")[(ei + i) % 2]].mul_nvfp4_native_moe_invariant
            out = mul(a, X.images, X.gs, off, m, n, k, E, a_row_index=a_idx.to(DEV), c_row_index=c_idx.to(DEV), **kw)
            assert out.shape == (m, n // 2 if act else n) and out.dtype == dtype
            assert _same(out[c_idx.long().to(DEV)], want), (counts, ei, "indexed")
            assert _same(mul(grouped, X.images, X.gs, off, m, n, k, E, **kw), want), (counts, ei, "grouped")
            qa = pk.quantize_activation_rows(a, fmt, a_idx.to(DEV))
            assert _same(mul(qa, X.images, X.gs, off, m, n, k, E, **kw), want), (counts, ei, "quantised")
    assert forms == {True, False}


# --- 2. malformed offsets, out-of-range C indices: the write contract through the C ABI --------------------------------------------------------

def abi_call(X, dtype, fmt, a, quantized, offsets, m, a_idx, a_rows, c_idx, c_rows, c, ws):
    from petit_kernel import ops
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    hints = ops._hints("nv", dtype)
    epi = _lib.Epilogue(X.bias.data_ptr(), 0, 0)
    rc = L.petit_gemm_nvfp4_native_moe_invariant(c.ptr, ptr(a), ptr(X.images), ptr(X.gs), ptr(offsets), X.E, m, X.n, X.k, ptr(a_idx), a_rows,
                                                 ptr(c_idx), c_rows, C.byref(hints), FMTS[fmt], quantized, C.byref(epi), ws.ptr,
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == OK


@pytest.mark.parametrize("form", ("split", "whole"))
@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
def test_write_contract_on_poisoned_guarded_buffers(pk, fmt, is_bf16, form):
    """E = 4, offsets that are well formed, leave rows to no expert, decrease, go negative and exceed m; a C index with out-of-range entries;
    16-bit input through an A index and quantised input: every row some expert owns is written with the dense entry's bits, rows of no expert
    and rows nothing names keep the poison, nothing lands outside c or outside exactly the queried workspace bytes."""
    from petit_kernel import ops
    dtype = dt(is_bf16)
    E, n, k = 4, 128, 1536
    split = form == "split"
    m = 8 if split else 70
    assert (pk.native_moe_invariant_form(m, E) == 1) == split
    X = experts(E, n, k, is_bf16)
    g = torch.Generator().manual_seed(m)
    a_rows, c_rows = m // 2, m + 5
    a = torch.randn(a_rows, k, generator=g).to(dtype).to(DEV)
    a_idx = torch.randint(0, a_rows, (m,), generator=g).to(torch.int32)
    c_idx = torch.randperm(c_rows, generator=g)[:m].to(torch.int32)
    c_idx[2::9] = c_rows + 1                                                              # outside [0, c_rows): stores nothing
    c_idx[4::17] = -3
    grouped = a[a_idx.long().to(DEV)].contiguous()
    for quantized in (0, 1):
        need = ops.native_moe_invariant_workspace_bytes(E, m, n, k, dtype, fmt, bool(quantized))
        assert need % 256 == 0 and (need > 0) == (split or not quantized)
        src = pk.quantize_activation_rows(a, fmt, a_idx.to(DEV)).data if quantized else a
        for name, fractions in OFFSETS.items():
            offsets = np.array([int(round(f * m)) for f in fractions], dtype=np.int32)
            owner = row_ownership(offsets, m)
            c, ws = _Guarded(c_rows * n // 2), _Guarded(max(need // 4, 64))
            assert ws.ptr.value % 256 == 0 and c.ptr.value % 16 == 0
            abi_call(X, dtype, fmt, src, quantized, torch.from_numpy(offsets).to(DEV), m, None if quantized else a_idx.to(DEV), a_rows, c_idx.to(DEV),
                     c_rows, c, ws)
            assert c.guards_intact() and ws.guards_intact(), name
            if not need:
                assert bool((ws.inside() == ws.POISON).all()), "a call without workspace wrote it"
            elif need // 4 < ws.count:
                assert bool((ws.inside()[need // 4:] == ws.POISON).all())
            got = c.inside().view(dtype).reshape(c_rows, n)
            want = torch.full((c_rows, n // 2), _Guarded.POISON, dtype=torch.int32, device=DEV).view(dtype).reshape(c_rows, n).clone()
            for r in range(m):
                if owner[r] >= 0 and 0 <= int(c_idx[r]) < c_rows:
                    image, gs, bias = X.expert(int(owner[r]))
                    want[int(c_idx[r])] = pk.mul_nvfp4_native_invariant(grouped[r:r + 1], image, gs, 1, n, k, fmt, bias)[0]
            assert _same(got, want), (form, quantized, name)


# --- 3. graph capture --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
def test_graph_capture_replays_and_follows_new_offsets(pk, fmt, is_bf16):
    dtype = dt(is_bf16)
    E, n, k = 4, 128, 1536
    X = experts(E, n, k, is_bf16)
    mul = pk.mul_nvfp4_native_moe_invariant
    g = torch.Generator().manual_seed(1)
    for counts, counts2 in (([3, 0, 4, 1], [0, 6, 0, 1]), ([65, 0, 4, 1], [10, 30, 0, 20])):
        m, m2 = sum(counts), sum(counts2)
        pool = torch.randn(m, k, generator=g).to(dtype).to(DEV)
        off = _offsets(counts)
        kw = dict(fmt=fmt, bias=X.bias, activation="silu_mul")
        eager = mul(pool, X.images, X.gs, off, m, n, k, E, **kw)
        for _ in range(3):                                                                # repeated launches are identical
            assert _same(mul(pool, X.images, X.gs, off, m, n, k, E, **kw), eager)
        eager2 = mul(pool, X.images, X.gs, _offsets(counts2), m, n, k, E, **kw)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = mul(pool, X.images, X.gs, off, m, n, k, E, **kw)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same(out, eager), m
        off.copy_(_offsets(counts2))                                                      # in place: the replay reads the new routing
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same(out[:m2], eager2[:m2]) and not _same(eager[:m2], eager2[:m2]), m
        assert bool((out[m2:].view(torch.int16) == 0).all())                              # rows of no expert keep the zeros


# --- 4. the composed layer of the example --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def example():
    spec = importlib.util.spec_from_file_location("nvfp4_native_invariant_example", ROOT / "examples" / "nvfp4_native_invariant.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("fmt", list(FMTS))
def test_the_examples_layer_gives_a_token_the_same_row_alone_and_in_a_batch(pk, fmt):
    """NvFp4InvariantMoE (align, gathering quantiser, the two launches, combine) on two tokens and on 40 (the whole form): each token's output
    row alone equals its row in the batch; and the dense layer of the example likewise."""
    E, H, I, topk = 4, 256, 256, 2
    g = torch.Generator().manual_seed(7)
    moe = example().NvFp4InvariantMoE((torch.randn(E, 2 * I, H, generator=g) * 0.05).bfloat16().to(DEV),
                                      (torch.randn(E, H, I, generator=g) * 0.05).bfloat16().to(DEV), fmt)
    dense = example().NvFp4InvariantLinear((torch.randn(64, H, generator=g) * 0.05).bfloat16().to(DEV), fmt=fmt)
    forms = set()
    for tokens in (2, 40):
        hidden = torch.randn(tokens, H, generator=g).bfloat16().to(DEV)
        w, ids = torch.topk(torch.softmax(torch.randn(tokens, E, generator=g), dim=1), topk, dim=1)
        w, ids = w.contiguous().to(DEV), ids.to(torch.int32).contiguous().to(DEV)
        forms.add(pk.native_moe_invariant_form(tokens * topk, E))
        full, dfull = moe(hidden, w, ids), dense(hidden)
        assert full.shape == (tokens, H) and not torch.isnan(full.float()).any()
        for t in (0, tokens - 1):
            assert _same(moe(hidden[t:t + 1], w[t:t + 1], ids[t:t + 1])[0], full[t]), (tokens, t)
            assert _same(dense(hidden[t:t + 1])[0], dfull[t]), (tokens, t)
    assert forms == {0, 1}

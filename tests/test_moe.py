"""Routed-expert (MoE) launch: petit_gemm_fp4_fp16_moe / mul_*_a16_moe, moe_align and fp4_moe.

Unmarked tests run without a GPU (argument checks of the C ABI, the stacked repack, moe_align on CPU tensors, which ids have a MoE form);
the @pytest.mark.gpu ones check the kernels against the oracle per expert, bit-identity with the dense path, graph replay with changing
routings and an end-to-end MoE layer.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from oracle import oracle as O

DEV = "cuda"


def _hints(pk, kind, is_bf16=True):
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = torch.bfloat16 if is_bf16 else torch.float16
    h.b_type = pk.DataType.float4_e2m1 if kind == "nv" else pk.DataType.mxfloat4_e2m1
    return h


def _is_tiled(pk, sid):
    return pk.ops._lib.describe_solution(sid).startswith("tiled")


def _min_streaming(kind, k):
    # K % 512 != 0 (two k-tiles per span): the MXFP4 table has two staged kernels of that span size (1 and 16 rows), both with a MoE form
    return 2 if kind == "mx" and k % 512 else 3


# --- without a GPU ----------------------------------------------------------------------------------------------------------------

def test_moe_abi_argument_checks_without_a_gpu():
    from petit_kernel import _lib
    L = _lib.lib
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p)
    auto = C.c_uint64(_lib.PETIT_SOLUTION_AUTO)

    def call(b_type, E, m, n, k, offsets=p):
        h = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, b_type, _lib.CXX_DTYPE_BF16, 0)
        return L.petit_gemm_fp4_fp16_moe(p, p, p, p, p, offsets, E, m, n, k, C.byref(h), auto, None, None)

    NV, MX = _lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_MXFP4_E2M1
    shape = _lib.PETIT_ERROR_PROBLEM_SHAPE
    assert call(NV, 8, 4, 24, 256) == shape                      # n % 16
    assert call(MX, 8, 4, 48, 256) == shape                      # MXFP4: n % 32
    assert call(NV, 8, 4, 256, 384) == shape                     # k % 256
    assert call(MX, 8, 4, 256, 640) == shape
    assert call(NV, 0, 4, 256, 256) == shape                     # E = 0
    assert call(NV, _lib.PETIT_MOE_MAX_EXPERTS + 1, 4, 256, 256) == shape
    assert call(NV, 8, 4, 256, 256, offsets=None) == shape       # null expert_offsets
    assert _lib.PETIT_MOE_MAX_EXPERTS == 1024
    # the resolver refuses the same problems (0) and names a kernel for a good one
    h = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, NV, _lib.CXX_DTYPE_BF16, 0)
    assert L.petit_gemm_moe_resolve_solution(C.byref(h), 8, 4, 24, 256, auto, None) == 0
    assert L.petit_gemm_moe_resolve_solution(C.byref(h), 0, 4, 256, 256, auto, None) == 0
    assert L.petit_gemm_moe_resolve_solution(C.byref(h), 8, 4, 256, 256, auto, None) != 0


@pytest.mark.parametrize("kind", ["nv", "mx"])
@pytest.mark.parametrize("k", [768, 2048])
def test_moe_forms_cover_both_regimes_without_a_gpu(kind, k):
    """Every (activation dtype, weight format) family keeps >= 3 streaming / decode and >= 2 tiled kernels with a MoE form for each span size;
    ids with a K split never have one; the MoE forms add no ids (the dense enumeration is unchanged by construction: the same table)."""
    import petit_kernel as pk
    n = 256
    for is_bf16 in (True, False):
        h = _hints(pk, kind, is_bf16)
        ids = set()
        for m in (1, 2, 4, 8, 16, 64, 512):
            ids.update(pk.ops.get_fp4_solutions(h, m, n, k))
        acc = [i for i in ids if pk.moe_resolve_solution(h, 8, 64, n, k, i)]
        assert sum(_is_tiled(pk, i) for i in acc) >= 2
        assert sum(not _is_tiled(pk, i) for i in acc) >= _min_streaming(kind, k)
        for i in acc:
            assert pk.moe_resolve_solution(h, 8, 64, n, k, i) == (i & ~(0xF << 28)) | ((1 if kind == "nv" else 2) << 28)
            split2 = (i & ~(0xF << 60)) | (2 << 60)
            assert pk.moe_resolve_solution(h, 8, 64, n, k, split2) == 0
        auto = pk.moe_resolve_solution(h, 8, 64, n, k, -1)
        assert auto in {(i & ~(0xF << 28)) | ((1 if kind == "nv" else 2) << 28) for i in acc}


def _moe_align_np(ids, E):
    flat = ids.reshape(-1)
    order = np.argsort(flat, kind="stable")
    counts = np.bincount(flat, minlength=E)
    return order, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


@pytest.mark.parametrize("case", ["random", "empty_first_last", "all_on_one", "single_token"])
def test_moe_align_cpu_matches_numpy(case):
    import petit_kernel as pk
    rng = np.random.default_rng(7)
    E, T, topk = 16, 37, 4
    if case == "random":
        ids = np.stack([rng.choice(E, topk, replace=False) for _ in range(T)])
    elif case == "empty_first_last":
        ids = np.stack([rng.choice(np.arange(1, E - 1), topk, replace=False) for _ in range(T)])
    elif case == "all_on_one":
        ids, topk = np.full((T, 1), 5), 1
    else:
        ids, T = np.array([[3, 0, 15, 9]]), 1
    order, offs = _moe_align_np(ids, E)
    sorted_idx, offsets = pk.moe_align(torch.from_numpy(ids.astype(np.int32)), E)
    assert sorted_idx.device.type == "cpu" and offsets.dtype == torch.int32 and offsets.shape == (E + 1,)
    assert np.array_equal(offsets.numpy(), offs)
    assert np.array_equal(sorted_idx.numpy(), order)
    if case == "empty_first_last":
        assert offs[1] == 0 and offs[E] == offs[E - 1]


@pytest.mark.parametrize("n,k", [(32, 256), (96, 768), (272, 2048)])
def test_stacked_repack_equals_per_expert_repacks(n, k):
    """The packed layout is n-tile-major: packing the stacked [E * n, k] tensors in one call gives the experts' blocks back to back."""
    from petit_kernel import offline
    E = 3
    rng = np.random.default_rng(n + k)
    q = torch.from_numpy(rng.integers(0, 256, (E * n, k // 2), dtype=np.uint8)).view(torch.int32)
    s_nv = torch.from_numpy(rng.integers(1, 120, (E * n, k // 16), dtype=np.uint8)).view(torch.float8_e4m3fn)
    s_mx = torch.from_numpy(rng.integers(110, 140, (E * n, k // 32), dtype=np.uint8))
    stacked = offline.repack_nvfp4_cpu(q, E * n, k)
    per = torch.cat([offline.repack_nvfp4_cpu(q[e * n:(e + 1) * n].contiguous(), n, k) for e in range(E)])
    assert torch.equal(stacked, per)
    stacked = offline.process_nvfp4_scales_cpu(s_nv, E * n, k).view(torch.uint8)
    per = torch.cat([offline.process_nvfp4_scales_cpu(s_nv[e * n:(e + 1) * n].contiguous(), n, k).view(torch.uint8) for e in range(E)])
    assert torch.equal(stacked, per)
    if n % 32 == 0:
        stacked = offline.process_mxfp4_scales_cpu(s_mx, E * n, k)
        per = torch.cat([offline.process_mxfp4_scales_cpu(s_mx[e * n:(e + 1) * n].contiguous(), n, k) for e in range(E)])
        assert torch.equal(stacked, per)


# --- on the GPU -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pk():
    import petit_kernel
    assert torch.cuda.is_available()
    assert torch.cuda.get_device_properties(0).gcnArchName.startswith("gfx950")
    return petit_kernel


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _to_f32(b, is_bf16):
    return O.bf16_bits_to_f32(b) if is_bf16 else O.f16_bits_to_f32(b)


class Experts:
    """E experts' [n, k] FP4 weights: raw (for the oracle) and packed back to back on the GPU (one repack of the stacked tensor)."""

    def __init__(self, pk, kind, E, n, k, seed, mx_band=(119, 136), gs_scale=1.0):
        rng = np.random.default_rng(seed)
        self.kind, self.E, self.n, self.k = kind, E, n, k
        self.q = rng.integers(0, 256, (E * n, k // 2), dtype=np.uint8)
        if kind == "nv":
            sf = rng.random((E * n, k // 16), dtype=np.float32) * 3.5 + 0.25
            self.s = torch.from_numpy(sf).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
        else:
            self.s = rng.integers(mx_band[0], mx_band[1], (E * n, k // 32), dtype=np.uint8)
        self.gs = ((rng.random(E) * 1.5 + 0.5) * gs_scale).astype(np.float32)
        qd = torch.from_numpy(self.q).to(DEV).view(torch.int32)
        if kind == "nv":
            self.b = pk.repack_nvfp4(qd, E * n, k)
            self.sp = pk.process_nvfp4_scales(torch.from_numpy(self.s).to(DEV).view(torch.float8_e4m3fn), E * n, k)
        else:
            self.b = pk.repack_mxfp4(qd, E * n, k)
            self.sp = pk.process_mxfp4_scales(torch.from_numpy(self.s).to(DEV), E * n, k)
        self.gsd = torch.from_numpy(self.gs).to(DEV)
        self._dq = {}

    def dq(self, e):  # f32 [n, k]
        if e not in self._dq:
            q, s = self.q[e * self.n:(e + 1) * self.n], self.s[e * self.n:(e + 1) * self.n]
            self._dq[e] = O.dequant_nvfp4(q, s) if self.kind == "nv" else O.dequant_mxfp4(q, s)
        return self._dq[e]

    def mul(self, pk, a, offsets, m, solution_id=-1, bias=None, activation=None):
        fn = pk.mul_nvfp4_a16_moe if self.kind == "nv" else pk.mul_mxfp4_a16_moe
        return fn(a, self.b, self.sp, self.gsd, offsets, m, self.n, self.k, self.E, solution_id, bias=bias, activation=activation)

    def dense(self, pk, a, e, solution_id=-1):
        n, k = self.n, self.k
        fn = pk.mul_nvfp4_a16 if self.kind == "nv" else pk.mul_mxfp4_a16
        per_s = n * k // (16 if self.kind == "nv" else 32)
        b = self.b.view(-1)[e * n * k // 8:(e + 1) * n * k // 8].view(n // 16, 2 * k)
        s = self.sp.view(-1)[e * per_s:(e + 1) * per_s]
        s = s.view(n, k // 16) if self.kind == "nv" else s.view(n // 32, k)
        return fn(a, b, s, self.gsd[e:e + 1], a.shape[0], n, k, solution_id)


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def _check_expert(got_bits, a_bits, is_bf16, ex, e, bias_e=None, act=False):
    _, cf = O.gemm_ref(a_bits, is_bf16, ex.dq(e), float(ex.gs[e]))
    y = cf.astype(np.float64)
    if bias_e is not None:
        y = y + bias_e[None, :]
    if act:
        h = y.shape[1] // 2
        y = y[:, :h] / (1.0 + np.exp(-y[:, :h])) * y[:, h:]
    c = _to_f32(got_bits, is_bf16).astype(np.float64)
    bound = np.maximum(1e-2, 1e-2 * np.abs(y))
    if ex.kind == "mx" and not act:   # e8m0 scales span many binades: an f32 accumulation carries ~sqrt(K) 2^-24 of sum |a||w| (test_gpu_parity)
        sa = (np.abs(_to_f32(a_bits, is_bf16)) @ np.abs(ex.dq(e)).T) * float(ex.gs[e])
        bound = np.maximum(bound, 1e-5 * sa)
    fin = np.abs(y) < (3.0e38 if is_bf16 else 6.0e4)   # (fp16 outputs beyond its range round to inf, as in test_gpu_parity.check_gemm)
    err = np.where(fin, np.abs(c - y), 0.0)
    assert np.isfinite(c[fin]).all()
    assert (err <= bound).all(), f"expert {e}: {int((err > bound).sum())} of {err.size} out of bound, worst err {err.max():.4g}"


def _routing_counts(rng, T, E, topk):
    ids = np.stack([rng.choice(E, topk, replace=False) for _ in range(T)])
    return np.bincount(ids.reshape(-1), minlength=E)


# (name, E, counts or (T, topk), k, bias, act)
PARITY_CASES = [
    ("decode_T1_E8_top2", 8, (1, 2), 2048, False, False),
    ("decode_T4_E128_top8", 128, (4, 8), 768, True, False),
    ("decode_T16_E8_top2_silu", 8, (16, 2), 2048, False, True),
    ("decode_T16_E128_top8", 128, (16, 8), 2048, False, False),
    ("decode_T4_E8_top8_bias_silu", 8, (4, 8), 768, True, True),
    ("counts_1_15_16_17_127_128_129_empty_ends", 10, [0, 1, 15, 16, 17, 127, 128, 129, 3, 0], 768, True, False),
    ("one_expert_holds_every_row", 8, [0, 0, 0, 300, 0, 0, 0, 0], 2048, False, True),
    ("prefill_T512_E8_top2", 8, (512, 2), 2048, False, False),
    ("prefill_T512_E64_top8_silu", 64, (512, 8), 768, True, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", PARITY_CASES, ids=[c[0] for c in PARITY_CASES])
@pytest.mark.parametrize("kind,is_bf16", [("nv", True), ("nv", False), ("mx", True), ("mx", False)])
def test_moe_vs_oracle_per_expert(pk, kind, is_bf16, case):
    name, E, routing, k, with_bias, act = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    counts = np.array(routing) if isinstance(routing, list) else _routing_counts(rng, routing[0], E, routing[1])
    m = int(counts.sum())
    n = 272 if kind == "nv" and not act else 288       # ragged n-tile counts (17 / 18 tiles)
    ex = Experts(pk, kind, E, n, k, seed=E * 1000 + k, mx_band=(122, 127) if act else (119, 136), gs_scale=0.05 if act else 1.0)
    dtype = torch.bfloat16 if is_bf16 else torch.float16
    a = rng.standard_normal((m, k), dtype=np.float32)
    a_bits = O.f32_to_bf16_bits(a) if is_bf16 else a.astype(np.float16).view(np.uint16)
    ad = torch.from_numpy(a_bits.view(np.int16).copy()).view(dtype).to(DEV)
    offs = _offsets(counts)
    bias = None
    if with_bias:
        bias = (torch.randn(E, n, generator=torch.Generator().manual_seed(3)) * 0.5).to(dtype).to(DEV)
    c = ex.mul(pk, ad, torch.from_numpy(offs).to(DEV), m, bias=bias, activation="silu_mul" if act else None)
    torch.cuda.synchronize()
    assert c.shape == (m, n // 2 if act else n) and c.dtype == dtype
    cb = _bits(c)
    bias_np = bias.float().cpu().numpy().astype(np.float64) if bias is not None else None
    for e in range(E):
        lo, hi = offs[e], offs[e + 1]
        if hi > lo:
            _check_expert(cb[lo:hi], a_bits[lo:hi], is_bf16, ex, e, None if bias_np is None else bias_np[e], act)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [768, 2048])
@pytest.mark.parametrize("kind,is_bf16", [("nv", True), ("nv", False), ("mx", True), ("mx", False)])
def test_moe_bit_identical_to_dense_per_expert(pk, kind, is_bf16, k):
    """For every id the MoE call accepts: each expert's rows equal a dense call on those rows with the same id, bit for bit (where the
    dense call takes that many rows: every expert whose row count the dense resolver accepts for the id is compared, and the count is printed);
    AUTO runs the id moe_resolve_solution names."""
    dtype = torch.bfloat16 if is_bf16 else torch.float16
    counts = np.array([1, 0, 3, 16, 40, 130, 0])
    E, m = len(counts), int(counts.sum())
    n = 288
    ex = Experts(pk, kind, E, n, k, seed=99 + k)
    offs = _offsets(counts)
    offd = torch.from_numpy(offs).to(DEV)
    ad = torch.randn(m, k, generator=torch.Generator().manual_seed(5)).to(dtype).to(DEV)
    h = _hints(pk, kind, is_bf16)
    ids = set()
    for r in (1, 3, 16, 40, 130):
        ids.update(pk.ops.get_fp4_solutions(h, r, n, k))
    accepted = sorted(i for i in ids if pk.moe_resolve_solution(h, E, m, n, k, i))
    assert sum(_is_tiled(pk, i) for i in accepted) >= 2 and sum(not _is_tiled(pk, i) for i in accepted) >= _min_streaming(kind, k)
    for sid in accepted:
        c = _bits(ex.mul(pk, ad, offd, m, sid))
        compared = 0
        # the experts whose row count the id's dense form takes, by the dense resolver: each of them must be compared, none may slip past below
        takes = [e for e in range(E) if counts[e] and pk.ops.resolve_solution(h, int(counts[e]), n, k, sid) != 0]
        for e in range(E):
            lo, hi = offs[e], offs[e + 1]
            if hi == lo:
                continue
            try:
                d = ex.dense(pk, ad[lo:hi].contiguous(), e, sid)
            except RuntimeError:
                assert e not in takes, f"{pk.ops._lib.describe_solution(sid)}: the dense resolver takes expert {e}'s {hi - lo} rows, the dense call refuses"
                continue   # (a staged kernel holds fewer rows than this expert has: the dense call refuses it)
            assert np.array_equal(c[lo:hi], _bits(d)), f"{pk.ops._lib.describe_solution(sid)}: expert {e} differs from the dense call"
            compared += 1
        print(f"moe vs dense {kind} bf16={is_bf16} k={k} [{pk.ops._lib.describe_solution(sid)}]: compared {compared} of {int((counts > 0).sum())} "
              f"experts with rows, the dense form takes {len(takes)}")
        assert compared >= 1, pk.ops._lib.describe_solution(sid)
        assert compared >= len(takes), pk.ops._lib.describe_solution(sid)
    auto = pk.moe_resolve_solution(h, E, m, n, k, -1)
    assert auto and pk.ops._lib.describe_solution(auto)
    assert np.array_equal(_bits(ex.mul(pk, ad, offd, m, -1)), _bits(ex.mul(pk, ad, offd, m, auto)))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["nv", "mx"])
def test_moe_refuses_ids_without_a_moe_form(pk, kind):
    n, k, E = 256, 2048, 4
    ex = Experts(pk, kind, E, n, k, seed=1)
    counts = np.array([2, 0, 1, 1])
    m = int(counts.sum())
    ad = torch.randn(m, k, device=DEV).to(torch.bfloat16)
    offd = torch.from_numpy(_offsets(counts)).to(DEV)
    h = _hints(pk, kind)
    ids = pk.ops.get_fp4_solutions(h, m, n, k)
    without = [i for i in ids if not pk.moe_resolve_solution(h, E, m, n, k, i)]
    assert without
    with pytest.raises(RuntimeError, match="No kernel implementation for solution_id="):
        ex.mul(pk, ad, offd, m, without[0])
    with_form = next(i for i in ids if pk.moe_resolve_solution(h, E, m, n, k, i))
    with pytest.raises(RuntimeError, match="No kernel implementation for solution_id="):
        ex.mul(pk, ad, offd, m, (with_form & ~(0xF << 60)) | (2 << 60))


def _make_layer(pk, kind, E, hid, inter, seed):
    w13 = Experts(pk, kind, E, 2 * inter, hid, seed, mx_band=(122, 127), gs_scale=0.05)
    w2 = Experts(pk, kind, E, hid, inter, seed + 1, mx_band=(122, 127), gs_scale=0.05)
    return w13, w2


def _layer_ref(x_bits, w13, w2, topk_w, topk_ids):
    xf = O.bf16_bits_to_f32(x_bits).astype(np.float64)
    inter = w13.n // 2
    out = np.zeros((xf.shape[0], w2.n))
    for e in np.unique(topk_ids):
        tok, slot = np.nonzero(topk_ids == e)
        y1 = xf[tok] @ w13.dq(e).astype(np.float64).T * float(w13.gs[e])
        h = y1[:, :inter] / (1.0 + np.exp(-y1[:, :inter])) * y1[:, inter:]
        y2 = h @ w2.dq(e).astype(np.float64).T * float(w2.gs[e])
        np.add.at(out, tok, y2 * topk_w[tok, slot][:, None])
    return out


def _routing(T, E, topk, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(T, E, generator=g)
    w, ids = torch.topk(torch.softmax(logits, -1), topk, dim=-1)
    return w.float(), ids.to(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [16, 256])
@pytest.mark.parametrize("kind", ["nvfp4", "mxfp4"])
def test_fp4_moe_end_to_end(pk, kind, T):
    """E = 8, top-2, hidden 1024, intermediate 512 against an f64 layer built from the oracle's dequant: rms error / output rms <= 1e-2
    (the exact-class budget of test_mlp_block_accuracy_budget)."""
    E, topk, hid, inter = 8, 2, 1024, 512
    w13, w2 = _make_layer(pk, kind[:2], E, hid, inter, 40 + T)
    x = torch.randn(T, hid, generator=torch.Generator().manual_seed(T)).to(torch.bfloat16)
    tw, tid = _routing(T, E, topk, T)
    out = pk.fp4_moe(x.to(DEV), w13.b, w13.sp, w13.gsd, w2.b, w2.sp, w2.gsd, tw.to(DEV), tid.to(DEV), kind)
    torch.cuda.synchronize()
    assert out.shape == (T, hid) and out.dtype == torch.bfloat16
    ref = _layer_ref(x.view(torch.int16).numpy().view(np.uint16), w13, w2, tw.numpy().astype(np.float64), tid.numpy())
    err = out.float().cpu().numpy().astype(np.float64) - ref
    rms = np.sqrt(np.mean(ref ** 2))
    assert np.sqrt(np.mean(err ** 2)) / rms <= 1e-2


@pytest.mark.gpu
def test_fp4_moe_graph_replay_with_changing_routing(pk):
    """One fp4_moe call captured under torch.cuda.graph with static input / routing buffers; three routings copied in and replayed, each
    bit-identical to the eager call.  (One capture stream, no parallel branches.)"""
    E, topk, hid, inter, T = 8, 2, 1024, 512, 16
    w13, w2 = _make_layer(pk, "nv", E, hid, inter, 77)
    x = torch.randn(T, hid, device=DEV).to(torch.bfloat16)
    tw0, tid0 = _routing(T, E, topk, 0)
    sx, stw, stid = x.clone(), tw0.to(DEV), tid0.to(DEV)

    def layer(xx, ww, ii):
        return pk.fp4_moe(xx, w13.b, w13.sp, w13.gsd, w2.b, w2.sp, w2.gsd, ww, ii, "nvfp4")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        layer(sx, stw, stid)    # warm-up off the default stream (allocator, lazy init)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = layer(sx, stw, stid)
    torch.cuda.synchronize()
    routings = [_routing(T, E, topk, 11), _routing(T, E, topk, 12), (torch.ones(T, topk) * 0.5, torch.tensor([[3, 5]] * T, dtype=torch.int32))]
    for i, (tw, tid) in enumerate(routings):
        xi = torch.randn(T, hid, device=DEV).to(torch.bfloat16)
        sx.copy_(xi)
        stw.copy_(tw.to(DEV))
        stid.copy_(tid.to(DEV))
        g.replay()
        torch.cuda.synchronize()
        eager = layer(xi, tw.to(DEV), tid.to(DEV))
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), eager.view(torch.int16)), f"replay {i} differs from the eager call"

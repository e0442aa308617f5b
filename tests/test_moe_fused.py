"""The fused MoE layer: indexed MoE launch (petit_gemm_fp4_fp16_moe_ex / mul_*_a16_moe_indexed), device align (petit_moe_align /
moe_align_device), top-k combine (petit_moe_combine / moe_combine) and fp4_moe_fused.

Unmarked tests run without a GPU (argument checks of the C ABI, Meta shapes of the torch ops, numpy restatements of the align and combine
definitions); the @pytest.mark.gpu ones check bit-identity with the plain MoE launch on gathered / scattered rows, the device align against
moe_align, the combine against its numpy restatement, the fused layer against the f64 oracle layer and fp4_moe, graph replay with changing
routings and out-of-range indices.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_moe import Experts, _hints, _layer_ref, _make_layer, _routing

DEV = "cuda"


# --- definitions, restated in numpy ----------------------------------------------------------------------------------------------------

def align_np(ids, E):
    """(sorted_pos, expert_offsets, token_index) of the align definition: routed entries (ids in [0, E)) grouped by expert, stable; rows past
    the routed count are -1."""
    topk = ids.shape[1]
    flat = ids.reshape(-1).astype(np.int64)
    valid = (flat >= 0) & (flat < E)
    pos = np.nonzero(valid)[0]
    pos = pos[np.argsort(flat[pos], kind="stable")]
    sp = np.full(flat.size, -1, np.int64)
    sp[:pos.size] = pos
    ti = np.where(sp >= 0, sp // topk, -1)
    off = np.concatenate([[0], np.cumsum(np.bincount(flat[valid], minlength=E))])
    return sp.astype(np.int32), off.astype(np.int32), ti.astype(np.int32)


def combine_np(slot_f32, w, ids, E):
    """acc = 0; for j in order, ids in [0, E) only: acc = acc + x * w, every step rounded to float32 (no FMA); returns the float32 acc."""
    T, topk = ids.shape
    x = slot_f32.reshape(T, topk, -1).astype(np.float32)
    acc = np.zeros((T, x.shape[2]), np.float32)
    for j in range(topk):
        prod = (x[:, j, :] * w[:, j:j + 1].astype(np.float32)).astype(np.float32)
        ok = ((ids[:, j] >= 0) & (ids[:, j] < E))[:, None]
        acc = np.where(ok, (acc + prod).astype(np.float32), acc)
    return acc


def _to16_bits(acc, is_bf16):
    t = torch.from_numpy(acc).to(torch.bfloat16 if is_bf16 else torch.float16)   # RNE
    return t.view(torch.int16).numpy().view(np.uint16)


# --- without a GPU ----------------------------------------------------------------------------------------------------------------

def test_fused_abi_argument_checks_without_a_gpu():
    from petit_kernel import _lib
    L = _lib.lib
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p)
    auto = C.c_uint64(_lib.PETIT_SOLUTION_AUTO)
    shape, bad = _lib.PETIT_ERROR_PROBLEM_SHAPE, _lib.PETIT_ERROR_BAD_ARGUMENT
    NV = _lib.CXX_DTYPE_FP4_E2M1
    h = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, NV, _lib.CXX_DTYPE_BF16, 0)

    def ex(E=8, m=4, n=256, k=256, a_idx=p, a_rows=4, c_idx=p, c_rows=4, c=p, a=p, offsets=p):
        return L.petit_gemm_fp4_fp16_moe_ex(c, a, p, p, p, offsets, E, m, n, k, a_idx, a_rows, c_idx, c_rows, C.byref(h), auto, None, None)

    assert ex(c=None) == shape and ex(a=None) == shape and ex(offsets=None) == shape     # null pointers
    assert ex(E=0) == shape and ex(E=_lib.PETIT_MOE_MAX_EXPERTS + 1) == shape
    assert ex(n=24) == shape and ex(k=384) == shape
    assert ex(a_idx=None, a_rows=3) == shape and ex(c_idx=None, c_rows=3) == shape     # identity needs rows >= m
    assert ex(a_rows=(1 << 32) // 512, k=256) == shape                                # a_rows * k * 2 >= 2^32
    assert ex(a_rows=(1 << 31) // 512 + 1, k=256) == shape                            # ... and past 2^31, the kernels' out-of-range marker
    assert ex(a_rows=(1 << 31) // 512 + 1, k=256, m=0) == shape                      # (checked before the empty problem returns)
    assert ex(a_rows=1 << 20, k=256, m=0) == _lib.PETIT_OK

    ws = L.petit_moe_align_workspace_bytes
    assert ws(1, 8, 256) == 0 and ws(128, 8, 256) == 0                                  # one chunk of 1024 entries: one launch, no scratch
    assert ws(129, 8, 256) == 2 * 256 * 4 and ws(4096, 8, 1024) == 32 * 1024 * 4
    assert ws(4, 0, 8) == 0 and ws(4, 8, 0) == 0

    def align(T=4, topk=2, E=8, ids=p, off=p, sp=p, ti=p, w=p):
        return L.petit_moe_align(ids, 0, T, topk, E, off, sp, ti, w, None)

    assert align(topk=0) == shape
    assert align(E=0) == shape and align(E=_lib.PETIT_MOE_MAX_EXPERTS + 1) == shape
    assert align(ids=None) == shape and align(off=None) == shape and align(sp=None) == shape and align(ti=None) == shape
    assert align(T=1 << 20, topk=1 << 12) == shape                                      # T * topk >= 2^31
    assert align(T=4096, topk=8, w=None) == shape                                       # several chunks need the workspace

    def combine(T=4, topk=2, n=256, E=8, dtype=_lib.CXX_DTYPE_BF16, out=p, slot=p, w=p, ids=p):
        return L.petit_moe_combine(out, slot, w, ids, 0, T, topk, n, E, dtype, None)

    assert combine(topk=0) == shape and combine(E=0) == shape and combine(E=_lib.PETIT_MOE_MAX_EXPERTS + 1) == shape
    assert combine(n=12) == shape and combine(n=0) == shape
    assert combine(out=None) == shape and combine(slot=None) == shape and combine(w=None) == shape and combine(ids=None) == shape
    assert combine(dtype=_lib.PETIT_DTYPE_FP32) == bad
    assert combine(T=0, out=None) == _lib.PETIT_OK                                      # nothing to do


def test_fused_ops_meta_shapes():
    import petit_kernel  # noqa: F401
    from petit_kernel import compiled
    assert compiled.available(), compiled.why_unavailable()
    ops = torch.ops.petit_kernel
    E, n, k, m = 8, 256, 512, 12
    a = torch.empty(5, k, dtype=torch.bfloat16, device="meta")
    b = torch.empty(E * n // 16, 2 * k, dtype=torch.int32, device="meta")
    s = torch.empty(E * n, k // 16, dtype=torch.uint8, device="meta")
    gs = torch.empty(E, dtype=torch.float32, device="meta")
    off = torch.empty(E + 1, dtype=torch.int32, device="meta")
    idx = torch.empty(m, dtype=torch.int32, device="meta")
    c = ops.mul_nvfp4_a16_moe_indexed(a, b, s, gs, off, m, n, k, E, idx, None, -1, -1, None, 1)
    assert c.shape == (m, n // 2) and c.dtype == torch.bfloat16 and c.device.type == "meta"
    c = ops.mul_mxfp4_a16_moe_indexed(a.half(), b, s, gs, off, m, n, k, E, None, idx, 40, -1, None, 0)
    assert c.shape == (40, n) and c.dtype == torch.float16
    ids = torch.empty(6, 4, dtype=torch.int64, device="meta")
    sp, offs, ti = ops.moe_align_device(ids, E)
    assert sp.shape == (24,) and ti.shape == (24,) and offs.shape == (E + 1,) and sp.dtype == offs.dtype == ti.dtype == torch.int32
    out = ops.moe_combine(torch.empty(24, n, dtype=torch.bfloat16, device="meta"), torch.empty(6, 4, device="meta"), ids, E)
    assert out.shape == (6, n) and out.dtype == torch.bfloat16


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_numpy_align_and_combine_restatements_match_the_cpu_layer(seed):
    """On valid ids the align definition is moe_align (CPU tensors), and the combine definition is fp4_moe's torch combine to within one
    rounding of the 16-bit output."""
    from petit_kernel.moe import moe_align
    rng = np.random.default_rng(seed)
    T, topk, E = int(rng.integers(1, 300)), int(rng.choice([1, 2, 8])), int(rng.choice([1, 8, 128]))
    ids = rng.integers(0, E, (T, topk)).astype(np.int32)
    sp, off, ti = align_np(ids, E)
    sorted_idx, offsets = moe_align(torch.from_numpy(ids), E)
    assert np.array_equal(sp, sorted_idx.numpy()) and np.array_equal(off, offsets.numpy())
    assert np.array_equal(ti, (sorted_idx // topk).numpy())

    H = 64
    slot = torch.randn(T * topk, H).to(torch.bfloat16)
    w = torch.rand(T, topk)
    ref = (slot.float() * w.reshape(-1)[:, None]).view(T, topk, H).sum(dim=1).to(torch.bfloat16)
    got = _to16_bits(combine_np(slot.float().numpy(), w.numpy(), ids, E), True)
    d = np.abs(got.astype(np.int32) - ref.view(torch.int16).numpy().view(np.uint16).astype(np.int32))
    assert d.max() <= 1


# --- on the GPU -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pk():
    import petit_kernel
    assert torch.cuda.is_available()
    assert torch.cuda.get_device_properties(0).gcnArchName.startswith("gfx950")
    return petit_kernel


def _u16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _ids_random(rng, T, topk, E):
    return np.stack([rng.choice(E, topk, replace=False) if E >= topk else rng.integers(0, E, topk) for _ in range(T)]).astype(np.int32)


@pytest.mark.gpu
def test_moe_align_device_equals_moe_align(pk):
    from petit_kernel.moe import moe_align
    rng = np.random.default_rng(5)
    cases = []
    for E in (1, 8, 128, 256, 1024):
        for T, topk in ((1, 1), (1, 8), (7, 2), (128, 8), (129, 8), (4096, 8)):
            cases.append((_ids_random(rng, T, topk, E), E))
    cases.append((np.full((300, 4), 5, np.int32), 8))                                 # every row on one expert
    cases.append((rng.integers(1, 7, (200, 2)).astype(np.int32), 8))                  # empty first and last experts
    cases.append((np.full((2048, 2), 0, np.int32), 16))                               # two chunks, one expert
    for ids, E in cases:
        for dt in (torch.int32, torch.int64):
            idd = torch.from_numpy(ids).to(dt).to(DEV)
            sp, off, ti = pk.moe_align_device(idd, E)
            ref_idx, ref_off = moe_align(idd, E)
            assert torch.equal(off, ref_off), (ids.shape, E)
            assert torch.equal(sp.long(), ref_idx), (ids.shape, E)
            assert torch.equal(ti.long(), ref_idx // ids.shape[1])
    # -1 (and other out-of-range) ids: the numpy definition
    for T, topk, E in ((1, 8, 8), (100, 8, 64), (3000, 4, 256)):
        ids = _ids_random(rng, T, topk, E)
        ids[rng.random(ids.shape) < 0.3] = -1
        ids[0, 0] = E                                                                  # out of range the other way
        for dt in (torch.int32, torch.int64):
            sp, off, ti = pk.moe_align_device(torch.from_numpy(ids).to(dt).to(DEV), E)
            rsp, roff, rti = align_np(ids, E)
            assert np.array_equal(sp.cpu().numpy(), rsp) and np.array_equal(off.cpu().numpy(), roff) and np.array_equal(ti.cpu().numpy(), rti)


def _moe_form_ids(pk, h, E, m, n, k):
    ids = set()
    for mm in (1, 2, 4, 8, 16, 64, 512):
        ids.update(pk.ops.get_fp4_solutions(h, mm, n, k))
    return sorted(i for i in ids if pk.moe_resolve_solution(h, E, m, n, k, i))


def _indexed(pk, kind):
    return pk.mul_nvfp4_a16_moe_indexed if kind == "nv" else pk.mul_mxfp4_a16_moe_indexed


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["nv", "mx"])
@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("regime", ["decode", "tiled"])
def test_gathered_and_scattered_bit_identical_to_plain_launch(pk, kind, is_bf16, regime):
    """For every id with a MoE form: gate_up on gathered rows (a_row_index) equals the plain launch on index_select'ed rows, with SiLU-mul
    and bias on and off; down with scattered rows (c_row_index) equals the plain launch's rows index_copy'd into slot order, and the slots
    of unrouted entries stay untouched."""
    from petit_kernel.moe import moe_align
    E, n, k = 8, 256, (2048 if regime == "decode" else 768)
    T, topk = (3, 2) if regime == "decode" else (200, 2)
    rng = np.random.default_rng(hash((kind, is_bf16, regime)) % 1000)
    dt = torch.bfloat16 if is_bf16 else torch.float16
    ex = Experts(pk, kind, E, n, k, 31)
    ids = _ids_random(rng, T, topk, E)
    sorted_idx, off = moe_align(torch.from_numpy(ids).to(DEV), E)
    m = T * topk
    tok = (sorted_idx // topk).int()
    x = torch.randn(T, k, device=DEV).to(dt)
    xg = x.index_select(0, sorted_idx // topk)
    bias = (torch.randn(E, n, device=DEV) * 0.5).to(dt)
    h = _hints(pk, kind, is_bf16)
    sids = _moe_form_ids(pk, h, E, m, n, k)
    assert sids
    fn = _indexed(pk, kind)
    # scatter target: three routed entries made unrouted (ids -1): their slots keep the sentinel
    drop = [0, m // 2, m - 1]
    c_idx = sorted_idx.int().clone()
    for r in drop:
        c_idx[r] = -1
    dropped_slots = sorted_idx[drop].cpu()
    for sid in sids:
        for act, b in ((None, None), ("silu_mul", bias)):
            if act and pk.moe_resolve_solution(h, E, m, n, k, sid, "silu_mul") == 0:
                continue
            plain = ex.mul(pk, xg, off, m, sid, bias=b, activation=act)
            got = fn(x, ex.b, ex.sp, ex.gsd, off, m, n, k, E, a_row_index=tok, solution_id=sid, bias=b, activation=act)
            assert torch.equal(plain.view(torch.int16), got.view(torch.int16)), f"gathered: id {sid:#x}, act {act}"
        plain = ex.mul(pk, xg, off, m, sid)
        out = torch.full((m, n), -7.0, dtype=dt, device=DEV)
        fn(xg, ex.b, ex.sp, ex.gsd, off, m, n, k, E, c_row_index=c_idx, solution_id=sid, out=out)
        want = torch.full((m, n), -7.0, dtype=dt, device=DEV)
        keep = torch.tensor([r for r in range(m) if r not in drop], device=DEV)
        want.index_copy_(0, sorted_idx[keep], plain[keep])
        assert torch.equal(out.view(torch.int16), want.view(torch.int16)), f"scattered: id {sid:#x}"
        assert (out[dropped_slots.to(DEV)] == -7.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("T,topk,E,H", [(1, 8, 256, 7168), (33, 2, 8, 4096), (700, 8, 128, 2048)])
def test_combine_bit_identical_to_numpy(pk, is_bf16, T, topk, E, H):
    rng = np.random.default_rng(T)
    dt = torch.bfloat16 if is_bf16 else torch.float16
    ids = _ids_random(rng, T, topk, E)
    ids[rng.random(ids.shape) < 0.2] = -1
    slot = torch.randn(T * topk, H, device=DEV).to(dt)
    w = torch.rand(T, topk, device=DEV)
    for idt in (torch.int32, torch.int64):
        idd = torch.from_numpy(ids).to(idt).to(DEV)
        a = pk.moe_combine(slot, w, idd, E)
        b = pk.moe_combine(slot, w, idd, E)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
        ref = _to16_bits(combine_np(slot.float().cpu().numpy(), w.cpu().numpy(), ids, E), is_bf16)
        assert np.array_equal(_u16(a), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 16, 256])
@pytest.mark.parametrize("kind", ["nvfp4", "mxfp4"])
def test_fp4_moe_fused_end_to_end(pk, kind, T):
    """Within test_fp4_moe_end_to_end's budget of the f64 layer, and within one bf16 ulp of fp4_moe per element; int64 ids and bf16 router
    weights are accepted."""
    E, topk, hid, inter = 8, 2, 1024, 512
    w13, w2 = _make_layer(pk, kind[:2], E, hid, inter, 40 + T)
    x = torch.randn(T, hid, generator=torch.Generator().manual_seed(T)).to(torch.bfloat16)
    tw, tid = _routing(T, E, topk, T)
    args = (x.to(DEV), w13.b, w13.sp, w13.gsd, w2.b, w2.sp, w2.gsd)
    out = pk.fp4_moe_fused(*args, tw.to(DEV), tid.to(DEV), kind)
    base = pk.fp4_moe(*args, tw.to(DEV), tid.to(DEV), kind)
    torch.cuda.synchronize()
    assert out.shape == (T, hid) and out.dtype == torch.bfloat16
    ref = _layer_ref(x.view(torch.int16).numpy().view(np.uint16), w13, w2, tw.numpy().astype(np.float64), tid.numpy())
    err = out.float().cpu().numpy().astype(np.float64) - ref
    assert np.sqrt(np.mean(err ** 2)) / np.sqrt(np.mean(ref ** 2)) <= 1e-2
    ulp = np.abs(_u16(out).astype(np.int32) - _u16(base).astype(np.int32))
    assert ulp.max() <= 1
    out64 = pk.fp4_moe_fused(*args, tw.to(torch.bfloat16).to(DEV), tid.long().to(DEV), kind)
    ref16 = pk.fp4_moe_fused(*args, tw.to(torch.bfloat16).float().to(DEV), tid.to(DEV), kind)
    assert torch.equal(out64.view(torch.int16), ref16.view(torch.int16))


@pytest.mark.gpu
def test_fp4_moe_fused_skips_unrouted_entries(pk):
    """-1 ids contribute nothing: the layer equals fp4_moe with those entries' weights set to zero (routed to any expert)."""
    E, topk, hid, inter, T = 8, 4, 1024, 512, 40
    w13, w2 = _make_layer(pk, "nv", E, hid, inter, 3)
    x = torch.randn(T, hid, device=DEV).to(torch.bfloat16)
    tw, tid = _routing(T, E, topk, 9)
    mask = torch.rand(T, topk, generator=torch.Generator().manual_seed(1)) < 0.3
    args = (x, w13.b, w13.sp, w13.gsd, w2.b, w2.sp, w2.gsd)
    out = pk.fp4_moe_fused(*args, tw.to(DEV), torch.where(mask, -1, tid).to(DEV), "nvfp4")
    base = pk.fp4_moe(*args, torch.where(mask, 0.0, tw).to(DEV), tid.to(DEV), "nvfp4")
    torch.cuda.synchronize()
    assert np.abs(_u16(out).astype(np.int32) - _u16(base).astype(np.int32)).max() <= 1


@pytest.mark.gpu
def test_fp4_moe_fused_graph_replay_with_changing_routing(pk):
    """fp4_moe_fused captured once under torch.cuda.graph (one capture stream, no parallel branches) and replayed with three routings, one
    of them with -1 entries: each replay is bit-identical to the eager call."""
    E, topk, hid, inter, T = 8, 2, 1024, 512, 16
    w13, w2 = _make_layer(pk, "nv", E, hid, inter, 77)
    x = torch.randn(T, hid, device=DEV).to(torch.bfloat16)
    tw0, tid0 = _routing(T, E, topk, 0)
    sx, stw, stid = x.clone(), tw0.to(DEV), tid0.to(DEV)

    def layer(xx, ww, ii):
        return pk.fp4_moe_fused(xx, w13.b, w13.sp, w13.gsd, w2.b, w2.sp, w2.gsd, ww, ii, "nvfp4")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        layer(sx, stw, stid)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = layer(sx, stw, stid)
    torch.cuda.synchronize()
    tw3, tid3 = _routing(T, E, topk, 13)
    tid3[::3, 1] = -1
    routings = [_routing(T, E, topk, 11), (torch.ones(T, topk) * 0.5, torch.tensor([[3, 5]] * T, dtype=torch.int32)), (tw3, tid3)]
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


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["decode", "tiled"])
def test_out_of_range_indices_read_zeros_and_drop_stores(pk, regime):
    """A indices outside [0, a_rows) (negative or too large) read zero rows; C indices outside [0, c_rows) store nothing.  The output sits
    between guard rows that must stay untouched.  (Safe by construction: the A descriptor bounds every load and every C store is checked.)"""
    E, n, k = 4, 256, 2048 if regime == "decode" else 768
    m = 4 if regime == "decode" else 160
    ex = Experts(pk, "nv", E, n, k, 12)
    off = torch.tensor([0, m // 4, m // 2, 3 * m // 4, m], dtype=torch.int32, device=DEV)
    a_rows = 7
    x = torch.randn(a_rows, k, device=DEV).to(torch.bfloat16)
    rng = np.random.default_rng(2)
    a_idx = rng.integers(0, a_rows, m).astype(np.int32)
    a_idx[::3] = a_rows
    a_idx[1::5] = -1
    a_idx[2::7] = 1 << 30
    xg = torch.zeros(m, k, dtype=torch.bfloat16, device=DEV)
    ok = (a_idx >= 0) & (a_idx < a_rows)
    xg[torch.from_numpy(np.nonzero(ok)[0]).to(DEV)] = x[torch.from_numpy(a_idx[ok]).long().to(DEV)]
    plain = ex.mul(pk, xg, off, m)
    got = pk.mul_nvfp4_a16_moe_indexed(x, ex.b, ex.sp, ex.gsd, off, m, n, k, E, a_row_index=torch.from_numpy(a_idx).to(DEV))
    assert torch.equal(plain.view(torch.int16), got.view(torch.int16))

    c_rows, guard = m, 16
    buf = torch.full((guard + c_rows + guard, n), 3.0, dtype=torch.bfloat16, device=DEV)
    out = buf[guard:guard + c_rows]
    c_idx = np.arange(m, dtype=np.int32)[::-1].copy()
    c_idx[::2] = [-1, c_rows, 1 << 30, -(1 << 30)] * (len(c_idx[::2]) // 4) + [-1] * (len(c_idx[::2]) % 4)
    pk.mul_nvfp4_a16_moe_indexed(xg, ex.b, ex.sp, ex.gsd, off, m, n, k, E, c_row_index=torch.from_numpy(c_idx).to(DEV), out=out)
    torch.cuda.synchronize()
    assert (buf[:guard] == 3.0).all() and (buf[guard + c_rows:] == 3.0).all()
    live = np.nonzero((c_idx >= 0) & (c_idx < c_rows))[0]
    want = torch.full((c_rows, n), 3.0, dtype=torch.bfloat16, device=DEV)
    want[torch.from_numpy(c_idx[live]).long().to(DEV)] = plain[torch.from_numpy(live).to(DEV)]
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
